"""Test helper: EmuEndsEngine (tests/emu_ends_engine.py) plus HipScanner.end_window and HipScanner.anchor_offsets, backed by the host
emulation of the two kernels (tests/emu_anchor_driver.py): `--ends --anchor` and batch.Job(ends=EndSpec(anchor=True)) without a GPU."""
import emu_anchor_driver as emua
from emu_ends_engine import EmuEndsEngine


class EmuAnchorEngine(EmuEndsEngine):
    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(EmuAnchorEngine())
        return hs[j]

    def end_window(self, slot, unit, tails, begin, end, k=12, span=2000):
        self.__dict__.setdefault("window_calls", []).append(slot)
        return emua.end_window(self._seqs(self.slots[slot]), unit, tails, begin, end, k, span)

    def anchor_offsets(self, codes, keep, length, ref, span, k=12):
        self.__dict__.setdefault("offset_calls", []).append(len(ref))
        return emua.window_offsets(codes, keep, length, ref, span, k)
