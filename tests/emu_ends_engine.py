"""Test helper: EmuVariantEngine (tests/emu_variant_engine.py) plus HipScanner.end_sketch and HipScanner.sketch_links, backed by the
host emulation of the two kernels (tests/emu_ends_driver.py): `--ends` and batch.Job(ends=...) without a GPU."""
import emu_ends_driver as emue
from emu_variant_engine import EmuVariantEngine


class EmuEndsEngine(EmuVariantEngine):
    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(EmuEndsEngine())
        return hs[j]

    def end_sketch(self, slot, unit, tails, begin, end, k=12, buckets=256):
        self.__dict__.setdefault("sketch_calls", []).append(slot)
        return emue.end_sketch(self._seqs(self.slots[slot]), unit, tails, begin, end, k, buckets)

    def sketch_links(self, sketch, min_match=6, max_links=32):
        self.__dict__.setdefault("link_calls", []).append(len(sketch))
        return emue.sketch_links(sketch, min_match, max_links)
