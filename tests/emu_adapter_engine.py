"""Test helper: EmuAnchorEngine (tests/emu_anchor_engine.py) plus HipScanner.adapter_find, backed by the host emulation of the kernel
(tests/emu_adapter_driver.py): `--adapters` and batch.Job(adapters=AdapterSpec(...)) without a GPU."""
import emu_adapter_driver as emuad
from emu_anchor_engine import EmuAnchorEngine


class EmuAdapterEngine(EmuAnchorEngine):
    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(EmuAdapterEngine())
        return hs[j]

    def adapter_find(self, slot, patterns, tails, begin, end):
        self.__dict__.setdefault("adapter_calls", []).append(slot)
        return emuad.adapter_find(self._seqs(self.slots[slot]), patterns, tails, begin, end)
