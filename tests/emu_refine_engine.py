"""Test helper: EmuAdapterEngine (tests/emu_adapter_engine.py) plus HipScanner.boundary_refine, backed by the host emulation of the
kernel (tests/emu_refine_driver.py): `--refine` and batch.Job(refine=RefineSpec(...)) without a GPU."""
import emu_refine_driver as emurf
from emu_adapter_engine import EmuAdapterEngine


class EmuRefineEngine(EmuAdapterEngine):
    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(EmuRefineEngine())
        return hs[j]

    def boundary_refine(self, slot, unit, tails, begin, end, at, hit=2, miss=1, sep=200):
        self.__dict__.setdefault("refine_calls", []).append(slot)
        return emurf.boundary_refine(self._seqs(self.slots[slot]), unit, tails, begin, end, at, hit, miss, sep)
