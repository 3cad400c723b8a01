"""Test helper: EmuMotifEngine (tests/emu_motif_engine.py) plus HipScanner.variant_census, backed by the host emulation of the
variant census kernel (tests/emu_variant_driver.py): `--variants` and batch.Job(variants=...) without a GPU."""
import emu_variant_driver as emuv
from emu_motif_engine import EmuMotifEngine


class EmuVariantEngine(EmuMotifEngine):
    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(EmuVariantEngine())
        return hs[j]

    def variant_census(self, slot, unit, tails, begin, end, bin=500, n_bins=40, want_profile=True):
        self.__dict__.setdefault("variant_calls", []).append(slot)
        return emuv.variant_census(self._seqs(self.slots[slot]), unit, tails, begin, end, bin, n_bins, want_profile)
