"""Test helper: EmuVariantEngine (tests/emu_variant_engine.py) plus HipScanner.tract_map, backed by the host emulation of the tract
map kernel (tests/emu_tract_driver.py): `--tracts` and batch.Job(tracts=...) without a GPU."""
import emu_tract_driver as emut
from emu_variant_engine import EmuVariantEngine


class EmuTractEngine(EmuVariantEngine):
    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(EmuTractEngine())
        return hs[j]

    def tract_map(self, slot, unit, block=64, min_hits=20, gap=1, min_blocks=2, max_tracts=8):
        self.__dict__.setdefault("tract_calls", []).append(slot)
        return emut.tract_map(self._seqs(self.slots[slot]), unit, block, min_hits, gap, min_blocks, max_tracts)
