"""Test helper: EmuRefineEngine (tests/emu_refine_engine.py) plus nib4 uploads (BAM batches, expanded by the host packer) and
HipScanner.mod_profile, backed by the host emulation of the kernel (tests/emu_methyl_driver.py): `--methyl` and
batch.Job(methyl=MethylSpec(...)) without a GPU."""
import emu_methyl_driver as emumt
from emu_refine_engine import EmuRefineEngine
from topsicle_amd import seqio


class EmuMethylEngine(EmuRefineEngine):
    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(EmuMethylEngine())
        return hs[j]

    def upload_nib4(self, slot, nib, src, desc, n_words):
        seq2, inv, d = seqio.pack_nib4_host(nib, src, desc, n_words)
        self.upload_packed(slot, seq2, inv if (d["flags"] & 1).any() else None, d)

    def mod_profile(self, slot, tails, begin, end, origin, mod_off, delta, prob, w=500, nb0=2, nb1=8, hi=205, lo=50):
        self.__dict__.setdefault("methyl_calls", []).append(slot)
        return emumt.mod_profile(self._seqs(self.slots[slot]), tails, begin, end, origin, mod_off, delta, prob, w, nb0, nb1, hi, lo)
