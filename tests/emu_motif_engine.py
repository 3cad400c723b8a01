"""Test helper: EmuFollowWideEngine (tests/emu_follow_wide_engine.py) plus HipScanner.motif_census, backed by the host emulation of
the motif census kernel (tests/emu_motif_driver.py): `--pattern auto` and topsicle_amd.motif without a GPU."""
import emu_motif_driver as emum
from emu_follow_wide_engine import EmuFollowWideEngine


class EmuMotifEngine(EmuFollowWideEngine):
    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(EmuMotifEngine())
        return hs[j]

    def motif_census(self, slot, u_min=4, u_max=32, lo=0, hi=1000, min_len=0, want_counts=False):
        return emum.motif_census(self._seqs(self.slots[slot]), u_min, u_max, lo, hi, min_len, want_counts)

    def upload_nib4(self, slot, nib, src, desc, n_words):
        """A BAM batch: expanded by the host restatement of the device's expansion kernel, then an ordinary packed upload."""
        from topsicle_amd import seqio
        seq2, inv, desc = seqio.pack_nib4_host(nib, src, desc, n_words)
        self.upload_packed(slot, seq2, inv if (desc["flags"] & 1).any() else None, desc)
