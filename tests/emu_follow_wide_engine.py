"""Test helper: EmuWideEngine (tests/emu_wide_engine.py) plus HipScanner.kmer_followers_wide, backed by the host emulation of the
wide followers kernel (tests/emu_follow_wide_driver.py)."""
import emu_follow_wide_driver as emuf
from emu_wide_engine import EmuWideEngine
from topsicle_amd import hiplib


class EmuFollowWideEngine(EmuWideEngine):
    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(EmuFollowWideEngine())
        return hs[j]

    def kmer_followers_wide(self, slot, n_fwd, follow, lo=100, hi=2000, min_len=0, want_hist=True):
        if not self.wide:
            raise hiplib.TopsicleHipError("tps_batch_kmer_followers_wide needs a table set with tps_set_patterns_wide")
        return emuf.followers_wide(self.patterns, self._seqs(self.slots[slot]), n_fwd, follow, lo, hi, min_len, want_hist)
