"""Test helper: EmuEngine (tests/emu_engine.py) plus HipScanner.set_patterns_wide, backed by the host emulation of the wide-table
kernel (tests/emu_wide_driver.py).  A narrow table set with set_patterns scans through the narrow emulation as before."""
import emu_wide_driver as emuw
from emu_engine import EmuEngine
from topsicle_amd import hiplib


class EmuWideEngine(EmuEngine):
    def __init__(self):
        super().__init__()
        self.wide = False

    def device_info(self):
        return "host emulation of tps_device.h / tps_wide.h (tests only)"

    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(EmuWideEngine())
        return hs[j]

    def set_patterns(self, patterns):
        super().set_patterns(patterns)
        self.wide = False

    def set_patterns_wide(self, patterns):
        if not patterns:
            raise hiplib.TopsicleHipError("empty pattern list")
        k = len(patterns[0])
        if any(len(p) != k for p in patterns):
            raise hiplib.TopsicleHipError("all patterns of one table must have the same length")
        emuw.table(patterns)                           # (raises for k > 32, P > 64, a non-ACGT letter)
        self.patterns = list(patterns)
        self.wide = True

    def kmer_followers(self, slot, n_fwd, follow, lo=100, hi=2000, min_len=0, want_hist=True):
        if self.wide:
            raise hiplib.TopsicleHipError("tps_batch_kmer_followers does not take a wide pattern table")
        return super().kmer_followers(slot, n_fwd, follow, lo, hi, min_len, want_hist)

    def scan(self, slot, prm):
        if not self.wide:
            return super().scan(slot, prm)
        s = self.slots[slot]
        p = hiplib.Params.from_buffer_copy(prm)
        s["out"] = emuw.scan(self.patterns, self._seqs(s), p, tails=s["tails"])
        s["flags"] = p.flags
