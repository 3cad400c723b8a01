"""Test helper: EmuAnchorEngine (tests/emu_anchor_engine.py) plus HipScanner.place_windows, backed by the host emulation of the
placement kernel (tests/emu_place_driver.py): `--ends --endref` without a GPU."""
import emu_place_driver as emup
from emu_anchor_engine import EmuAnchorEngine


class EmuPlaceEngine(EmuAnchorEngine):
    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(EmuPlaceEngine())
        return hs[j]

    def place_windows(self, codes, keep, length, ref_codes, ref_keep, ref_length, span, k=12, max_occ=16):
        self.__dict__.setdefault("place_calls", []).append((len(length), len(ref_length)))
        return emup.place_windows(codes, keep, length, ref_codes, ref_keep, ref_length, span, k, max_occ)
