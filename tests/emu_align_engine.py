"""Test helper: EmuPlaceEngine (tests/emu_place_engine.py) plus HipScanner.align_windows, backed by the host emulation of the banded
alignment kernel (tests/emu_align_driver.py): `--ends --anchor --consensus`, and `--endref` on what it wrote, without a GPU."""
import emu_align_driver as emul
from emu_place_engine import EmuPlaceEngine


class EmuAlignEngine(EmuPlaceEngine):
    def helper(self, j):
        hs = self.__dict__.setdefault("_helpers", [])
        while len(hs) <= j:
            hs.append(EmuAlignEngine())
        return hs[j]

    def align_windows(self, codes, length, ref_codes, ref_length, ref, centre, span, cols=True, pile_row=None, n_pile=0):
        self.__dict__.setdefault("align_calls", []).append((len(length), len(ref_length), n_pile))
        return emul.window_align(codes, length, ref_codes, ref_length, ref, centre, span, cols, pile_row, n_pile)
