"""What the read-analysis calls refuse, library against emulation: return code AND message.  Both sides call the same check function
(the feature headers under csrc/; DESIGN.md, "How a read-analysis call is put together"), so tps_last_error has to say what the
emulation's *_last_error says.  The refusal tables are the ones the CPU tests feed the emulation (tests/*_cases.py), on one read of 120
bases; nothing is launched on a refused call."""
import ctypes as C
import re

import numpy as np
import pytest

import adapter_cases as adc
import anchor_cases as ac
import emu_anchor_driver
import emu_driver
import emu_ends_driver
import emu_follow_wide_driver
import emu_motif_driver
import emu_place_driver
import emu_tract_driver
import emu_variant_driver
import ends_cases as ec
import motif_cases as mc
import place_cases as pc
import test_adapter
import test_gpu_adapter
import test_gpu_ends
import test_gpu_ends_anchor
import test_gpu_tract
import test_gpu_variant
import tract_cases as tc
import variant_cases as vc
from topsicle_amd import allsteps, hiplib, variants

pytestmark = pytest.mark.gpu

READ = "ACGT" * 30
SLOT = 3
U6 = variants.unit_code("CCCTAA")[0]
PATS = allsteps.patterns_to_search(telopattern="CCCTAA", cut_length=4)
# the followers calls have no table among the CPU tests: (n_fwd, follow, lo, hi, with a histogram, picks_words and hist_len off by)
FOLLOW = [(0, 2, 100, 2000, True, 0, 0), (len(PATS) // 2 + 1, 2, 100, 2000, True, 0, 0), (3, -1, 100, 2000, True, 0, 0), (3, 2, -1, 2000, True, 0, 0),
          (3, 2, 0, 4097, True, 0, 0), (3, 2, 500, 500, True, 0, 0), (3, 9, 100, 2000, True, 0, 0), (3, 2, 100, 2000, True, 1, 0), (3, 2, 100, 2000, True, 0, -1)]
FOLLOW_NARROW = FOLLOW + [(16, 2, 100, 2000, True, 0, 0)]
FOLLOW_WIDE = FOLLOW + [(33, 2, 100, 2000, True, 0, 0), (3, 2, 100, 2000, False, -1, 0)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _emu(call):
    """(code, message) of an emulation driver's refusal"""
    with pytest.raises(RuntimeError) as e:
        call()
    m = re.fullmatch(r"\w+ rc=(-?\d+): (.*)", str(e.value), re.S)
    assert m, str(e.value)
    return int(m.group(1)), m.group(2)


def _follow_arrays(n_fwd, follow, lo, hi, hist, d_picks, d_hist):
    """stand-ins large enough for every case, and the lengths the call is told"""
    picks, counters = np.zeros(4096, np.uint32), np.zeros(2 * 33 * (4 ** 8 + 1), np.uint64)
    bins = 4 ** follow + 1 if 0 <= follow <= 8 else 1
    return picks, (counters if hist else None), 2 * n_fwd * ((hi - lo + 31) // 32) + d_picks, (2 * n_fwd * bins + d_hist) if hist else 0


def _pairs(sc):
    """(what is asked, the emulation's answer, the library's answer) of every refusal of every call"""
    lib, h = sc.lib, sc._h
    bases, offsets = hiplib.pack_reads([READ])
    for wide, cases in ((False, FOLLOW_NARROW), (True, FOLLOW_WIDE)):
        (sc.set_patterns_wide if wide else sc.set_patterns)(PATS)
        for n_fwd, follow, lo, hi, hist, dp, dh in cases:
            picks, counters, pl, hl = _follow_arrays(n_fwd, follow, lo, hi, hist, dp, dh)
            args = (n_fwd, follow, lo, hi, 0)
            if wide:
                L = emu_follow_wide_driver.lib()
                e = L.emu_followers_wide("".join(PATS).encode(), len(PATS), 4, _p(bases), _p(offsets), C.c_int64(1), *args, 0, _p(picks), C.c_int64(pl),
                                         _p(counters), C.c_int64(hl)), L.emu_follow_wide_last_error().decode()
                g = lib.tps_batch_kmer_followers_wide(h, SLOT, *args, _p(picks), pl, _p(counters), hl), sc._err()
            else:
                L = emu_driver.lib()
                e = L.emu_followers("".join(PATS).encode(), len(PATS), 4, _p(bases), _p(offsets), C.c_int64(1), *args, _p(picks), C.c_int64(pl),
                                    _p(counters), C.c_int64(hl)), L.emu_last_error().decode()
                g = lib.tps_batch_kmer_followers(h, SLOT, *args, _p(picks), pl, _p(counters), hl), sc._err()
            yield ("followers_wide" if wide else "followers", args, dp, dh), e, g
    for kw, _ in mc.REFUSALS:
        with pytest.raises(hiplib.TopsicleHipError) as err:
            sc.motif_census(SLOT, **kw)
        m = re.fullmatch(r"libtopsicle_hip error (-?\d+): (.*)", str(err.value), re.S)
        yield ("motif", kw), _emu(lambda: emu_motif_driver.motif_census([READ], **kw)), (int(m.group(1)), m.group(2))
    for kw, _ in vc.REFUSALS:
        a = dict(dict(code=U6, m=6, tails=[0], begin=[0], end=[100], bin=500, n_bins=40), **kw)
        e = _emu(lambda: emu_variant_driver.variant_census_code([READ], a["code"], a["m"], a["tails"], a["begin"], a["end"], a["bin"], a["n_bins"]))
        yield ("variant", kw), e, (test_gpu_variant._raw_call(sc, slot=SLOT, **a), sc._err())
    for kw, _ in tc.REFUSALS:
        a = dict(dict(code=U6, m=6, block=64, min_hits=20, gap=1, min_blocks=2, max_tracts=8, lens=None), **kw)
        yield ("tract", kw), _emu(lambda: emu_tract_driver.tract_map_code([READ], **a)), (test_gpu_tract._raw_call(sc, slot=SLOT, **a), sc._err())
    for kw, _ in ec.SKETCH_REFUSALS:
        a = dict(dict(code=U6, m=6, tails=[0], begin=[0], end=[100], k=12, buckets=256, lens=None), **kw)
        yield ("sketch", kw), _emu(lambda: emu_ends_driver.end_sketch_code([READ], **a)), (test_gpu_ends._raw_sketch(sc, slot=SLOT, **a), sc._err())
    s = np.arange(128, dtype=np.uint32).reshape(2, 64)
    dg, ln, mt = np.zeros(2, np.int32), np.zeros(2 * 256, np.int32), np.zeros(2 * 256, np.int32)
    for kw, _ in ec.LINK_REFUSALS:
        a = dict(dict(min_match=6, max_links=4, buckets=None, lens=None, n=None), **kw)
        n, b = 2 if a["n"] is None else a["n"], 64 if a["buckets"] is None else a["buckets"]
        sl, dl, ll, tl = a["lens"] if a["lens"] is not None else (n * b, n, n * a["max_links"], n * a["max_links"])
        g = lib.tps_sketch_links(h, _p(s), n, b, sl, a["min_match"], a["max_links"], _p(dg), dl, _p(ln), ll, _p(mt), tl), sc._err()
        yield ("links", kw), _emu(lambda: emu_ends_driver.sketch_links(s, **a)), g
    for kw, _ in ac.WINDOW_REFUSALS:
        a = dict(ac.WINDOW_GOOD, **kw)
        yield ("window", kw), _emu(lambda: emu_anchor_driver.end_window_code([READ], **a)), (test_gpu_ends_anchor._raw_window(sc, slot=SLOT, **a), sc._err())
    codes, keep = np.zeros((2, 7), np.uint32), np.zeros((2, 4), np.uint32)
    out = [np.zeros(4, np.int32) for _ in range(7)]
    for kw, _ in ac.OFFSET_REFUSALS:
        a = dict(ac.OFFSET_GOOD, **kw)
        n = 2 if a["n"] is None else a["n"]
        le, rf = np.array(a["length"], np.int32), np.array(a["ref"], np.int32)
        g = lib.tps_window_offsets(h, _p(codes), _p(keep), _p(le), _p(rf), n, a["span"], a["k"], _p(out[0]), _p(out[1]), _p(out[2]),
                                   n if a["out_len"] is None else a["out_len"]), sc._err()
        yield ("offsets", kw), _emu(lambda: emu_anchor_driver.window_offsets(codes, keep, **a)), g
    r = pc.REFUSAL_ROWS
    for kw, _ in pc.REFUSALS:
        a = dict(pc.GOOD, **kw)
        le, rl = np.array(a["length"], np.int32), np.array(a["ref_length"], np.int32)
        cl, kl, n, rcl, rkl, n_ref, ol = pc.GOOD_LENS if a["lens"] is None else a["lens"]
        g = lib.tps_window_place(h, _p(r["codes"]), cl, _p(r["keep"]), kl, _p(le), n, _p(r["ref_codes"]), rcl, _p(r["ref_keep"]), rkl, _p(rl), n_ref,
                                 a["span"], a["k"], a["max_occ"], *[_p(o) for o in out], ol), sc._err()
        yield ("place", kw), _emu(lambda: emu_place_driver.place_windows(**r, **a)), g
    for kw, _ in adc.REFUSALS:
        yield ("adapter", kw), _emu(lambda: test_adapter._call(**kw)), (test_gpu_adapter._raw(sc, slot=SLOT, **kw), sc._err())


def test_library_and_emulation_refuse_with_the_same_code_and_message():
    with hiplib.HipScanner(0) as sc:
        sc.upload(SLOT, *hiplib.pack_reads([READ]))
        seen = {}
        for what, emu, gpu in _pairs(sc):
            assert emu[0] != 0 and emu[1], what
            assert gpu == emu, what
            seen[what[0]] = seen.get(what[0], 0) + 1
        sc.sync()
    assert seen == dict(followers=len(FOLLOW_NARROW), followers_wide=len(FOLLOW_WIDE), motif=len(mc.REFUSALS), variant=len(vc.REFUSALS), tract=len(tc.REFUSALS),
                        sketch=len(ec.SKETCH_REFUSALS), links=len(ec.LINK_REFUSALS), window=len(ac.WINDOW_REFUSALS), offsets=len(ac.OFFSET_REFUSALS),
                        place=len(pc.REFUSALS), adapter=len(adc.REFUSALS))
