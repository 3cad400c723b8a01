"""batch.run_analysis, the one dispatch of the boundary analyses (variants, ends -- with and without the windows --, adapters,
refine), on a stub engine that records its calls and answers with rows made of the regions it was given: which calls are made and
in what order, what is submitted, and what reaches the sink on each of the routes -- the whole batch resident, a subset of it
(second pass of the two-pass route), an empty subset, nothing resident.  And the order of the launches behind one scan."""
import numpy as np
import pytest

import together_cases as tg
from topsicle_amd import adapters, allsteps, batch, ends, hiplib, refine, tracts, variants

N, STORED = 5, [1, 3]                         # five reads; reads 1 and 3 have a boundary the CLI would store: 160 and 400
PRM = hiplib.make_params(window=100, slide=6, trimfirst=100, maxlen=20000)
SEQS = ["ACGTACGTACGTACGTA", "GGGTTTAAACCCGGGTTTAA"]


def results():
    res = np.zeros(N, hiplib.RESULT_DTYPE)
    res["pass"], res["n_win"], res["bkp"] = [1, 1, 0, 1, 1], [50, 50, 50, 50, 0], [-1, 10, 10, 50, 10]
    res["tail"] = [1, 0, 1, 1, 1]             # (the reads without a region are submitted with tail 0 all the same)
    return res


class Stub:
    """Every row it hands out starts with the `end` of the read's region: the read is recognised wherever the row lands."""

    def __init__(self):
        self.calls = []

    def _called(self, name, slot, tails, begin, end, *extra):
        assert all(np.asarray(a).dtype == dt for a, dt in zip((tails, begin, end) + extra, (np.uint8, np.int32, np.int32, np.int32)))
        self.calls.append((name, slot, *(np.asarray(a).tolist() for a in (tails, begin, end) + extra)))
        return np.asarray(end)

    def variant_census(self, slot, unit, tails, begin, end, bin, n_bins):
        e = self._called("variant_census", slot, tails, begin, end)
        return np.tile(e.astype(np.uint32)[:, None], (1, 2 + 4 * len(unit))), np.full((n_bins, 2 + 4 * len(unit)), 77, np.int64)

    def end_sketch(self, slot, unit, tails, begin, end, k, buckets):
        e = self._called("end_sketch", slot, tails, begin, end)
        return np.tile(e.astype(np.uint32)[:, None], (1, buckets)), e.astype(np.uint32) + 1

    def end_window(self, slot, unit, tails, begin, end, k, span):
        e = self._called("end_window", slot, tails, begin, end)
        return np.tile(e.astype(np.uint32)[:, None] + 2, (1, (span + 15) // 16)), np.tile(e.astype(np.uint32)[:, None] + 3, (1, (span + 31) // 32))

    def adapter_find(self, slot, seqs, tails, begin, end):
        e = self._called("adapter_find", slot, tails, begin, end)
        return np.tile(e.astype(np.uint16)[:, None], (1, len(seqs))), np.tile(e.astype(np.uint16)[:, None] + 1, (1, len(seqs)))

    def boundary_refine(self, slot, unit, tails, begin, end, at, hit=2, miss=1, sep=200):
        e = self._called("boundary_refine", slot, tails, begin, end, at)
        rows = np.zeros(len(e), hiplib.REFINE_DTYPE)
        rows["pos"], rows["score"] = e, (hit, miss, sep) == (3, 2, 150)
        return rows


# name -> (the spec, the engine calls in order, the regions of reads 1 and 3: (begin, end[, at]) each)
ANALYSES = {
    "variants": (lambda sink: variants.VariantSpec("CCCTAACCCTAA", 500, 4, sink), ["variant_census"], [(100, 160), (100, 400)]),
    "ends": (lambda sink: ends.EndSpec("CCCTAA", 12, 64, 2000, sink), ["end_sketch"], [(160, 2160), (400, 2400)]),
    "ends_anchor": (lambda sink: ends.EndSpec("CCCTAA", 12, 64, 2000, sink, anchor=True), ["end_sketch", "end_window"], [(160, 2160), (400, 2400)]),
    "adapters": (lambda sink: adapters.AdapterSpec(SEQS, 256, sink), ["adapter_find"], [(0, 256), (0, 256)]),
    "refine": (lambda sink: refine.RefineSpec("CCCTAA", 3, 2, 150, sink), ["boundary_refine"], [(100, 20000, 155), (100, 20000, 395)]),
}
ROUTES = {"resident": (True, None), "subset": (True, STORED), "empty_subset": (True, []), "nothing_resident": (False, None)}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", ANALYSES)
def test_calls_submitted_reads_and_what_the_sink_gets(name, route):
    make, names, regions = ANALYSES[name]
    with_engine, slot_index = ROUTES[route]
    got = []
    spec = make(lambda *a: got.append(a))
    eng, res, recs = Stub(), results(), object()
    batch.run_analysis(spec, PRM, eng if with_engine else None, 3, recs, res, None if slot_index is None else np.array(slot_index, np.int64))
    (g_recs, g_res, *out), = got
    assert g_recs is recs and g_res is res
    # -- the calls: none without resident reads, else each once and in order, on the slot given, with every resident read
    submitted = {"resident": list(range(N)), "subset": STORED}.get(route, [])
    assert [c[0] for c in eng.calls] == (names if submitted else [])
    whole = [regions[STORED.index(i)] if i in STORED else (0,) * len(regions[0]) for i in range(N)]
    for _name, slot, tails, *args in eng.calls:
        assert slot == 3
        assert tails == [int(res["tail"][i]) if i in STORED else 0 for i in submitted]       # tail 0 on an empty region
        assert [list(a) for a in zip(*args)] == [list(whole[i]) for i in submitted]
    # -- the outputs: one row per read of the batch, the stub's where the read was submitted, the empty answer everywhere else
    empty = spec.empty(N)
    per_read = len(empty) - spec.per_batch
    assert len(out) == len(empty) and spec.per_batch == (name == "variants")
    for j, (o, e) in enumerate(zip(out[:per_read], empty)):
        assert len(o) == N and o.dtype == e.dtype and o.shape == e.shape
        for i in range(N):
            key = o[i]["pos"] if o.dtype.names else np.atleast_1d(o[i])[0]
            if i in submitted:
                assert int(key) == whole[i][1] + j, (i, j, key)                              # the stub's j-th output for this read's region
            else:
                assert np.array_equal(o[i], e[i]), i
    if name == "refine":
        assert (out[0]["score"][submitted] == 1).all()                                       # (hit, miss and sep reached the call)
    if spec.per_batch:                                                                       # the profile: as it came, never scattered
        assert out[-1].shape == empty[-1].shape and (out[-1] == (77 if submitted else 0)).all()


def test_empty_answers():
    """What a read without a region gets: zero counts and a zero profile; an empty sketch of no k-mers and all-zero window rows; every
    sequence at its full length, ending at 0; a zero row without a runner-up."""
    sink = None
    counts, profile = ANALYSES["variants"][0](sink).empty(3)
    assert counts.shape == (3, 26) and counts.dtype == np.uint32 and profile.shape == (4, 26) and profile.dtype == np.int64 and not counts.any() and not profile.any()
    sketch, kept, codes, keep = ANALYSES["ends_anchor"][0](sink).empty(3)
    assert (sketch == ends.EMPTY).all() and sketch.shape == (3, 64) and not kept.any() and codes.shape == (3, 125) and keep.shape == (3, 63)
    assert not codes.any() and not keep.any() and len(ANALYSES["ends"][0](sink).empty(3)) == 2
    dist, end = ANALYSES["adapters"][0](sink).empty(3)
    assert dist.tolist() == [[17, 20]] * 3 and dist.dtype == end.dtype == np.uint16 and not end.any()
    rows, = ANALYSES["refine"][0](sink).empty(3)
    assert rows.dtype == hiplib.REFINE_DTYPE and (rows["runner_pos"] == -1).all() and not any(rows[f].any() for f in rows.dtype.names if f != "runner_pos")


def test_launches_behind_one_scan_keep_their_order():
    """variants, ends (the sketch, then the windows), adapters, refine, then the tract map -- whatever order the keywords come in;
    every read of the batch is submitted on the one-pass route."""
    order = []

    def recorded(name, inner):
        def call(self, slot, unit, *a, **kw):
            order.append((name, len(a[0]) if a else None))                     # (the reads submitted; the map takes the whole batch as it is)
            return inner(self, slot, unit, *a, **kw)
        return call
    cls = tg.every_engine()
    Recording = type("Recording", (cls,), {name: recorded(name, getattr(cls, name)) for name in
                                           ("variant_census", "end_sketch", "end_window", "adapter_find", "boundary_refine", "tract_map")})
    reads = tg.ec.detection_reads(tg.IDENT)[0][:9]
    recs = [type("R", (), {"seq": s, "id": f"read{i}"})() for i, s in enumerate(reads)]
    sink = lambda *a: None                     # noqa: E731
    job = batch.Job(allsteps.patterns_to_search(telopattern="CCCTAA", cut_length=4), hiplib.make_params(min_len=5000, min_count=100),
                    tracts=tracts.TractSpec("CCCTAA", sink=sink), refine=ANALYSES["refine"][0](sink), adapters=ANALYSES["adapters"][0](sink),
                    ends=ANALYSES["ends_anchor"][0](sink), variants=ANALYSES["variants"][0](sink))
    assert job.analyses == [job.variants, job.ends, job.adapters, job.refine]
    batch.scan_jobs(Recording(), recs, [job])
    assert order == [("variant_census", 9), ("end_sketch", 9), ("end_window", 9), ("adapter_find", 9), ("boundary_refine", 9), ("tract_map", None)]
