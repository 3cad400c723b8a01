"""bench.py --dump-outputs: the size plan (no GPU: shapes only)."""
import bench
from topsicle_amd import hiplib


def _bound(n_reads, sizes, prm, m):
    nw = hiplib.window_count(prm.maxlen, prm.window, prm.slide, prm.trimfirst, prm.maxlen)
    total = 0
    for P in sizes:
        total += m * (8 * (len(bench.DUMP_RESULT_FIELDS) + 1) + 2 * P * 4)
        total += min(n_reads, bench.DUMP_SUMS_READS) * (8 + nw * 4) + min(n_reads, bench.DUMP_RAW_READS) * (8 + nw * P * 4)
    return total


def test_dump_plan_keeps_every_read_while_it_fits_and_samples_beyond():
    prm = hiplib.make_params(window=100, slide=6, trimfirst=100, maxlen=20000, flags=31)
    for n_reads, sizes in ((10000, [12]), (10000, [12, 12, 12]), (25000, [14]), (400000, [12, 12, 12]), (3000000, [12])):
        m = bench.dump_plan(n_reads, sizes, prm)
        assert min(n_reads, bench.DUMP_SUMS_READS) <= m <= n_reads
        assert _bound(n_reads, sizes, prm, m) <= bench.DUMP_LIMIT_BYTES, (n_reads, sizes)
        if m < n_reads:                              # as many as fit: one more read would not
            assert _bound(n_reads, sizes, prm, m + 1) > bench.DUMP_LIMIT_BYTES
    assert bench.dump_plan(10000, [12, 12, 12], prm) == 10000         # config5 at its own size: every read
    assert bench.dump_plan(400000, [12, 12, 12], prm) < 400000
