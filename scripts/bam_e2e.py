"""File -> results rates of the same reads as BGZF FASTQ and as unaligned BAM on one MI355X (README / DESIGN section 7), and an A/B of
the BAM device route (tps_batch_upload_nib4: 4-bit codes expanded by tps_pack_kernel_nib4) against host packing (tps_pack_nib4 +
tps_batch_upload_packed).  Sets: BASELINE config 2 (10 000 x 15 kb, CCCTAA, k = 4) and a log-normal WGS-like set (few telomeric reads).
The kernel time per batch comes from a separate run under `rocprofv3 --kernel-trace --stats` (--quick: one pass of the BAM route).

    python scripts/bam_e2e.py [--quick] [--out DIR]
"""
import argparse
import json
import os
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from topsicle_amd import allsteps, batch, hiplib, seqio, synth  # noqa: E402

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CODE4 = np.zeros(256, np.uint8)
for _i, _c in enumerate(b"=ACMGRSVTWYHKDBN"):
    CODE4[_c] = _i


def _block(data):
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    c = co.compress(data) + co.flush()
    head = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", len(c) + 25)
    return head + c + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))


def write_bgzf(path, data):
    """bgzip's layout: 65280-byte blocks of text, deflate level 6 (compressed on a thread pool: zlib lets go of the GIL)."""
    chunks = [data[i:i + 65280] for i in range(0, len(data), 65280)]
    with ThreadPoolExecutor(16) as ex, open(path, "wb") as fh:
        for b in ex.map(_block, chunks, chunksize=64):
            fh.write(b)
        fh.write(EOF_BLOCK)


def fastq_text(bases, offsets):
    raw = bases.tobytes()
    out = []
    for i in range(len(offsets) - 1):
        s = raw[offsets[i]:offsets[i + 1]]
        out.append(b"@%08x-0000-4000-8000-000000000000\n%s\n+\n%s\n" % (i, s, b"5" * len(s)))
    return b"".join(out)


def ubam_bytes(bases, offsets):
    text = b"@HD\tVN:1.6\tSO:unknown\n@RG\tID:r\tPL:ONT\n"
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", 0)]
    codes = CODE4[bases]
    for i in range(len(offsets) - 1):
        c = codes[offsets[i]:offsets[i + 1]]
        L = len(c)
        if L & 1:
            c = np.append(c, 0)
        packed = ((c[0::2] << 4) | c[1::2]).astype(np.uint8).tobytes()
        name = b"%08x-0000-4000-8000-000000000000\x00" % i
        aux = b"RGZr\x00"
        body = struct.pack("<iiBBHHHiiii", -1, -1, len(name), 255, 4680, 0, 4, L, -1, -1, 0) + name + packed + b"\x14" * L + aux
        out.append(struct.pack("<i", len(body)) + body)
    return b"".join(out)


class HostPacked:
    """The host route of the A/B: a context whose nib4 uploads are packed on the host (tps_pack_nib4) and uploaded packed."""

    def __init__(self, sc):
        self._sc = sc

    def __getattr__(self, k):
        return getattr(self._sc, k)

    def upload_nib4(self, slot, nib, src, desc, n_words):
        seq2, inv, d = seqio.pack_nib4_host(nib, src, desc, n_words)
        self._sc.upload_packed(slot, seq2, inv if (d["flags"] & 1).any() else None, d)


def run(engines, path, pats, prm):
    pool = batch.EnginePool(engines, pats, two_pass="off")
    t0 = time.perf_counter()
    nb = npass = 0
    for pb, res, _s, _r, _w in pool.scan_file(path, prm):
        nb += pb.n_bases
        npass += int(res["pass"].sum())
    return nb, npass, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="one pass of the BAM route per set (the rocprofv3 run)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    motif = "CCCTAA"
    pats = allsteps.patterns_to_search(motif, 4)
    prm = hiplib.make_params(min_len=9000, min_count=allsteps.min_count_for_cutoff(0.7, 1000 / 6, 1000))
    sets = {}
    b, o, _ = synth.make_reads(10000, 15000, motif, 20250920)
    sets["config2_10000x15kb"] = (b, o)
    rng = np.random.default_rng(7)
    lens = np.clip(rng.lognormal(np.log(12000), 0.7, 12000), 200, 200000).astype(np.int64)
    tb, to, _ = synth.make_reads(len(lens), int(lens.max()), motif, 11, telomeric_fraction=0.01)
    parts = [tb[to[i]:to[i] + lens[i]] for i in range(len(lens))]
    wb = np.concatenate(parts)
    wo = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    sets["wgs_lognormal_12000"] = (wb, wo)
    scs = [hiplib.HipScanner(0) for _ in range(2)]
    for s in scs:
        s.set_patterns(pats)
    results = {}
    with tempfile.TemporaryDirectory() as d:
        for name, (bb, oo) in sets.items():
            fq, bam = os.path.join(d, name + ".fastq.gz"), os.path.join(d, name + ".bam")
            write_bgzf(fq, fastq_text(bb, oo))
            write_bgzf(bam, ubam_bytes(bb, oo))
            r = {"bases": int(oo[-1]), "reads": len(oo) - 1, "fastq_gz_bytes": os.path.getsize(fq), "bam_bytes": os.path.getsize(bam)}
            routes = [("bam_device", scs, bam)] if a.quick else [("bgzf_fastq", scs, fq), ("bam_device", scs, bam),
                                                                   ("bam_host_pack", [HostPacked(s) for s in scs], bam)]
            run(scs, bam, pats, prm)                       # warm-up: page cache, pinned pools, plans
            for route, engines, path in routes:
                best = None
                for _ in range(1 if a.quick else 3):
                    nb, npass, t = run(engines, path, pats, prm)
                    best = t if best is None else min(best, t)
                r[route] = {"s": round(best, 4), "bases_per_s": float("%.3g" % (nb / best)), "passing": npass}
            results[name] = r
            print(json.dumps({name: r}), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bam_e2e.json"), "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
