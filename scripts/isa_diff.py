#!/usr/bin/env python3
"""Compare the gfx950 assembly of every kernel group between two source trees (no GPU needed).

A refactor that is meant to leave the kernels' machine code alone is proven here: each of the TPS_KGROUPS translation units
is compiled to assembly with the build's own flags, once from OLD_SRC_DIR and once from the tree's csrc, and the two files
are compared line by line after the `__hip_cuid_<hash>` symbol (a hash of the source text) is replaced by a fixed word.

  usage: scripts/isa_diff.py OLD_SRC_DIR [--groups 1,2] [--cache DIR] [--define TPS_STAMPS] [--out FILE] [-j N]

OLD_SRC_DIR: the csrc directory of an older revision, inside a copy of that revision's tree (the sources include
../../include/topsicle_hip.h), e.g.
    mkdir /tmp/old && git archive HEAD~1 topsicle_amd/csrc include | tar -x -C /tmp/old
    scripts/isa_diff.py /tmp/old/topsicle_amd/csrc
--cache: keep the assembly files there (old_g<N>.s, new_g<N>.s); an old_g<N>.s that is already present is not compiled again.
Prints one line per group (`group 3: identical` or `group 3: 17 differing lines`) and exits 1 if any group differs."""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KGROUPS = 18         # = TPS_KGROUPS in csrc/tps_kernels.h
FLAGS = ["--offload-arch=gfx950", "-O3", "-fno-vectorize", "-std=c++17", "-fPIC", "-Wno-unused-variable"]


def compile_isa(src, group, out, defines):
    cmd = ["/opt/rocm/bin/hipcc"] + FLAGS + [f"-D{d}" for d in defines] + \
          [f"-DTPS_KGROUP={group}", "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-S", "-o", out,
           os.path.join(src, "tps_kernels.hip" if group else "topsicle_hip.hip")]
    p = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if p.returncode:
        raise RuntimeError(f"hipcc failed on group {group} of {src}:\n{p.stderr[-4000:]}")
    return out


def normalised(path):
    return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", open(path).read()).split("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old_src")
    ap.add_argument("--new-src", default=os.path.join(ROOT, "topsicle_amd", "csrc"))
    ap.add_argument("--groups", default=",".join(str(g) for g in range(KGROUPS)))
    ap.add_argument("--cache", default="")
    ap.add_argument("--define", action="append", default=[])
    ap.add_argument("--out", default="")
    ap.add_argument("-j", type=int, default=min(8, os.cpu_count() or 1))
    o = ap.parse_args()
    groups = [int(g) for g in o.groups.split(",")]
    tmp = None if o.cache else tempfile.TemporaryDirectory()
    d = o.cache or tmp.name
    os.makedirs(d, exist_ok=True)
    jobs = []
    with concurrent.futures.ThreadPoolExecutor(o.j) as ex:
        for g in groups:
            old = os.path.join(d, f"old_g{g}.s")
            if not (o.cache and os.path.exists(old)):
                jobs.append(ex.submit(compile_isa, o.old_src, g, old, o.define))
            jobs.append(ex.submit(compile_isa, o.new_src, g, os.path.join(d, f"new_g{g}.s"), o.define))
        for j in jobs:
            j.result()
    lines, bad = [], 0
    for g in groups:
        a, b = normalised(os.path.join(d, f"old_g{g}.s")), normalised(os.path.join(d, f"new_g{g}.s"))
        n = sum(1 for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[:1] in "+-" and l[:3] not in ("+++", "---")) if a != b else 0
        bad += n != 0
        lines.append(f"group {g}: " + ("identical" if n == 0 else f"{n} differing lines") + f"  ({len(b)} lines of assembly)")
    head = "# gfx950 assembly of an older csrc against this tree's, per kernel group (scripts/isa_diff.py; hipcc " + \
           " ".join(FLAGS + [f"-D{d}" for d in o.define]) + " -DTPS_KGROUP=<g> --cuda-device-only -S; __hip_cuid_<hash> normalised)\n"
    text = head + "\n".join(lines) + f"\n{len(groups) - bad} of {len(groups)} groups identical\n"
    sys.stdout.write(text)
    if o.out:
        open(o.out, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
