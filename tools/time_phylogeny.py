#!/usr/bin/env python3
"""Device time of neighbour joining beside average linkage on the same points, the numpy restatement on
the host, and what `dafs --phylogeny` adds to a run.

  python tools/time_phylogeny.py [--n 512 2048 8192] [--ref-up-to 2048] [--no-c3] [--out profiles/<name>.json]

Per N: random points in the unit square, their Euclidean distances as the float64 matrix of Context.nj_tree and
1 - d / max(d) as the float32 matrix of Context.linkage_tree("average").  Warm context, the last of three calls: the
milliseconds of k_nj_init, k_nj_rowsum, k_nj_pick and k_nj_update summed over their launches (HIP events of the library's stage
recorder, which brackets every launch), the seconds of the whole nj_tree call with the recorder off, and the same two for the
linkage call.  Up to --ref-up-to rows the seconds of tests/nj_ref.py on the host, and whether the device's tree equals it to
the byte.  c3: the command line on random_set(128, 150) (bench.py's c3), wall-clock of the whole process with and without
--phylogeny, the second of two runs each.  Prints one JSON line per measurement (and writes them to --out)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch  # before the library, as in bench.py: both then share one HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from dafs_amd import capi, synth  # noqa: E402
from nj_ref import nj_ref  # noqa: E402

NJ_KERNELS = ("k_nj_init", "k_nj_rowsum", "k_nj_pick", "k_nj_update")
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")


def timed(ctx, call, kernels):
    """(seconds of the whole call with the recorder off, {kernel: [ms, launches]} with it on); the last of three calls each"""
    for _ in range(3):
        t0 = time.perf_counter()
        out = call()
        t_call = time.perf_counter() - t0
    ctx.stage_timing(True)
    try:
        for _ in range(3):
            ctx.stage_report()
            call()
            st = ctx.stage_report()
    finally:
        ctx.stage_timing(False)
    return out, t_call, {k: [round(st[k][0], 4), int(st[k][2])] for k in kernels if k in st}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512, 2048, 8192])
    ap.add_argument("--ref-up-to", type=int, default=2048)
    ap.add_argument("--no-c3", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)
        if a.out:  # after every line: a run that is cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("".join(json.dumps(x) + "\n" for x in lines))

    torch.cuda.init()
    ctx = capi.Context(0)
    try:
        for n in a.n:
            pts = np.random.default_rng(n).random((n, 2))
            dist = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
            sim = (1.0 - dist / dist.max()).astype(np.float32)
            tree, t_nj, k_nj = timed(ctx, lambda: ctx.nj_tree(dist), NJ_KERNELS)
            _, t_avg, k_avg = timed(ctx, lambda: ctx.linkage_tree("average", sim), ("k_linkage_init", "k_linkage_joins"))
            line = dict(what="Context.nj_tree beside Context.linkage_tree('average') on the same points; warm context, last of three calls; "
                             "kernels: [ms over all launches, launches]",
                        n=n, nj_call_s=round(t_nj, 4), nj_kernels=k_nj, nj_kernels_ms=round(sum(v[0] for v in k_nj.values()), 3),
                        average_call_s=round(t_avg, 4), average_kernels=k_avg, negative_lengths=int((tree[2] < 0).sum()))
            if n <= a.ref_up_to:
                t0 = time.perf_counter()
                want = nj_ref(dist)
                line["nj_ref_host_s"] = round(time.perf_counter() - t0, 3)
                line["equals_restatement"] = all(np.asarray(x).tobytes() == y.tobytes() for x, y in zip(tree, want))
            emit(line)
    finally:
        ctx.close()
    if not a.no_c3:
        recs = synth.random_set(128, 150)
        with tempfile.TemporaryDirectory() as tmp:
            fa, nwk = os.path.join(tmp, "c3.fa"), os.path.join(tmp, "c3.nwk")
            with open(fa, "w") as fh:
                fh.write(synth.to_fasta(recs))
            secs, outs = {}, {}
            for name, extra in (("plain", []), ("phylogeny", ["--phylogeny", nwk])):
                for _ in range(2):
                    t0 = time.perf_counter()
                    r = subprocess.run([DAFS] + extra + [fa], capture_output=True, text=True, timeout=900)
                    secs[name] = round(time.perf_counter() - t0, 3)
                    assert r.returncode == 0, r.stderr
                    outs[name] = r.stdout
            emit(dict(what="dafs on c3 (random_set(128, 150)), wall-clock of the whole process, second of two runs", rows=len(recs),
                      plain_s=secs["plain"], with_phylogeny_s=secs["phylogeny"], same_stdout=outs["plain"] == outs["phylogeny"],
                      newick_bytes=os.path.getsize(nwk)))
    return 0 if all(x.get("equals_restatement", True) and x.get("same_stdout", True) for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
