#!/usr/bin/env python3
"""Device time of the bootstrap of the neighbour-joining tree: the batched joins (k_nj_batch, one
workgroup per replicate) against the same call with the replicates sent one by one through the kernels of section 22, one tree
through either form, and what `dafs --phylogeny-bootstrap` adds to a run.

  python tools/time_bootstrap.py [--n 128 512 2048] [--replicates 100] [--no-c3] [--out profiles/<name>.json]

Per n: n = 128 is the c3 alignment (pipeline.run on random_set(128, 150)), the other sizes are synthetic rows of 300 columns
that differ from one ancestor in a fifth of their cells.  Model jc.  Warm context, the last of three calls: the milliseconds of
k_boot_pack, k_boot_dist and k_nj_batch (or k_nj_init .. k_nj_update) summed over their launches (HIP events of the library's
stage recorder), the seconds of the whole alignment_bootstrap call with the recorder off, the number of fix-up entries, and the
seconds of dafs_host_tree_support alone on the replicate trees.  Both forms must return the same arrays.  One tree: nj_tree
(the kernels of section 22) beside nj_trees of the one matrix (k_nj_batch).  c3: the command line with and without
--phylogeny-bootstrap, wall-clock of the whole process, the second of two runs each.  Prints one JSON line per measurement
(and writes them to --out)."""
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
from dafs_amd import capi, pipeline, synth  # noqa: E402

KERNELS = ("k_boot_pack", "k_boot_dist", "k_nj_batch", "k_nj_init", "k_nj_rowsum", "k_nj_pick", "k_nj_update")
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
SWITCH = "DAFS_NJ_BATCH_MAX_N"


def timed(ctx, call):
    """(result, seconds of the whole call with the recorder off, {kernel: [ms, launches]} with it on); the last of three each"""
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
    return out, t_call, {k: [round(st[k][0], 4), int(st[k][2])] for k in KERNELS if k in st}


def looped(call):
    """call() with the batched form switched off"""
    os.environ[SWITCH] = "0"
    try:
        return call()
    finally:
        del os.environ[SWITCH]


def synthetic_rows(n, columns=300):
    rng = np.random.default_rng(n)
    ancestor = rng.integers(0, 4, columns)
    return np.where(rng.random((n, columns)) < 0.2, rng.integers(0, 4, (n, columns)), ancestor[None, :]).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[128, 512, 2048])
    ap.add_argument("--replicates", type=int, default=100)
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
    B = a.replicates
    try:
        for n in a.n:
            if n == 128:
                recs = synth.random_set(128, 150)
                cell = capi.encode_cells(pipeline.run([r[0] for r in recs], [r[1] for r in recs], ctx=ctx).rows)
                rows = "c3"
            else:
                cell, rows = synthetic_rows(n), "synthetic"
            tree = ctx.alignment_tree(cell)
            call = lambda: ctx.alignment_bootstrap(cell, B=B, tree=tree, trees=True)  # noqa: E731
            got, t_batched, k_batched = timed(ctx, call)
            fixups = int(capi.bootstrap_fixups())
            want, t_looped, k_looped = looped(lambda: timed(ctx, call))
            t0 = time.perf_counter()
            support = capi.tree_support(tree[0], tree[1], got[1], got[2])
            t_support = time.perf_counter() - t0
            emit(dict(what="Context.alignment_bootstrap, model jc: batched joins against %s=0 (the replicates one by one through the kernels "
                           "of one tree); warm context, last of three calls; kernels: [ms over all launches, launches]" % SWITCH,
                      n=n, columns=int(cell.shape[1]), rows=rows, replicates=B, batched_call_s=round(t_batched, 4), batched_kernels=k_batched,
                      looped_call_s=round(t_looped, 4), looped_kernels=k_looped, fixups=fixups, host_support_s=round(t_support, 4),
                      same_arrays=all(x.tobytes() == y.tobytes() for x, y in zip(got, want)), same_support=bool((support == got[0]).all()),
                      splits_at_95_percent=int((got[0] * 100 >= 95 * B).sum()), splits=int((got[0] >= 0).sum())))
            if n <= 512:  # one tree through either form
                pts = np.random.default_rng(n).random((n, 2))
                dist = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
                one, t_one, k_one = timed(ctx, lambda: ctx.nj_tree(dist))
                bat, t_bat, k_bat = timed(ctx, lambda: ctx.nj_trees(dist[None]))
                emit(dict(what="one tree: Context.nj_tree (k_nj_pick and k_nj_update per join) beside Context.nj_trees of the one matrix "
                               "(k_nj_batch); warm context, last of three calls", n=n, nj_tree_call_s=round(t_one, 5), nj_tree_kernels=k_one,
                          nj_trees_call_s=round(t_bat, 5), nj_trees_kernels=k_bat,
                          same_arrays=all(np.asarray(x).tobytes() == y[0].tobytes() for x, y in zip(one, bat))))
    finally:
        ctx.close()
    if not a.no_c3:
        recs = synth.random_set(128, 150)
        with tempfile.TemporaryDirectory() as tmp:
            fa, nwk = os.path.join(tmp, "c3.fa"), os.path.join(tmp, "c3.nwk")
            with open(fa, "w") as fh:
                fh.write(synth.to_fasta(recs))
            secs, outs = {}, {}
            for name, extra in (("plain", ["--phylogeny", nwk]), ("bootstrap", ["--phylogeny", nwk, "--phylogeny-bootstrap", str(B)])):
                for _ in range(2):
                    t0 = time.perf_counter()
                    r = subprocess.run([DAFS] + extra + [fa], capture_output=True, text=True, timeout=900)
                    secs[name] = round(time.perf_counter() - t0, 3)
                    assert r.returncode == 0, r.stderr
                    outs[name] = r.stdout
            emit(dict(what="dafs --phylogeny on c3 (random_set(128, 150)) without and with --phylogeny-bootstrap, wall-clock of the whole "
                           "process, second of two runs", rows=len(recs), replicates=B, phylogeny_s=secs["plain"], with_bootstrap_s=secs["bootstrap"],
                      same_stdout=outs["plain"] == outs["bootstrap"]))
    return 0 if all(x.get("same_arrays", True) and x.get("same_support", True) and x.get("same_stdout", True) for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
