#!/usr/bin/env python3
"""Wall time of a BRAliBase-like set of many small families on one warm context, two ways: a loop of pipeline.run (one
family at a time) and one pipeline.run_batch (all families through shared launches).  Both must give the same outputs.

  python tools/time_batch.py [--families 512] [--out profiles/<name>.json]

The families are synth.family_set / synth.random_set draws of 5-15 sequences of 80-200 nt.  Prints one JSON line (and
writes it to --out): the two wall times and, per way, the device time of every stage kernel (dafs_hip_stage_report).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dafs_amd import capi, pipeline, synth  # noqa: E402


def family_list(count, seed=2024):
    rng = synth.SplitMix64(seed)
    fams = []
    for k in range(count):
        n = 5 + rng.below(11)
        L = 80 + rng.below(121)
        recs = synth.family_set(n, L, seed=seed + 7 * k) if k % 4 else synth.random_set(n, L, seed=seed + 7 * k)
        fams.append(([r[0] for r in recs], [r[1] for r in recs]))
    return fams


def stages(ctx):
    return {k: dict(ms=round(v[0], 3), launches=v[2]) for k, v in sorted(ctx.stage_report().items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", type=int, default=512)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fams = family_list(a.families)
    ctx = capi.Context(0)
    try:
        pipeline.run_batch(fams[:4], ctx=ctx)  # warm: code objects loaded, workspaces allocated
        for nm, sq in fams[:2]:
            pipeline.run(nm, sq, ctx=ctx)
        ctx.stage_timing(True)
        t0 = time.perf_counter()
        loop = [pipeline.run(nm, sq, ctx=ctx).output for nm, sq in fams]
        t_loop = time.perf_counter() - t0
        st_loop = stages(ctx)
        t0 = time.perf_counter()
        res = pipeline.run_batch(fams, ctx=ctx)
        t_batch = time.perf_counter() - t0
        batch = [r.output for r in res]
        dd_memory = res[0].dd_memory  # (reserved, in use, peak) bytes of the resident nodes of the (single) sub-batch
        st_batch = stages(ctx)
        ctx.stage_timing(False)
    finally:
        ctx.close()
    line = dict(what="many-family throughput: loop of pipeline.run against one pipeline.run_batch, warm context",
                families=len(fams), sequences=sum(len(s) for _, s in fams), pairs=sum(len(s) * (len(s) - 1) // 2 for _, s in fams),
                seq_per_family="5-15", length_nt="80-200", loop_s=round(t_loop, 3), batch_s=round(t_batch, 3),
                speedup=round(t_loop / t_batch, 2), outputs_equal=loop == batch,
                phase1_estimate_bytes=sum(pipeline.family_bytes([len(x) for x in sq]) for _, sq in fams),
                sub_batches=len(pipeline.pack_families([pipeline.family_bytes([len(x) for x in sq]) for _, sq in fams], pipeline.DEFAULT_BATCH_BYTES)),
                nodes_reserved_bytes=int(dd_memory[0]), nodes_peak_bytes=int(dd_memory[2]), stages_loop=st_loop, stages_batch=st_batch)
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(s + "\n")
    return 0 if line["outputs_equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
