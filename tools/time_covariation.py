#!/usr/bin/env python3
"""Time dafs_hip_alignment_covariation_null on a warm context.

  python tools/time_covariation.py [--out FILE] [--null shuffle|tree] ... [c3] [synthetic]

c3: the final alignment of random_set(128, 150) (bench.py's c3) with 100 shuffles, beside the wall-clock of the whole c3 run.
synthetic: a 512 x 12 000 code matrix (a random ancestor, 30 % of the cells redrawn, 10 % non-nucleotides) with 10 shuffles.
After a warm-up call the annotation is taken three times: wall-clock per call and the device time of each of its kernels
(stage timing).  --null (default shuffle; may be given several times: every null is timed on the same inputs in one job)
chooses the null.  Under tree the default tree is built inside the call: its identity and linkage kernels are reported as
default_tree_kernels, and default_tree_wall_ms is the wall-clock of the call less that of the same call with the tree passed in.
Prints one JSON line per input and null and writes the list to FILE (default profiles/r10_a_time_covariation.json)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dafs_amd import capi, pipeline, synth  # noqa: E402

REPEATS = 3


def synthetic(n=512, length=12000, seed=51):
    rs = np.random.RandomState(seed)
    code = np.tile(rs.randint(0, 4, length), (n, 1))
    redraw = rs.rand(n, length) < 0.3
    code[redraw] = rs.randint(0, 4, int(redraw.sum()))
    code[rs.rand(n, length) < 0.1] = 4
    return code.astype(np.uint8)


def timed(ctx, code, ss, shuffles, null="shuffle"):
    first = ctx.alignment_covariation(code, ss, shuffles=shuffles, null=null)  # warm-up
    ctx.stage_timing(True)
    ctx.stage_report()
    walls = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        r = ctx.alignment_covariation(code, ss, shuffles=shuffles, null=null)
        walls.append((time.perf_counter() - t) * 1e3)
        assert r["best_e"].tobytes() == first["best_e"].tobytes() and r["col_sum"].tobytes() == first["col_sum"].tobytes()
    st = ctx.stage_report()
    ctx.stage_timing(False)
    per = lambda keep: {k: dict(ms_per_call=v[0] / REPEATS, longest_ms=v[1], launches_per_call=v[2] // REPEATS) for k, v in st.items() if keep(k)}
    n, length = code.shape
    out = dict(null=null, n=n, columns=length, column_pairs=length * (length - 1) // 2, shuffles=shuffles, wall_ms=[round(w, 3) for w in walls],
               kernels=per(lambda k: k.startswith("k_cov_")), pairs_e_le_005=int((first["pair_e"][ss != capi.NONE] <= 0.05).sum()) if ss is not None else None,
               columns_best_e_le_005=int((first["best_e"] <= 0.05).sum()))
    if null == "tree":  # the default tree's share: its kernels, and the call without it (the same tree passed in)
        out["default_tree_kernels"] = per(lambda k: k.startswith(("k_ali_", "k_linkage_")))
        ident = ctx.alignment_identity(np.where(code == 4, 5, code).astype(np.uint8), matrix=True, nearest=False)
        iu = np.triu_indices(n, 1)
        sim = np.zeros((n, n), np.float32)
        both = ident.aligned[iu]
        sim[iu] = np.where(both > 0, ident.ident[iu].astype(np.float64) / np.maximum(both, 1).astype(np.float64), 0.0).astype(np.float32)
        _, left, right = ctx.linkage_tree("average", sim)
        given = []
        for _ in range(REPEATS + 1):
            t = time.perf_counter()
            r = ctx.alignment_covariation(code, ss, shuffles=shuffles, null=null, tree=(left, right))
            given.append((time.perf_counter() - t) * 1e3)
            assert r["best_e"].tobytes() == first["best_e"].tobytes()
        out["wall_tree_given_ms"] = [round(w, 3) for w in given[1:]]
        out["default_tree_wall_ms"] = round(min(walls) - min(given[1:]), 3)
    return out


def main(args):
    out = os.path.join(ROOT, "profiles", "r10_a_time_covariation.json")
    if "--out" in args:
        out = args[args.index("--out") + 1]
        args = args[:args.index("--out")] + args[args.index("--out") + 2:]
    nulls = []
    while "--null" in args:
        nulls.append(args[args.index("--null") + 1])
        args = args[:args.index("--null")] + args[args.index("--null") + 2:]
    results = []
    ctx = capi.Context(0)
    for cfg in args or ["c3", "synthetic"]:
        if cfg == "c3":
            recs = synth.random_set(128, 150, seed=12345)
            names, seqs = [r[0] for r in recs], [r[1] for r in recs]
            pipeline.run(names, seqs, ctx=ctx)  # warm-up of the run itself
            t0 = time.perf_counter()
            res = pipeline.run(names, seqs, ctx=ctx)
            head = dict(config="c3", run_s=round(time.perf_counter() - t0, 3), consensus_pairs=int((res.ss != capi.NONE).sum()))
            code, ss, shuffles = capi.encode_alignment(res.rows), res.ss, 100
        else:
            head, code, ss, shuffles = dict(config="synthetic"), synthetic(), None, 10
        for null in nulls or ["shuffle"]:
            r = dict(head)
            if cfg == "c3":
                t0 = time.perf_counter()
                pipeline.run(names, seqs, ctx=ctx, covariation=dict(null=null))
                r["run_with_covariation_s"] = round(time.perf_counter() - t0, 3)
            r.update(timed(ctx, code, ss, shuffles, null))
            results.append(r)
            print(json.dumps(r), flush=True)
    ctx.close()
    with open(out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
