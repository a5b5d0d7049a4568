#!/usr/bin/env python3
"""Time dafs_hip_alignment_identity and dafs_hip_alignment_weights on a warm context.

  python tools/time_alistat.py [--out FILE] [c3] [synthetic] [synthetic_nr] [add_each]

c3: the final alignment of random_set(128, 150) (bench.py's c3): nearest rows and both matrices.
synthetic: a 10 000 x 300 alignment (a random ancestor, 30 % of the cells redrawn, 30 % gaps, 5 % N): nearest rows only.
synthetic_nr: the same with the redundancy bits at 0.9 and the non-redundant subset.
add_each: 32 new sequences against a 32-row seed with nearest=True, beside the same call without it.
After a warm-up call every measurement is taken three times: wall-clock per call and the device time of each kernel (stage
timing).  Prints one JSON line per input; with --out also writes the list to FILE (profiles/r15_a_time_alistat.json is one)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dafs_amd import capi, pipeline, synth  # noqa: E402

REPEATS = 3
TI, TJ = 16, 64  # the tile of k_ali_pairs (alistat.hip)


def synthetic(n=10000, length=300, seed=61):
    rs = np.random.RandomState(seed)
    cell = np.tile(rs.randint(0, 4, length), (n, 1))
    redraw = rs.rand(n, length) < 0.3
    cell[redraw] = rs.randint(0, 4, int(redraw.sum()))
    draw = rs.rand(n, length)
    cell[draw < 0.30] = 5
    cell[(draw >= 0.30) & (draw < 0.35)] = 4
    return cell.astype(np.uint8)


def tiles(n):
    """(tiles of the triangle passes, those that leave at the diagonal test)"""
    bi, bj = (n + TI - 1) // TI, (n + TJ - 1) // TJ
    leave = sum(1 for i in range(bi) for j in range(bj) if j * TJ + TJ - 1 <= i * TI)
    return bi * bj, leave


def timed(ctx, cell, nr=None, matrix=False):
    first = ctx.alignment_identity(cell, nr=nr, matrix=matrix)  # warm-up
    w_first = ctx.alignment_weights(cell)
    ctx.stage_timing(True)
    ctx.stage_report()
    walls, walls_w, walls_sel = [], [], []
    for _ in range(REPEATS):
        t = time.perf_counter()
        r = ctx.alignment_identity(cell, nr=nr, matrix=matrix)
        walls.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter()
        w = ctx.alignment_weights(cell)
        walls_w.append((time.perf_counter() - t) * 1e3)
        assert r.nearest.tobytes() == first.nearest.tobytes() and w.tobytes() == w_first.tobytes()
        if nr is not None:
            t = time.perf_counter()
            kept, _ = capi.nr_select(r.red, np.arange(len(cell), dtype=np.uint32))
            walls_sel.append((time.perf_counter() - t) * 1e3)
    st = ctx.stage_report()
    ctx.stage_timing(False)
    kern = {k: dict(ms_per_call=v[0] / REPEATS, longest_ms=v[1], launches_per_call=v[2] // REPEATS) for k, v in st.items() if k.startswith("k_ali_")}
    n, length = cell.shape
    pairs = n * (n - 1) // 2
    total, leave = tiles(n)
    out = dict(n=n, columns=length, row_pairs=pairs, nr=nr, matrix=matrix, identity_wall_ms=[round(x, 3) for x in walls],
               weights_wall_ms=[round(x, 3) for x in walls_w], kernels=kern, tiles=total, tiles_leaving_at_the_diagonal=leave,
               share_leaving=round(leave / total, 4))
    near = kern.get("k_ali_pairs<nearest>")
    if near and near["ms_per_call"] > 0:
        out["nearest_row_pairs_per_s"] = pairs / (near["ms_per_call"] * 1e-3)
        out["nearest_cell_comparisons_per_s"] = pairs * length / (near["ms_per_call"] * 1e-3)
    if nr is not None:
        out["nr_select_wall_ms"] = [round(x, 3) for x in walls_sel]
        out["kept"] = int(kept.sum())
    return out


def add_each_config(ctx):
    recs = synth.family_set(64, 100, seed=62)
    names, seqs = [r[0] for r in recs], [r[1] for r in recs]
    seed = pipeline.run(names[:32], seqs[:32], ctx=ctx)
    walls = {}
    for nearest in (False, True):
        pipeline.add_each(names[:32], seed.rows, names[32:], seqs[32:], ctx=ctx, nearest=nearest)  # warm-up
        w = []
        for _ in range(REPEATS):
            t = time.perf_counter()
            each = pipeline.add_each(names[:32], seed.rows, names[32:], seqs[32:], ctx=ctx, nearest=nearest)
            w.append(round(time.perf_counter() - t, 4))
        walls[nearest] = w
    return dict(config="add_each", seed_rows=32, hits=32, wall_s_without=walls[False], wall_s_with_nearest=walls[True],
                mean_pid_to_nearest=float(np.nanmean(each.nearest.pid)))


def main(args):
    out = None
    if "--out" in args:
        out = args[args.index("--out") + 1]
        args = args[:args.index("--out")] + args[args.index("--out") + 2:]
    results = []
    ctx = capi.Context(0)
    for cfg in args or ["c3", "synthetic", "synthetic_nr", "add_each"]:
        if cfg == "c3":
            recs = synth.random_set(128, 150, seed=12345)
            res = pipeline.run([r[0] for r in recs], [r[1] for r in recs], ctx=ctx)
            r = dict(config="c3", **timed(ctx, capi.encode_cells(res.rows), matrix=True))
        elif cfg == "synthetic":
            r = dict(config="synthetic", **timed(ctx, synthetic()))
        elif cfg == "synthetic_nr":
            r = dict(config="synthetic_nr", **timed(ctx, synthetic(), nr=0.9))
        else:
            r = add_each_config(ctx)
        results.append(r)
        print(json.dumps(r), flush=True)
    ctx.close()
    if out:
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
