#!/usr/bin/env python3
"""Time dafs_hip_alignment_compare on a warm context.

  python tools/time_compare.py [--out FILE] [c3] [synthetic] [synthetic_matrix] [pp]

c3: the final alignment of random_set(128, 150) (bench.py's c3) against the alignment of a second run with -r 1, with the pair
matrices.  synthetic: two 10 000 x 300 / 307 alignments of the same sequences (30 % gaps, the test alignment with half of the
rows' gaps drawn again and the others shifted), without the matrices; synthetic_matrix: the same with them.  After a warm-up
call every measurement is taken three times: wall-clock per call and the device time of each kernel (stage timing).
pp: family_set(32, 120) aligned with reliability, compared with the alignment its generator implies (synth does not expose one,
so: with a second run refined by -r 1): residues, pairs and accuracy per PP class.
Prints one JSON line per input; with --out also writes the list to FILE (profiles/r16_a_time_compare.json is one)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dafs_amd import capi, pipeline, stockholm, synth  # noqa: E402

REPEATS = 3
TI, TJ = 16, 64  # the tile of k_cmp_pairs (compare.hip)


def synthetic(n=10000, length=300, seed=61):
    rs = np.random.RandomState(seed)
    cell_r = np.full((n, length), 5, np.uint8)
    cell_t = np.full((n, length + 7), 5, np.uint8)
    for r in range(n):
        at = np.nonzero(rs.rand(length) >= 0.30)[0]
        codes = rs.randint(0, 4, len(at))
        cell_r[r, at] = codes
        if r % 2:
            cell_t[r, np.sort(rs.choice(length + 7, len(at), replace=False))] = codes
        else:
            cell_t[r, at + np.where(np.arange(len(at)) < len(at) // 2, 0, rs.randint(0, 8))] = codes
    return cell_r, cell_t


def timed(ctx, cell_r, cell_t, matrix, **kw):
    first = ctx.alignment_compare(cell_r, cell_t, matrix=matrix, **kw)  # warm-up
    ctx.stage_timing(True)
    ctx.stage_report()
    walls = []
    for _ in range(REPEATS):
        t = time.perf_counter()
        r = ctx.alignment_compare(cell_r, cell_t, matrix=matrix, **kw)
        walls.append((time.perf_counter() - t) * 1e3)
        assert r.shared.tobytes() == first.shared.tobytes()
    st = ctx.stage_report()
    ctx.stage_timing(False)
    kern = {k: dict(ms_per_call=v[0] / REPEATS, longest_ms=v[1], launches_per_call=v[2] // REPEATS) for k, v in st.items() if k.startswith("k_cmp_")}
    n, len_r = cell_r.shape
    bi, bj = (n + TI - 1) // TI, (n + TJ - 1) // TJ
    computed = sum(1 for i in range(bi) for j in range(bj) if not j * TJ + TJ - 1 <= i * TI)
    out = dict(n=n, columns_ref=len_r, columns_test=cell_t.shape[1], matrix=matrix, wall_ms=[round(x, 3) for x in walls], kernels=kern,
               sps=r.sps, ppv=r.ppv, tc=r.tc, tiles=bi * bj, tiles_computed=computed)
    pairs = kern.get("k_cmp_pairs<shared>")
    if pairs and pairs["ms_per_call"] > 0:  # every computed tile compares 16 x 64 row pairs over all columns
        out["key_comparisons_per_s"] = computed * TI * TJ * len_r / (pairs["ms_per_call"] * 1e-3)
    return out, r


def main(args):
    out = None
    if "--out" in args:
        out = args[args.index("--out") + 1]
        args = args[:args.index("--out")] + args[args.index("--out") + 2:]
    results = []
    ctx = capi.Context(0)
    for cfg in args or ["c3", "synthetic", "synthetic_matrix", "pp"]:
        if cfg == "c3":
            recs = synth.random_set(128, 150, seed=12345)
            names, seqs = [r[0] for r in recs], [r[1] for r in recs]
            a = pipeline.run(names, seqs, ctx=ctx)
            b = pipeline.run(names, seqs, ctx=ctx, t_max=100)  # a second run: fewer iterations per node
            r = dict(config="c3", **timed(ctx, capi.encode_cells(b.rows), capi.encode_cells(a.rows), True, ss_ref=b.ss, ss_test=a.ss)[0])
        elif cfg in ("synthetic", "synthetic_matrix"):
            cell_r, cell_t = synthetic()
            r = dict(config=cfg, **timed(ctx, cell_r, cell_t, cfg == "synthetic_matrix")[0])
        else:
            recs = synth.family_set(32, 120, seed=63)
            names, seqs = [r[0] for r in recs], [r[1] for r in recs]
            a = pipeline.run(names, seqs, ctx=ctx, reliability=True)
            b = pipeline.run(names, seqs, ctx=ctx, t_max=100)
            pp = [None] * len(a.rows)
            for i, (row, rel) in enumerate(zip(a.rows, a.reliability["residue"])):
                chars = iter([stockholm.pp_char(p) for p in rel])
                pp[i] = "".join("." if ch == "-" else next(chars) for ch in row)
            got = ctx.alignment_compare(b.rows, a.rows, pp=capi.encode_pp(pp))
            r = dict(config="pp", n=len(names), reference="a second run with t_max=100 (synth exposes no alignment)", sps=got.sps, ppv=got.ppv,
                     classes={capi.PP_CLASSES[q]: dict(residues=int(got.pp_residues[q]), ref=int(got.pp_ref[q]), shared=int(got.pp_shared[q]),
                                                       accuracy=None if got.pp_ref[q] == 0 else float(got.pp_accuracy[q])) for q in range(11)})
        results.append(r)
        print(json.dumps(r), flush=True)
    ctx.close()
    if out:
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
