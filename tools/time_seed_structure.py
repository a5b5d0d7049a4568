#!/usr/bin/env python3
"""Time pipeline.add_each with and without the seed's consensus structure, on the set-up of
tools/time_add_each.py.

  python tools/time_seed_structure.py [--out FILE] [K ...]

A 32-row seed of ~120 nt is aligned by a run (family_set(32 + 512, 120)'s first 32 members); the seed's structure is the ss of
that run.  Then K further members (default 32 and 512) are added by add_each, (a) without and (b) with seed_ss.  Each way runs
twice on a warm context of its own, the two alternating, and the second run is reported.  Prints one JSON line per K: the
.seconds parts both ways; the time of the Context.structure_support call over all K placements of (b) (one call per chunk as
add_each makes it, best of three); and, over the placed rows, the mean canonical / both and expected / both both ways -- for
(a) the support of its placements for the same carried structure, which is not the structure (a) prints; and how many of the K
nodes had consensus base pairs, with their mean iteration count.  --out also writes the lines as one JSON list."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dafs_amd import capi, pipeline, synth  # noqa: E402

M, LENGTH, POOL = 32, 120, 512


def _round(d):
    return {k: round(v, 4) for k, v in d.items()}


def _placed_support(seed_names, seed_rows, seed_ss, names, seqs, each):
    """The support of every placement of `each` for the seed's structure carried into its columns, from the stores of a joint
    phase 1 per chunk as add_each builds them: (per-sequence dict of arrays, seconds of the support calls, best of three)."""
    m = len(seed_rows)
    seed_seqs = [r.replace("-", "") for r in seed_rows]
    seed_mask = np.array([[ch != "-" for ch in r] for r in seed_rows], np.uint8)
    cons = [capi.row_constraint(seed_mask[r], seed_ss, seed_seqs[r]) for r in range(m)] if getattr(each, "support", None) is not None else None
    src, ctx = capi.Context(0), capi.Context(0)
    out = {k: [] for k in ("both", "canonical", "half", "expected")}
    best = 0.0
    try:
        src.set_sequences(seed_seqs + seqs)
        src.fold_begin(0.01, constraints=None if cons is None else cons + [None] * len(seqs))
        try:
            src.align_posteriors(capi.ALIGN_PROBCONS, 0.01, 0, m * (m + len(seqs)) - m * (m + 1) // 2, fetch=False)
        finally:
            src.fold_end()
        n = m + 1
        for chunk in each.chunks:
            ctx.families_from(src, [list(range(m)) + [m + j] for j in chunk])
            ctx.consistency_bp(0.25)
            alns, sss = [], []
            for f, j in enumerate(chunk):
                res = each.results[j]
                mask = np.array([[ch != "-" for ch in row] for row in [res.rows[-1]] + res.rows[:-1]], np.uint8)
                alns.append((np.concatenate([[f * n + m], np.arange(f * n, f * n + m)]).astype(np.uint32), mask))
                sss.append(pipeline.carry_structure(seed_ss, np.flatnonzero(res.rf).astype(np.uint32), len(res.rf)))
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                got = ctx.structure_support(alns, sss)
                times.append(time.perf_counter() - t0)
            best += min(times)
            for g in got:
                for k in out:
                    out[k].append(g[k][0])  # the new sequence's row
    finally:
        src.close()
        ctx.close()
    return {k: np.array(v) for k, v in out.items()}, best


def _means(sup):
    has = sup["both"] > 0
    return dict(rows=int(len(has)), rows_with_pairs=int(has.sum()), mean_both=round(float(sup["both"].mean()), 3),
                canonical_per_both=round(float((sup["canonical"][has] / sup["both"][has]).mean()), 4),
                expected_per_both=round(float((sup["expected"][has] / sup["both"][has]).mean()), 4))


def _nodes(each):
    """what the K nodes did: how many had consensus base pairs to couple their subproblems, and the mean iteration count"""
    return dict(with_consensus_pairs=sum(1 for r in each.results if r.dd_log[0][2] > 0), mean_iterations=round(float(each.iterations.mean()), 2))


def main(ks, out):
    recs = synth.family_set(M + POOL, LENGTH, seed=4242)
    names, seqs = [r[0] for r in recs], [r[1] for r in recs]
    seed_run = pipeline.run(names[:M], seqs[:M])
    srows = seed_run.rows
    keep = [c for c in range(len(srows[0])) if any(r[c] != "-" for r in srows)]
    now = {c: k for k, c in enumerate(keep)}
    srows = ["".join(r[c] for c in keep) for r in srows]
    seed_ss = np.array([now[int(seed_run.ss[c])] if seed_run.ss[c] != pipeline.NONE and int(seed_run.ss[c]) in now else pipeline.NONE for c in keep],
                       np.uint32)
    snames = names[:M]
    ctx = capi.Context(0)  # warm-up of every kernel on a small case
    pipeline.add_each(snames, srows, names[M:M + 2], seqs[M:M + 2], ctx=ctx)
    pipeline.add_each(snames, srows, names[M:M + 2], seqs[M:M + 2], ctx=ctx, seed_ss=seed_ss)
    ctx.close()
    lines = []
    for k in ks:
        ca, cb = capi.Context(0), capi.Context(0)
        new_names, new_seqs = names[M:M + k], seqs[M:M + k]
        rec = dict(m=M, k=k, length=LENGTH, seed_columns=len(srows[0]), seed_pairs=int((seed_ss != pipeline.NONE).sum()))
        for _ in range(2):
            a = pipeline.add_each(snames, srows, new_names, new_seqs, ctx=ca)
            b = pipeline.add_each(snames, srows, new_names, new_seqs, ctx=cb, seed_ss=seed_ss)
        ca.close()
        cb.close()
        sup_a, _ = _placed_support(snames, srows, seed_ss, new_names, new_seqs, a)
        sup_b, t_sup = _placed_support(snames, srows, seed_ss, new_names, new_seqs, b)
        assert all(sup_b[key].tobytes() == b.support[key].tobytes() for key in sup_b)  # the tool's stores are add_each's
        rec["a_without"] = dict(seconds=_round(a.seconds), chunks=len(a.chunks), support=_means(sup_a), nodes=_nodes(a))
        rec["b_with_structure"] = dict(seconds=_round(b.seconds), chunks=len(b.chunks), support=_means(sup_b), nodes=_nodes(b),
                                       support_call_seconds=round(t_sup, 5))
        rec["same_rows"] = sum(x.rows == y.rows for x, y in zip(a.results, b.results))
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        if out:
            with open(out, "w") as f:
                json.dump(lines, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    args = sys.argv[1:]
    out = None
    if "--out" in args:
        at = args.index("--out")
        out = args[at + 1]
        del args[at:at + 2]
    main([int(a) for a in args] or [32, 512], out)
