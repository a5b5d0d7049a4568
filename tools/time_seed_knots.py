#!/usr/bin/env python3
"""What a pseudoknotted seed structure costs and gives when sequences are added, on the planted H-type
family of tools/time_levels.py (planted_family: two crossing stems of 6 pairs, no indels).

  python tools/time_seed_knots.py [--out profiles/<name>.json] [--members 64] [--seed-rows 8]

A seed of the family's first --seed-rows members is built by pipeline.run with decoder "Levels" at -G 2,4; the rest is added by
pipeline.add_each.  Three arms alternate in one job, each on a warm context of its own, and the second run of each is reported:
  (a) no structure;
  (b) the seed's level 0 only -- today's seed_ss, the plain constrained fold and k_bp_compact;
  (c) both levels -- seed_ss with seed_level, one fold per level and k_bp_compact_levels.
Per arm: add_each's .seconds (phase 1, nodes, total), the nodes' mean iteration count, the stage recorder's device times of the
compaction kernels in a fold of the source context's sequences as the arm folds them, and expected / both of the placed rows at
stem A's and at stem B's planted pairs separately (Context.structure_support on a structure holding that stem alone, carried
into each placement's columns, from the stores of the arm's own phase 1).  Prints one JSON line; --out writes it too."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dafs_amd import capi, pipeline  # noqa: E402
from time_levels import planted_family  # noqa: E402

NONE, FREE = pipeline.NONE, 0xFF
THS = (1.0 / 3.0, 1.0 / 5.0)


def _round(d):
    return {k: round(float(v), 4) for k, v in d.items()}


def _stem(columns, pairs, col_of):
    """a structure over `columns` columns holding the planted pairs (residue indices of the first seed row) alone"""
    ss = np.full(columns, NONE, np.uint32)
    for i, j in pairs:
        ss[col_of[i]] = col_of[j]
    return ss


def _arm_constraints(arm, seed_mask, seed_seqs, ss, level):
    if arm == "a":
        return None
    if arm == "b":
        ss0 = np.where(level == 0, ss, NONE).astype(np.uint32)
        return [capi.row_constraint(seed_mask[r], ss0, seed_seqs[r]) for r in range(len(seed_seqs))]
    K = int(level[level != FREE].max()) + 1 if (level != FREE).any() else 1
    return [capi.row_constraint_levels(seed_mask[r], ss, level, K, seed_seqs[r]) for r in range(len(seed_seqs))]


def _stems_support(arm, seed_rows, ss, level, seqs, each, stems):
    """per stem the mean expected / both over the placed rows, from a phase 1 as the arm's add_each runs it, and the compaction
    kernels' device times of that phase 1's fold"""
    m = len(seed_rows)
    seed_seqs = [r.replace("-", "") for r in seed_rows]
    seed_mask = np.array([[ch != "-" for ch in r] for r in seed_rows], np.uint8)
    cons = _arm_constraints(arm, seed_mask, seed_seqs, ss, level)
    src, ctx = capi.Context(0), capi.Context(0)
    out = {name: [] for name in stems}
    try:
        src.set_sequences(seed_seqs + seqs)
        src.stage_timing(True)
        src.stage_report()
        src.fold_begin(0.01, constraints=None if cons is None else cons + [None] * len(seqs))
        try:
            src.align_posteriors(capi.ALIGN_PROBCONS, 0.01, 0, m * (m + len(seqs)) - m * (m + 1) // 2, fetch=False)
        finally:
            src.fold_end()
        rep = src.stage_report()
        src.stage_timing(False)
        kernels = {k: (round(v[0], 4), v[2]) for k, v in rep.items() if k.startswith("k_bp_compact") or k.startswith("k_contrafold")}
        n = m + 1
        for chunk in each.chunks:
            ctx.families_from(src, [list(range(m)) + [m + j] for j in chunk])
            ctx.consistency_bp(0.25)
            alns = []
            for f, j in enumerate(chunk):
                res = each.results[j]
                mask = np.array([[ch != "-" for ch in row] for row in [res.rows[-1]] + res.rows[:-1]], np.uint8)
                alns.append((np.concatenate([[f * n + m], np.arange(f * n, f * n + m)]).astype(np.uint32), mask))
            for name, stem in stems.items():
                sss = [pipeline.carry_structure(stem, np.flatnonzero(each.results[j].rf).astype(np.uint32), len(each.results[j].rf)) for j in chunk]
                for g in ctx.structure_support(alns, sss):
                    if g["both"][0]:
                        out[name].append(float(g["expected"][0]) / float(g["both"][0]))  # the new sequence's row
    finally:
        src.close()
        ctx.close()
    return {name: dict(rows_with_pairs=len(v), expected_per_both=round(float(np.mean(v)), 4) if v else None) for name, v in out.items()}, kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--members", type=int, default=64)
    ap.add_argument("--seed-rows", type=int, default=8)
    a = ap.parse_args()
    recs, pairs_a, pairs_b = planted_family(n=a.members)
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    m = a.seed_rows
    ctx = capi.Context(0)
    seed_run = pipeline.run(names[:m], seqs[:m], ctx=ctx, decoder="Levels", th_s1=THS)
    ctx.close()
    # the run's rows and structure as the seed reader would return them: input order, no all-gap column
    snames, srows, ss, level = names[:m], seed_run.rows, seed_run.ss, seed_run.ss_level
    col_of = np.flatnonzero(np.frombuffer(srows[0].encode("latin-1"), np.uint8) != ord("-"))
    stems = dict(stem_a=_stem(len(ss), pairs_a, col_of), stem_b=_stem(len(ss), pairs_b, col_of))
    found = {k: int(sum(1 for c in np.flatnonzero(v != NONE) if ss[c] == v[c])) for k, v in stems.items()}
    ss0 = np.where(level == 0, ss, NONE).astype(np.uint32)
    new_names, new_seqs = names[m:], seqs[m:]
    kw = dict(a={}, b=dict(seed_ss=ss0), c=dict(seed_ss=ss, seed_level=level))
    ctxs = {arm: capi.Context(0) for arm in kw}
    runs = {}
    for _ in range(2):
        for arm in ("a", "b", "c"):
            runs[arm] = pipeline.add_each(snames, srows, new_names, new_seqs, ctx=ctxs[arm], **kw[arm])
    for c in ctxs.values():
        c.close()
    rec = dict(what="planted H-type family: a Levels seed, the rest added by add_each; (a) no structure, (b) level 0 only, (c) both levels",
               members=a.members, seed_rows=m, added=len(new_seqs), length_nt=len(seqs[0]), seed_ss=seed_run.ss_str,
               seed_pairs_per_level=[int(((level == k) & (ss != NONE)).sum()) for k in range(2)], planted_pairs_in_seed=found)
    for arm in ("a", "b", "c"):
        each = runs[arm]
        sup, kernels = _stems_support(arm, srows, ss, level, new_seqs, each, stems)
        rec[arm] = dict(seconds=_round(each.seconds), chunks=len(each.chunks), mean_iterations=round(float(each.iterations.mean()), 2),
                        fold_kernels_ms=kernels, support=sup)
    rec["same_rows_b_c"] = sum(x.rows == y.rows for x, y in zip(runs["b"].results, runs["c"].results))
    rec["same_rows_a_c"] = sum(x.rows == y.rows for x, y in zip(runs["a"].results, runs["c"].results))
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
