#!/usr/bin/env python3
"""Thresholds chosen by pseudo-expected accuracy on a warm context: what the choice costs beside the
fixed-threshold decodes in the same job, what k_pea_total's memory rate is, and what the choice keeps on a family with a
planted pseudoknot and on random sequences.

  python tools/time_auto.py [--out profiles/<name>.json] [--repeat 5] [--wide 12000] [--wide-only] [--parent-tree DIR]

Timed is the final decode alone, Context.consensus_structures over alignments that a run has just produced:
  * the root alignment of the c3 set (synth.random_set(128, 150), bench.py's configuration), one alignment;
  * the 2 016 root alignments of pipeline.pairwise over 64 sequences of about 150 nt, one call;
  * one one-row alignment of --wide columns over synthetic base-pairing rows built here (one call each, no repeat).
Each with the plain call at -G 2, "Levels" at -G 2,4, `auto` with one level and `auto,auto` (the default candidates, -G
1,2,4,8,16,32): the best of --repeat wall times and the stage recorder's per-kernel times and launch counts of one more call.

The planted family is tools/time_levels.py's (an H-type pseudoknot, 8 members): reported are the thresholds `auto,auto`
chooses and the planted pairs of each stem it returns, beside the fixed -G 2,4.  On the random c3 set: whether `auto,auto`
keeps a level 1.  --parent-tree DIR: a built checkout of the parent commit; the plain and the "Levels" decodes of the first
two jobs are then also timed with that tree's package and library, in a child process of the same job (--fixed-only --tree
DIR), and recorded as build "parent" beside this build's, to show that they did not move.  Prints one JSON line per job (and
writes them to --out as they come)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --tree DIR (the child of --parent-tree): the package and library that are timed; a tree without the automatic choice
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv[1:-1] else ROOT
FIXED_ONLY = "--fixed-only" in sys.argv[1:]
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dafs_amd import capi, pipeline, synth  # noqa: E402
from time_levels import planted_family, planted_found  # noqa: E402

NONE = 0xFFFFFFFF
FIXED = (1.0 / 3.0, 1.0 / 5.0)
DECODES = (("plain_G_2", FIXED[0]), ("levels_G_2_4", FIXED))
if not FIXED_ONLY:
    DECODES += (("auto", capi.AutoThresholds()), ("auto_auto", capi.AutoThresholds(levels=2)))


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def time_decodes(ctx, alns, repeat):
    """per decode the best wall time of `repeat` calls (repeat = 0: of the one recorded call), the per-kernel device times and
    launch counts of one more, the pairs per level and, for the automatic ones, how often each candidate was chosen"""
    out = {}
    for label, th in DECODES:
        best = min([_timed(lambda: ctx.consensus_structures(alns, th)) for _ in range(repeat + 1 if repeat else 0)][1:], default=None)
        ctx.stage_timing(True)
        try:
            ctx.stage_report()
            t0 = time.perf_counter()
            got = ctx.consensus_structures(alns, th)
            once = time.perf_counter() - t0
            rep = ctx.stage_report()
        finally:
            ctx.stage_timing(False)
        rec = dict(wall_ms=round((once if best is None else best) * 1e3, 3), kernels_ms={k: (round(v[0], 4), v[2]) for k, v in sorted(rep.items())})
        if label == "plain_G_2":
            rec["pairs"] = int(sum(int(np.sum(ss != NONE)) for _, ss in got))
        else:
            K = 1 if label == "auto" else 2
            rec["pairs_per_level"] = [int(sum(int(np.sum((g[1] != NONE) & (g[2] == k))) for g in got)) for k in range(K)]
        if label.startswith("auto"):
            C = len(th.candidates)
            rec["chosen_per_level"] = [[int(sum(1 for g in got if g[3].chosen[k] == c)) for c in range(C)] for k in range(th.levels)]
            rec["kept_levels"] = [int(sum(1 for g in got if len(g[3].thresholds) == m)) for m in range(th.levels + 1)]
        out[label] = rec
    return out


def wide_rows(L, seed=5):
    """base-pairing rows of one sequence of L residues: per row a dozen scattered weak cells, and stems of eight strong pairs"""
    rs = np.random.RandomState(seed)
    cells = [dict() for _ in range(L)]
    for i in range(L - 4):
        for j in rs.randint(i + 4, L, 12):
            cells[i][int(j)] = 0.02 + 0.2 * rs.rand()
    for _ in range(L // 40):
        i = int(rs.randint(0, L - 60))
        j = i + int(rs.randint(24, 60))
        for k in range(8):
            cells[i + k][j - k] = 0.6 + 0.35 * rs.rand()
    rowptr, col, val = [0], [], []
    for c in cells:
        for j in sorted(c):
            col.append(j)
            val.append(c[j])
        rowptr.append(len(col))
    return np.array(rowptr, np.uint32), np.array(col, np.uint32), np.array(val, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--wide", type=int, default=12000, help="columns of the one-row alignment (0: leave it out)")
    ap.add_argument("--wide-only", action="store_true", help="the one-row alignment alone")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: its fixed decodes in the same job")
    ap.add_argument("--fixed-only", action="store_true", help="the plain and the Levels decodes of the first two jobs alone")
    ap.add_argument("--tree", default=None, help="time this tree's package and library (with --fixed-only)")
    a = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("".join(json.dumps(x) + "\n" for x in lines))

    if a.tree and not a.fixed_only:
        ap.error("--tree times a tree without the automatic choice: it needs --fixed-only")
    build = "this" if TREE == ROOT else "parent"
    gammas = None if FIXED_ONLY else list(capi.AutoThresholds().gammas)
    ctx = capi.Context(0)
    try:
        if not a.wide_only:
            recs = synth.random_set(128, 150, seed=12345)
            res = pipeline.run([n for n, _ in recs], [s for _, s in recs], ctx=ctx)
            emit(dict(what="final decode of the c3 root alignment (128 rows, random sequences), warm context", build=build,
                      columns=int(res.root[1].shape[1]), gammas=gammas, decodes=time_decodes(ctx, [res.root], a.repeat)))
            recs = []
            for k in range(4):
                recs += synth.family_set(8, 150, seed=2026 + k)
            recs += synth.random_set(32, 150, seed=3026)
            pw = pipeline.pairwise(["%s_%d" % (r[0], k) for k, r in enumerate(recs)], [r[1] for r in recs], ctx=ctx)
            if len(pw.chunks) == 1:  # the context still holds the stores of all pairs
                emit(dict(what="final decode of all pair alignments of pipeline.pairwise at N = 64, one call, warm context", build=build,
                          alignments=len(pw.results), gammas=gammas, decodes=time_decodes(ctx, [r.root for r in pw.results], a.repeat)))
        if not a.wide_only and not FIXED_ONLY:
            recs, pairs_a, pairs_b = planted_family()
            names, seqs = [n for n, _ in recs], [s for _, s in recs]
            au = pipeline.run(names, seqs, ctx=ctx, decoder="Levels", th_s1=capi.AutoThresholds(levels=2))
            lv = pipeline.run(names, seqs, ctx=ctx, decoder="Levels", th_s1=FIXED)
            emit(dict(what="planted H-type pseudoknot, 8 members, stems of 6 pairs: planted pairs in the consensus structure",
                      length_nt=len(seqs[0]), planted_per_stem=len(pairs_a),
                      auto_auto=dict(stem_a=planted_found(au, pairs_a), stem_b=planted_found(au, pairs_b), ss=au.ss_str,
                                     chosen_gammas=list(au.ss_auto.gammas), f=round(au.ss_auto.f, 6), pairs_per_level=[int(n) for n in au.ss_auto.npairs],
                                     candidate_pairs=au.ss_auto.cand_pairs.tolist()),
                      levels_G_2_4=dict(stem_a=planted_found(lv, pairs_a), stem_b=planted_found(lv, pairs_b), ss=lv.ss_str)))
        if a.wide and not FIXED_ONLY:
            L = a.wide
            ctx.set_sequences(["".join(np.random.RandomState(3).choice(list("ACGU"), L))])
            ctx.set_bp([wide_rows(L)])
            dec = time_decodes(ctx, [(np.array([0], np.uint32), np.ones((1, L), np.uint8))], 0)
            ms = dec["auto"]["kernels_ms"].get("k_pea_total", (0.0, 0))[0]
            emit(dict(what="one one-row alignment of %d columns, synthetic rows, one call per decode" % L, columns=L, gammas=gammas, decodes=dec,
                      k_pea_total=dict(bytes_read=2 * L * (L - 1), ms=ms, gb_per_s=round(2 * L * (L - 1) / (ms * 1e-3) / 1e9, 1) if ms else None)))
    finally:
        ctx.close()
    if a.parent_tree and not a.wide_only:  # a fresh process: the library is chosen when the package is imported
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--fixed-only", "--repeat", str(a.repeat), "--tree", a.parent_tree],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            return r.returncode
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                emit(json.loads(ln))
    return 0


if __name__ == "__main__":
    sys.exit(main())
