#!/usr/bin/env python3
"""The level-by-level decode on a warm context: what K = 2 and K = 3 levels cost beside K = 1 in the
same job, and what the decoder finds in a family with a planted pseudoknot.

  python tools/time_levels.py [--out profiles/<name>.json] [--repeat 5]

Timed is the final decode alone, Context.consensus_structures over alignments that a run has just produced:
  * the root alignment of the c3 set (synth.random_set(128, 150), bench.py's configuration), one alignment;
  * the 2 016 root alignments of pipeline.pairwise over 64 sequences of about 150 nt, one call.
Each with the plain call and with K = 1, 2, 3 levels at thresholds 1/3, 1/5, 1/9 (-G 2,4,8): the best of --repeat wall times
and the stage recorder's per-kernel times of one more call.

The planted family is built here: a root with two stems whose pairs cross (an H-type pseudoknot: A5' B5' A3' B3'), members
with substitutions that keep both stems complementary.  Reported: how many planted pairs of either stem the structure of
pipeline.run holds with decoder "Levels" at -G 2,4 and with the plain decoder at -G 2, as counted.  Prints one JSON line per
job (and writes them to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dafs_amd import capi, pipeline, synth  # noqa: E402

NONE = 0xFFFFFFFF
THS = (1.0 / 3.0, 1.0 / 5.0, 1.0 / 9.0)
PAIRS = ("AU", "UA", "GC", "CG", "GU", "UG")


def time_decodes(ctx, alns, repeat):
    """per decoder the best wall time of `repeat` calls, the per-kernel device times of one more, and the pairs per level"""
    out = {}
    for label, th in [("plain", THS[0])] + [("K=%d" % k, THS[:k]) for k in (1, 2, 3)]:
        ctx.consensus_structures(alns, th)
        best = min(_timed(lambda: ctx.consensus_structures(alns, th)) for _ in range(repeat))
        ctx.stage_timing(True)
        try:
            ctx.stage_report()
            got = ctx.consensus_structures(alns, th)
            rep = ctx.stage_report()
        finally:
            ctx.stage_timing(False)
        rec = dict(wall_ms=round(best * 1e3, 3), kernels_ms={k: (round(v[0], 4), v[2]) for k, v in sorted(rep.items())})
        if label != "plain":
            rec["pairs_per_level"] = [int(sum(int(np.sum((ss != NONE) & (lv == k))) for _, ss, lv in got)) for k in range(len(th))]
        else:
            rec["pairs"] = int(sum(int(np.sum(ss != NONE)) for _, ss in got))
        out[label] = rec
    return out


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def planted_family(n=8, stem=6, loop=5, seed=7, comp=0.5, sub=0.15):
    """(records, stem A pairs, stem B pairs): residue indices of the planted pairs, the same in every member (no indels)"""
    rs = np.random.RandomState(seed)
    rnd = lambda k: [str(x) for x in rs.choice(list("ACGU"), k)]
    a = [PAIRS[2 + rs.randint(2)] for _ in range(stem)]  # G-C rich stems
    b = [PAIRS[2 + rs.randint(2)] for _ in range(stem)]
    parts = [rnd(loop), [p[0] for p in a], rnd(loop), [p[0] for p in b], rnd(loop), [p[1] for p in reversed(a)], rnd(loop),
             [p[1] for p in reversed(b)], rnd(loop)]
    start = np.cumsum([0] + [len(p) for p in parts])
    root = [ch for p in parts for ch in p]
    pairs_a = [(int(start[1]) + k, int(start[6]) - 1 - k) for k in range(stem)]
    pairs_b = [(int(start[3]) + k, int(start[8]) - 1 - k) for k in range(stem)]
    planted = {i for pr in pairs_a + pairs_b for i in pr}
    recs = []
    for m in range(n):
        s = list(root)
        for i, j in pairs_a + pairs_b:
            if rs.rand() < comp:
                s[i], s[j] = PAIRS[rs.randint(len(PAIRS))]
        for i in range(len(s)):
            if i not in planted and rs.rand() < sub:
                s[i] = "ACGU"[rs.randint(4)]
        recs.append(("knot_%d" % m, "".join(s)))
    return recs, pairs_a, pairs_b


def planted_found(res, pairs):
    """planted pairs (residue indices of the first sequence) that the result's structure holds, through that row's columns"""
    col = np.flatnonzero(np.frombuffer(res.rows[0].encode("latin-1"), np.uint8) != ord("-"))
    return int(sum(1 for i, j in pairs if res.ss[col[i]] == col[j]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    lines = []
    ctx = capi.Context(0)
    try:
        recs = synth.random_set(128, 150, seed=12345)
        res = pipeline.run([n for n, _ in recs], [s for _, s in recs], ctx=ctx)
        lines.append(dict(what="final decode of the c3 root alignment (128 rows), warm context", columns=int(res.root[1].shape[1]),
                          thresholds=THS, decodes=time_decodes(ctx, [res.root], a.repeat)))
        print(json.dumps(lines[-1]), flush=True)
        recs = []
        for k in range(4):
            recs += synth.family_set(8, 150, seed=2026 + k)
        recs += synth.random_set(32, 150, seed=3026)
        pw = pipeline.pairwise(["%s_%d" % (r[0], k) for k, r in enumerate(recs)], [r[1] for r in recs], ctx=ctx)
        if len(pw.chunks) == 1:  # the context still holds the stores of all pairs
            lines.append(dict(what="final decode of all pair alignments of pipeline.pairwise at N = 64, one call, warm context",
                              alignments=len(pw.results), thresholds=THS, decodes=time_decodes(ctx, [r.root for r in pw.results], a.repeat)))
            print(json.dumps(lines[-1]), flush=True)
        recs, pairs_a, pairs_b = planted_family()
        names, seqs = [n for n, _ in recs], [s for _, s in recs]
        lv = pipeline.run(names, seqs, ctx=ctx, decoder="Levels", th_s1=THS[:2])
        nu = pipeline.run(names, seqs, ctx=ctx, th_s1=THS[0])
        lines.append(dict(what="planted H-type pseudoknot, 8 members, stems of 6 pairs: planted pairs in the consensus structure",
                          length_nt=len(seqs[0]), levels_G_2_4=dict(stem_a=planted_found(lv, pairs_a), stem_b=planted_found(lv, pairs_b),
                                                                  ss=lv.ss_str, scores=[float(x) for x in lv.ss_scores]),
                          nussinov_G_2=dict(stem_a=planted_found(nu, pairs_a), stem_b=planted_found(nu, pairs_b), ss=nu.ss_str),
                          planted_per_stem=len(pairs_a)))
        print(json.dumps(lines[-1]), flush=True)
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
