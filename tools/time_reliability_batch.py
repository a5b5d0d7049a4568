#!/usr/bin/env python3
"""Time the reliability annotation of many alignments: one Context.alignment_reliability call per alignment against one
Context.alignment_reliabilities call, and what that does to the drivers.

  python tools/time_reliability_batch.py [--part a b c] [--tree DIR] [--label NAME] [--out FILE]

Every figure is the second of two runs on a warm context.
  (a) the annotation alone, on the stores the drivers leave in the context: the 2 016 two-row final alignments of
      pipeline.pairwise at N = 64 (~150 nt), and the placements of pipeline.add_each of 512 sequences against the 32-row seed
      of tools/time_add_each.py (those of its first chunk); one call per alignment, then one call for all, the results compared
  (b) the `final` stage and the total of pipeline.pairwise(reliability=True) at N = 64 and of
      pipeline.run_batch(reliability=True) over 512 families of 3-8 sequences of 60-100 nt.  This part uses nothing that an
      older tree lacks: --tree DIR imports the package from DIR, so that one job can alternate two builds
  (c) pipeline.add_each(merged=True) against pipeline.add_each(reliability=True) at k = 512 with the seed's structure: the
      transform stage, the final stage and the total -- what the wanted rows and the listed transform save
Prints one JSON line per measurement; --out appends them to FILE."""
import argparse
import json
import os
import sys
import time

import numpy as np

M, LENGTH, POOL = 32, 120, 512


def _round(d):
    return {k: round(v, 4) for k, v in d.items()}


def _pair_set(synth, n, length, seed=2026):  # tools/time_pairwise.py's
    recs = []
    for k in range(n // 2 // 8):
        recs += synth.family_set(8, length, seed=seed + k)
    recs += synth.random_set(n - len(recs), length, seed=seed + 1000)
    return ["%s_%d" % (r[0], k) for k, r in enumerate(recs)], [r[1] for r in recs]


def _seed(pipeline, synth):  # tools/time_seed_structure.py's
    recs = synth.family_set(M + POOL, LENGTH, seed=4242)
    names, seqs = [r[0] for r in recs], [r[1] for r in recs]
    run = pipeline.run(names[:M], seqs[:M])
    keep = [c for c in range(len(run.rows[0])) if any(r[c] != "-" for r in run.rows)]
    now = {c: k for k, c in enumerate(keep)}
    srows = ["".join(r[c] for c in keep) for r in run.rows]
    ss = np.array([now[int(run.ss[c])] if run.ss[c] != pipeline.NONE and int(run.ss[c]) in now else pipeline.NONE for c in keep], np.uint32)
    return names, seqs, srows, ss


def _both_ways(ctx, alns, sss):
    """(seconds of one call per alignment, seconds of one call for all, equal), each the second of two runs"""
    for _ in range(2):
        t0 = time.perf_counter()
        single = [ctx.alignment_reliability(s, m, ss) for (s, m), ss in zip(alns, sss)]
        t1 = time.perf_counter()
        batch = ctx.alignment_reliabilities(alns, sss)
        t2 = time.perf_counter()
    same = all(a[k].tobytes() == b[k].tobytes() for a, b in zip(single, batch) for k in ("residue", "col", "pair", "pair_rows"))
    return t1 - t0, t2 - t1, same


def part_a(capi, pipeline, synth, emit):
    ctx = capi.Context(0)
    try:
        names, seqs = _pair_set(synth, 64, 150)
        pw = pipeline.pairwise(names, seqs, ctx=ctx)  # its one chunk's stores stay in the context
        assert len(pw.chunks) == 1
        alns = [(np.array([2 * j, 2 * j + 1], np.uint32), np.array([[ch != "-" for ch in row] for row in r.rows], np.uint8))
                for j, r in enumerate(pw.results)]
        one, all_, same = _both_ways(ctx, alns, [r.ss for r in pw.results])
        emit(dict(part="a", what="pairwise N=64: the annotation of its final alignments alone", alignments=len(alns), rows=2,
                  per_alignment_calls_s=round(one, 4), one_call_s=round(all_, 4), equal=same))
        names, seqs, srows, _ = _seed(pipeline, synth)
        chunks = pipeline.add_each(names[:M], srows, names[M:], seqs[M:], ctx=ctx, reliability=True).chunks
        k0 = len(chunks[0])  # the first chunk again, alone, so that its stores are the ones left in the context
        each = pipeline.add_each(names[:M], srows, names[M:M + k0], seqs[M:M + k0], ctx=ctx, reliability=True)
        assert each.chunks == [list(range(k0))]
        n = M + 1
        alns, sss = [], []
        for f, r in enumerate(each.results):
            mask = np.array([[ch != "-" for ch in row] for row in [r.rows[-1]] + r.rows[:-1]], np.uint8)
            alns.append((np.concatenate([[f * n + M], np.arange(f * n, f * n + M)]).astype(np.uint32), mask))
            sss.append(r.ss)
        one, all_, same = _both_ways(ctx, alns, sss)
        for _ in range(2):
            t0 = time.perf_counter()
            ctx.alignment_reliabilities(alns, sss, want=[np.arange(n) == 0] * len(alns))
            new_only = time.perf_counter() - t0
        emit(dict(part="a", what="add_each of 512 against a 32-row seed: the annotation of the first chunk's placements alone",
                  alignments=len(alns), rows=n, chunks=len(chunks), per_alignment_calls_s=round(one, 4), one_call_s=round(all_, 4),
                  one_call_new_rows_only_s=round(new_only, 4), equal=same))
    finally:
        ctx.close()


def part_b(capi, pipeline, synth, emit):
    ctx = capi.Context(0)
    try:
        names, seqs = _pair_set(synth, 64, 150)
        rs = np.random.RandomState(7)
        fams = []
        for k in range(512):
            recs = synth.family_set(int(rs.randint(3, 9)), int(rs.randint(60, 101)), seed=7000 + k)
            fams.append(([r[0] for r in recs], [r[1] for r in recs]))
        pipeline.pairwise(names[:6], seqs[:6], ctx=ctx, reliability=True)  # warm
        pipeline.run_batch(fams[:4], ctx=ctx, reliability=True)
        for _ in range(2):
            t0 = time.perf_counter()
            pw = pipeline.pairwise(names, seqs, ctx=ctx, reliability=True)
            t_pw = time.perf_counter() - t0
        emit(dict(part="b", what="pairwise(reliability=True), N=64", pairs=len(pw.pairs), final_s=round(pw.seconds["final"], 4), total_s=round(t_pw, 4)))
        for _ in range(2):
            t0 = time.perf_counter()
            res = pipeline.run_batch(fams, ctx=ctx, reliability=True)
            t_rb = time.perf_counter() - t0
        subs = {id(r.seconds): r.seconds for r in res}
        emit(dict(part="b", what="run_batch(reliability=True), 512 families of 3-8 sequences of 60-100 nt", families=len(fams),
                  sub_batches=len(subs), final_s=round(sum(s["final"] for s in subs.values()), 4), total_s=round(t_rb, 4)))
    finally:
        ctx.close()


def part_c(capi, pipeline, synth, emit):
    names, seqs, srows, ss = _seed(pipeline, synth)
    ca, cb = capi.Context(0), capi.Context(0)
    try:
        for c in (ca, cb):
            pipeline.add_each(names[:M], srows, names[M:M + 2], seqs[M:M + 2], ctx=c, seed_ss=ss, merged=True, reliability=c is cb)  # warm
        for _ in range(2):
            a = pipeline.add_each(names[:M], srows, names[M:], seqs[M:], ctx=ca, seed_ss=ss, merged=True)
            b = pipeline.add_each(names[:M], srows, names[M:], seqs[M:], ctx=cb, seed_ss=ss, reliability=True)
        same = all(p.tobytes() == r.reliability["residue"][M].tobytes() for p, r in zip(a.merged.pp, b.results))
        emit(dict(part="c", what="add_each at k=512 against a 32-row seed with its structure", k=POOL, merged_columns=len(a.merged.rf),
                  seed_columns=len(srows[0]), merged_listed=_round(a.seconds), reliability_full=_round(b.seconds), new_rows_equal=same))
    finally:
        ca.close()
        cb.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", nargs="+", default=["a", "b", "c"])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, a.tree)
    from dafs_amd import capi, pipeline, synth

    def emit(rec):
        if a.label:
            rec = dict(build=a.label, **rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(rec) + "\n")
    for p in a.part:
        {"a": part_a, "b": part_b, "c": part_c}[p](capi, pipeline, synth, emit)


if __name__ == "__main__":
    main()
