#!/usr/bin/env python3
"""Wall time of all pairwise structural alignments of one set of sequences on a warm context, two ways: one
pipeline.pairwise (phase 1 once over the N sequences, the pairs' two-sequence families gathered on the device) and one
pipeline.run_batch over the N(N-1)/2 two-sequence families (every sequence folded N-1 times).  Both must give the same
outputs.

  python tools/time_pairwise.py [--n 64 128] [--length 150] [--out profiles/<name>.json]

The sets are half synth.family_set draws (families of 8), half synth.random_set, lengths about --length.  Prints one JSON
line per N (and writes them to --out): the two wall times, pairwise's phase 1 / transforms / nodes / final split, the same
split of run_batch (summed over its sub-batches), the chunks and sub-batches under the default byte budget, and the peak
device memory of the resident nodes of each.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dafs_amd import capi, pipeline, synth  # noqa: E402


def sequence_set(n, length, seed=2026):
    recs = []
    for k in range(n // 2 // 8):
        recs += synth.family_set(8, length, seed=seed + k)
    recs += synth.random_set(n - len(recs), length, seed=seed + 1000)
    return ["%s_%d" % (r[0], k) for k, r in enumerate(recs)], [r[1] for r in recs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--length", type=int, default=150)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    ctx = capi.Context(0)
    try:
        names, seqs = sequence_set(16, a.length)
        pipeline.pairwise(names[:6], seqs[:6], ctx=ctx)  # warm: code objects loaded, workspaces allocated
        pipeline.run_batch([([names[x], names[y]], [seqs[x], seqs[y]]) for x, y in pipeline.all_pairs(6)], ctx=ctx)
        for n in a.n:
            names, seqs = sequence_set(n, a.length)
            t0 = time.perf_counter()
            pw = pipeline.pairwise(names, seqs, ctx=ctx)
            t_pw = time.perf_counter() - t0
            fams = [([names[x], names[y]], [seqs[x], seqs[y]]) for x, y in pw.pairs]
            t0 = time.perf_counter()
            res = pipeline.run_batch(fams, ctx=ctx)
            t_batch = time.perf_counter() - t0
            subs, seen = [], set()
            for r in res:  # one seconds dict per sub-batch, shared by its families
                if id(r.seconds) not in seen:
                    seen.add(id(r.seconds))
                    subs.append(r)
            batch_split = dict(phase1=sum(r.seconds["fold_launch"] + r.seconds["pair"] for r in subs),
                               transforms=sum(r.seconds["pct_fold_tree"] for r in subs),
                               nodes=sum(r.seconds["progressive"] for r in subs), final=sum(r.seconds["final"] for r in subs))
            line = dict(what="all pairs of N sequences: one pipeline.pairwise against one pipeline.run_batch of the two-sequence families, warm context",
                        n=n, length_nt=a.length, pairs=len(pw.pairs), pairwise_s=round(t_pw, 3), run_batch_s=round(t_batch, 3),
                        speedup=round(t_batch / t_pw, 2), outputs_equal=[r.output for r in pw.results] == [r.output for r in res],
                        pairwise_split_s={k: round(v, 3) for k, v in pw.seconds.items()},
                        run_batch_split_s={k: round(v, 3) for k, v in batch_split.items()},
                        folds_pairwise=n, folds_run_batch=2 * len(pw.pairs), chunks=len(pw.chunks), sub_batches=len(subs),
                        nodes_peak_bytes_pairwise=int(max(m[2] for m in pw.dd_memory)),
                        nodes_peak_bytes_run_batch=int(max(r.dd_memory[2] for r in subs)))
            print(json.dumps(line), flush=True)
            lines.append(line)
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))
    return 0 if all(x["outputs_equal"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
