#!/usr/bin/env python3
"""Time pipeline.add (new sequences added to a fixed seed) against aligning everything from scratch.

  python tools/time_add.py [K ...]

A 32-row seed of ~120 nt is aligned by a run (family_set(32 + 128, 120)'s first 32 members); then K new members of the same
family (default 32 and 128) are added to it, and pipeline.run aligns the 32 + K sequences from scratch.  Each is timed twice
on a warm context of its own.  Prints one JSON line per K: wall seconds of phase 1 and of the node phase (add) or the
progressive phase (run), and the peak device memory of the resident nodes."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dafs_amd import capi, pipeline, synth  # noqa: E402

M, LENGTH, POOL = 32, 120, 128


def main(ks):
    recs = synth.family_set(M + POOL, LENGTH, seed=4242)
    names, seqs = [r[0] for r in recs], [r[1] for r in recs]
    seed_run = pipeline.run(names[:M], seqs[:M])
    srows = seed_run.rows
    keep = [c for c in range(len(srows[0])) if any(r[c] != "-" for r in srows)]
    srows = ["".join(r[c] for c in keep) for r in srows]
    snames = names[:M]
    # warm-up of every kernel on a small case
    pipeline.add(snames[:4], srows[:4], names[M:M + 2], seqs[M:M + 2])
    for k in ks:
        new_names, new_seqs = names[M:M + k], seqs[M:M + k]
        add_t, run_t = [], []
        ctx = capi.Context(0)
        for _ in range(2):
            r = pipeline.add(snames, srows, new_names, new_seqs, ctx=ctx)
            add_t.append(dict(phase1_s=round(r.seconds["phase1"], 4), nodes_s=round(r.seconds["nodes"], 4),
                              final_s=round(r.seconds["final"], 4), total_s=round(r.seconds["total"], 4), node_peak_bytes=r.dd_memory[2]))
        ctx.close()
        ctx = capi.Context(0)
        for _ in range(2):
            r2 = pipeline.run(names[:M + k], seqs[:M + k], ctx=ctx)
            s = r2.seconds
            run_t.append(dict(phase1_s=round(s["fold_launch"] + s["pair"] + s["pct_fold_tree"], 4), progressive_s=round(s["progressive"], 4),
                              final_s=round(s["final"], 4), total_s=round(s["total"], 4), node_peak_bytes=r2.dd_memory[2]))
        ctx.close()
        print(json.dumps(dict(m=M, k=k, length=LENGTH, seed_columns=len(srows[0]), merged_columns=len(r.rf),
                              insert_columns=int((~r.rf).sum()), add=add_t, run_from_scratch=run_t,
                              run_columns=len(r2.rows[0]))), flush=True)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [32, 128])
