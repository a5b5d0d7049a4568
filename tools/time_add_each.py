#!/usr/bin/env python3
"""Time pipeline.add_each (each new sequence added to a fixed seed on its own) against the other ways of
adding the same sequences.

  python tools/time_add_each.py [--out FILE] [K ...]

A 32-row seed of ~120 nt is aligned by a run (family_set(32 + 512, 120)'s first 32 members); then K further members (default
32, 128 and 512) are added to it:
  (a) add_each                   the matching transform for the listed (seed, new) pairs only
  (b) add_each, reliability=True the full matching transform (and the reliability annotation in `final`)
  (c) add                        the joint run: one family of 32 + K, the new sequences inform one another
  (d) K add calls of one sequence each (K = 32 only): what add_each replaces
Each runs twice on a warm context of its own, the runs alternating, and the second is reported.  Prints one JSON line per K:
the .seconds parts, the peak device memory of the resident nodes (the largest chunk's) and the estimated bytes of the largest
chunk's stores (seed_each_bytes without the node, or family_bytes of the joint family); --out also writes the lines as one
JSON list."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dafs_amd import capi, pipeline, synth  # noqa: E402

M, LENGTH, POOL = 32, 120, 512


def _round(d):
    return {k: round(v, 4) for k, v in d.items()}


def main(ks, out):
    recs = synth.family_set(M + POOL, LENGTH, seed=4242)
    names, seqs = [r[0] for r in recs], [r[1] for r in recs]
    seed_run = pipeline.run(names[:M], seqs[:M])
    srows = seed_run.rows
    keep = [c for c in range(len(srows[0])) if any(r[c] != "-" for r in srows)]
    srows = ["".join(r[c] for c in keep) for r in srows]
    snames = names[:M]
    seed_lens = [len(r.replace("-", "")) for r in srows]
    # warm-up of every kernel on a small case
    ctx = capi.Context(0)
    pipeline.add_each(snames[:4], srows[:4], names[M:M + 2], seqs[M:M + 2], ctx=ctx)
    pipeline.add_each(snames[:4], srows[:4], names[M:M + 2], seqs[M:M + 2], ctx=ctx, reliability=True)
    pipeline.add(snames[:4], srows[:4], names[M:M + 2], seqs[M:M + 2], ctx=ctx)
    ctx.close()
    lines = []
    for k in ks:
        # one context per way and K: a context's node peak is that of its lifetime
        ca, cb, cc, cd = (capi.Context(0) for _ in range(4))
        new_names, new_seqs = names[M:M + k], seqs[M:M + k]
        sizes = [pipeline.seed_each_bytes(seed_lens, len(srows[0]), len(s)) - pipeline.node_bytes(len(s), len(srows[0])) for s in new_seqs]
        rec = dict(m=M, k=k, length=LENGTH, seed_columns=len(srows[0]))
        for _ in range(2):
            a = pipeline.add_each(snames, srows, new_names, new_seqs, ctx=ca)
            b = pipeline.add_each(snames, srows, new_names, new_seqs, ctx=cb, reliability=True)
            c = pipeline.add(snames, srows, new_names, new_seqs, ctx=cc)
            if k == 32:
                t0 = time.perf_counter()
                singles = [pipeline.add(snames, srows, [nm], [sq], ctx=cd) for nm, sq in zip(new_names, new_seqs)]
                d_total = time.perf_counter() - t0
        for key, r in (("a_add_each_listed", a), ("b_add_each_full", b)):
            rec[key] = dict(seconds=_round(r.seconds), chunks=len(r.chunks), node_peak_bytes=max(mem[2] for mem in r.dd_memory),
                            store_estimate_bytes=max(sum(sizes[j] for j in ch) for ch in r.chunks))
        rec["c_add_joint"] = dict(seconds=_round(c.seconds), node_peak_bytes=c.dd_memory[2],
                                  store_estimate_bytes=pipeline.family_bytes(seed_lens + [len(s) for s in new_seqs]))
        if k == 32:
            parts = {key: sum(r.seconds[key] for r in singles) for key in ("phase1", "nodes", "final")}
            parts["total"] = d_total
            rec["d_add_one_by_one"] = dict(seconds=_round(parts), node_peak_bytes=max(r.dd_memory[2] for r in singles))
            rec["a_equals_d"] = all(x.output == y.output for x, y in zip(a.results, singles))
        rec["a_equals_b"] = all(x.output == y.output for x, y in zip(a.results, b.results))
        for c4 in (ca, cb, cc, cd):
            c4.close()
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
    main([int(a) for a in args] or [32, 128, 512], out)
