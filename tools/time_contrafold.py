#!/usr/bin/env python3
"""Device time of k_contrafold and k_contrafold_posterior (Context.stage_report) on one set per path of the kernel:

  128x150   the benchmark's set: two term buffers, FC ring
  32x400    one buffer, no ring
  32xGC90   32 copies of "GC" * 90: most lists overflow the pool, the cells run their pipelined in-cell loops
  32x181c   32 sequences of 181 nt under a random structure: the constrained in-cell loops

  python tools/time_contrafold.py                         the library DAFS_HIP_LIB names (default: the regular build);
                                                          WARM folds, then REPS timed ones: one JSON line per set
  python tools/time_contrafold.py N L                     the same for N random sequences of about L nt alone
  python tools/time_contrafold.py --ab PARENT.so NEW.so [ROUNDS]
      parent, new, parent, new ... ROUNDS times, each in a process of its own; per set and kernel the median of each run, then
      the parent's median, the spread of the parent's runs against each other, and the new library's median beside them.
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KERNELS = ("k_contrafold", "k_contrafold_posterior")


def structure(L, rng):
    """three hairpin stems of four G-C pairs, one in each third of the sequence: (0-based pairs, constraint string)"""
    cons, pairs, third = ["?"] * L, [], L // 3
    for t in range(3):
        i = t * third + rng.below(third - 30)
        j = i + 14 + rng.below(12)
        for h in range(4):
            cons[i + h], cons[j - h] = "(", ")"
            pairs.append((i + h, j - h))
    return pairs, "".join(cons)


def sets(argv):
    from dafs_amd import synth

    def rnd(n, L, **kw):
        return [r[1] for r in synth.random_set(n, L, seed=12345, **kw)]
    if argv:
        n, L = int(argv[0]), int(argv[1])
        return [("%dx%d" % (n, L), rnd(n, L), None)]
    rng = synth.SplitMix64(181)
    seqs, cons = [], []
    for s in rnd(32, 181, jitter=0):
        pairs, c = structure(len(s), rng)
        b = list(s)
        for i, j in pairs:
            b[i], b[j] = "G", "C"
        seqs.append("".join(b))
        cons.append(c)
    return [("128x150", rnd(128, 150), None), ("32x400", rnd(32, 400), None), ("32xGC90", ["GC" * 90] * 32, None), ("32x181c", seqs, cons)]


def measure(argv):
    from dafs_amd import capi
    warm, reps = int(os.environ.get("WARM", "2")), int(os.environ.get("REPS", "9"))
    ctx = capi.Context(0)
    ctx.stage_timing(True)
    for name, seqs, cons in sets(argv):
        ctx.set_sequences(seqs)
        for _ in range(warm):
            ctx.fold_posteriors(0.01, constraints=cons)
        ctx.stage_report()
        row = {"set": name, "host_ms": []}
        for _ in range(reps):
            t = time.perf_counter()
            ctx.fold_posteriors(0.01, constraints=cons)
            row["host_ms"].append(round(1e3 * (time.perf_counter() - t), 3))
            rep = ctx.stage_report()
            for k in KERNELS:
                row.setdefault(k, []).append(round(rep[k][0], 4))
        print(json.dumps(row), flush=True)
    ctx.close()


def ab(parent, new, rounds):
    runs = {"parent": [], "new": []}
    for r in range(rounds):
        for tag, lib in (("parent", parent), ("new", new)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, DAFS_HIP_LIB=os.path.abspath(lib)),
                               capture_output=True, text=True, timeout=300)
            if p.returncode != 0:  # nothing more is started on a device that a run has left in doubt
                raise SystemExit("%s, round %d: exit status %d\n%s%s" % (tag, r, p.returncode, p.stdout, p.stderr))
            rows = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
            for d in rows:
                print("%s %d %s" % (tag, r, json.dumps(d)), flush=True)
            runs[tag].append({d["set"]: d for d in rows})
    print("%-8s %-24s %10s %10s %21s  %s" % ("set", "kernel", "parent ms", "new ms", "parent runs min..max", "new against the parent's runs"))
    for name in runs["parent"][0]:
        for k in KERNELS:
            pm = [statistics.median(run[name][k]) for run in runs["parent"]]
            nm = statistics.median(statistics.median(run[name][k]) for run in runs["new"])
            where = "within" if min(pm) <= nm <= max(pm) else ("below" if nm < min(pm) else "ABOVE")
            print("%-8s %-24s %10.4f %10.4f %10.4f..%-9.4f  %s" % (name, k, statistics.median(pm), nm, min(pm), max(pm), where))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--ab"]:
        ab(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 4)
    else:
        measure(sys.argv[1:])
