#!/usr/bin/env python3
"""Wall time of pipeline.cluster on a mixed set of sequences, on a warm context (the second of two runs), beside one
pipeline.run_batch that is handed the same partition: run_batch is the floor, the difference is what the clustering costs.

  python tools/time_cluster.py [--n 512 2048] [--length 120] [--out profiles/<name>.json]

The sets are synth.family_set families of 8 for three quarters of the sequences and synth.random_set for the last quarter,
lengths about --length, in a fixed shuffled order.  The cut asks for as many clusters as the set was planted with (the
families plus the unrelated sequences).  Prints one JSON line per N (and writes them to --out): the seconds of the
similarity pass with its number of ranges, of the tree and cut, of the batch and in total; the share of pairs computed twice
(the pairs within the clusters, which the batch computes again, over all pairs); run_batch's seconds on the same partition;
whether the partition is the planted one and whether both gave the same outputs.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dafs_amd import capi, pipeline, synth  # noqa: E402


def sequence_set(n, length, seed=2027):
    """(names, seqs, planted label per sequence): families of 8, a quarter unrelated, shuffled by a fixed generator"""
    recs, planted = [], []
    nfam = (n - n // 4) // 8
    for k in range(nfam):
        recs += synth.family_set(8, length, seed=seed + k)
        planted += [k] * 8
    rest = synth.random_set(n - len(recs), length, seed=seed + 100000)
    planted += list(range(nfam, nfam + len(rest)))
    recs += rest
    rng = synth.SplitMix64(seed)
    order = list(range(n))
    for i in range(n - 1, 0, -1):
        j = rng.below(i + 1)
        order[i], order[j] = order[j], order[i]
    return ["%s_%d" % (recs[k][0], k) for k in order], [recs[k][1] for k in order], [planted[k] for k in order]


def same_partition(labels, planted):
    pairs = set(zip((int(x) for x in labels), planted))
    return len(pairs) == len(set(planted)) == len(set(int(x) for x in labels))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--length", type=int, default=120)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    ctx = capi.Context(0)
    try:
        for n in a.n:
            names, seqs, planted = sequence_set(n, a.length)
            k = len(set(planted))
            for _ in range(2):  # the second run is the warm one
                t0 = time.perf_counter()
                cl = pipeline.cluster(names, seqs, count=k, ctx=ctx)
                t_cluster = time.perf_counter() - t0
            fams = [([names[i] for i in m], [seqs[i] for i in m]) for m in cl.clusters]
            for _ in range(2):
                t0 = time.perf_counter()
                res = pipeline.run_batch(fams, ctx=ctx)
                t_batch = time.perf_counter() - t0
            within = sum(len(m) * (len(m) - 1) // 2 for m in cl.clusters)
            line = dict(what="pipeline.cluster of N mixed sequences against pipeline.run_batch handed the same partition; warm context, second of two runs",
                        n=n, length_nt=a.length, clusters=len(cl.clusters), largest_cluster=max(len(m) for m in cl.clusters),
                        planted_partition=same_partition(cl.labels, planted), pairs=n * (n - 1) // 2, ranges=cl.ranges,
                        cluster_s=round(t_cluster, 3), split_s={key: round(v, 3) for key, v in cl.seconds.items()},
                        pairs_computed_twice=within, share_computed_twice=round(within / (n * (n - 1) // 2), 5),
                        run_batch_s=round(t_batch, 3), clustering_costs_s=round(t_cluster - t_batch, 3),
                        outputs_equal=[r.output for r in cl.results] == [r.output for r in res])
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
