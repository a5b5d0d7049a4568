#!/usr/bin/env python3
"""What clustering on structural pair scores costs and what it returns, on a warm context (the second
of two runs).

  python tools/time_cluster_structure.py [--n 512 2048] [--length 120] [--out profiles/<name>.json]

The sets are synth.structured_family_set families of 8 (three stems) for three quarters of the sequences and synth.random_set
for the last quarter, lengths about --length, in a fixed shuffled order.  Prints one JSON line per N (and writes them to
--out): the seconds of the fold of all sequences; of the similarity pass with each score and its number of ranges; the
kernels of the structure pass by stage timing (HIP events of the library's recorder: k_struct_sim per range and in all,
k_struct_w, the pair kernel beside them); the largest number of terms of a pair (--terms-n and below: from a full-pair-set
store); and, for {sequence, structure, mix} x {guide, average} cut at the planted number of clusters, the planted families
returned whole (all members in one cluster) and exactly (that cluster holds nothing else).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dafs_amd import capi, synth  # noqa: E402


def sequence_set(n, length, seed=2031):
    """(names, seqs, planted label per sequence): structured families of 8, a quarter unrelated, shuffled by a fixed generator"""
    recs, planted = [], []
    nfam = (n - n // 4) // 8
    for k in range(nfam):
        recs += synth.structured_family_set(8, length, stems=3, seed=seed + k)
        planted += [k] * 8
    rest = synth.random_set(n - len(recs), length, seed=seed + 100000)
    planted += list(range(nfam, nfam + len(rest)))
    recs += rest
    rng = synth.SplitMix64(seed)
    order = list(range(n))
    for i in range(n - 1, 0, -1):
        j = rng.below(i + 1)
        order[i], order[j] = order[j], order[i]
    return ["%s_%d" % (recs[k][0], k) for k in order], [recs[k][1] for k in order], [planted[k] for k in order], nfam


def families_returned(labels, planted, nfam):
    """(whole, exact) of the nfam planted families of 8"""
    whole = exact = 0
    for f in range(nfam):
        got = {int(labels[i]) for i in range(len(planted)) if planted[i] == f}
        if len(got) == 1:
            whole += 1
            c = got.pop()
            exact += sum(1 for x in labels if int(x) == c) == 8
    return whole, exact


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512, 2048])
    ap.add_argument("--length", type=int, default=120)
    ap.add_argument("--terms-n", type=int, default=512, help="largest N at which a full-pair-set store is made to count the terms")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    ctx = capi.Context(0)
    try:
        for n in a.n:
            names, seqs, planted, nfam = sequence_set(n, a.length)
            k = len(set(planted))
            line = dict(what="similarity pass with each score on N mixed sequences (structured families of 8 and random sequences); warm context, "
                             "second of two runs", n=n, length_nt=a.length, pairs=n * (n - 1) // 2, planted_families=nfam, clusters_asked=k)
            for _ in range(2):
                ctx.set_sequences(seqs)
                t0 = time.perf_counter()
                ctx.fold_posteriors(0.01)
                line["fold_s"] = round(time.perf_counter() - t0, 4)
            sims = {}
            for score in capi.SCORES:
                for _ in range(2):
                    ctx.set_sequences(seqs)
                    if score != "sequence":
                        ctx.fold_posteriors(0.01)
                    t0 = time.perf_counter()
                    sims[score], ranges = ctx.similarity(capi.ALIGN_PROBCONS, 0.01, score=score)
                    line["pass_%s_s" % score] = round(time.perf_counter() - t0, 4)
                line["ranges"] = ranges
            # the kernels of the structure pass
            ctx.set_sequences(seqs)
            ctx.fold_posteriors(0.01)
            ctx.stage_timing(True)
            ctx.stage_report()
            ctx.similarity(capi.ALIGN_PROBCONS, 0.01, score="structure")
            st = ctx.stage_report()
            ctx.stage_timing(False)
            ms, longest, launches = st["k_struct_sim"]
            line["k_struct_sim_ms"] = dict(total=round(ms, 3), per_range=round(ms / launches, 3), longest=round(longest, 3), launches=launches)
            line["k_struct_w_ms"] = round(st["k_struct_w"][0], 3)
            line["k_pairhmm3_ms"] = round(st["k_pairhmm3"][0], 3)
            if n <= a.terms_n:
                ctx.set_sequences(seqs)
                ctx.fold_posteriors(0.01)
                ctx.align_posteriors(capi.ALIGN_PROBCONS, 0.01, fetch=False)
                T, terms, W = ctx.structure_scores()
                line["terms_max"], line["terms_mean"] = int(terms.max()), round(float(terms.mean()), 1)
                line["T_max_over_2_40"] = round(int(T.max()) / float(1 << 40), 3)
            quality = {}
            for score in capi.SCORES:
                for linkage in ("guide", "average"):
                    t0 = time.perf_counter()
                    tree = capi.build_tree(sims[score]) if linkage == "guide" else ctx.linkage_tree(linkage, sims[score])
                    labels, _ = capi.cluster_cut(tree, count=k)
                    whole, exact = families_returned(labels, planted, nfam)
                    quality["%s/%s" % (score, linkage)] = dict(whole=whole, exact=exact, tree_s=round(time.perf_counter() - t0, 3))
            line["families_returned_of_%d" % nfam] = quality
            print(json.dumps(line), flush=True)
            lines.append(line)
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
