#!/usr/bin/env python3
"""Device time of the linkage rules beside the host guide tree on the same matrix, and what each tree's
cut recovers of a planted partition.

  python tools/time_linkage.py [--n 512 2048 8192] [--length 120] [--check-up-to 2048] [--out profiles/<name>.json]

The sets are those of tools/time_cluster.py: synth.family_set families of 8 for three quarters of the sequences, synth.random_set
for the rest, shuffled.  Per N one similarity pass, then on the block it left on the device, warm context, the second of two
runs: per rule the seconds of k_linkage_init and k_linkage_joins (HIP events of the library's stage recorder) and of the whole
Context.linkage_tree call, and the row rescans per join (the head of an L0 launch's workspace); the seconds of
dafs_host_build_tree on the same matrix; and for the guide tree and the three rules, cut at count = planted families +
unrelated sequences, how many planted families come back whole and the largest piece of a family.  Up to --check-up-to
sequences every tree is also compared with the numpy restatement.  Prints one JSON line per N (and writes them to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # before the library, as in bench.py: both then share one HIP runtime

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dafs_amd import capi  # noqa: E402
from linkage_ref import RULES, linkage_ref  # noqa: E402
from time_cluster import sequence_set  # noqa: E402


def recovered(labels, planted):
    """(planted families of 8 that are one whole cluster, the largest number of a family's members in one cluster)"""
    fams = {}
    for i, p in enumerate(planted):
        fams.setdefault(p, []).append(i)
    sizes = np.bincount(np.asarray(labels, np.int64))
    whole, piece = 0, 0
    for members in fams.values():
        if len(members) < 2:
            continue
        got = np.bincount(np.asarray(labels, np.int64)[members])
        piece = max(piece, int(got.max()))
        whole += int(got.max() == len(members) and sizes[int(got.argmax())] == len(members))
    return whole, piece


def rescans(rule, sim):
    """row rescans of one L0 launch, from the head of its workspace"""
    dev = torch.device("cuda", 0)
    n = sim.shape[0]
    d_sim = torch.from_numpy(sim).to(dev)
    ws = torch.zeros(capi.linkage_workspace(n), dtype=torch.uint8, device=dev)
    out = [torch.zeros(2 * n - 1, dtype=t, device=dev) for t in (torch.float32, torch.int32, torch.int32)]
    torch.cuda.synchronize(dev)
    capi.check(capi.linkage_launch(capi.LINKAGES.index(rule), n, d_sim.data_ptr(), ws.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                   out[2].data_ptr(), None))
    torch.cuda.synchronize(dev)
    head = ws[:16].cpu().numpy()
    assert head[:8].view(np.uint32).tolist() == [0, n - 1]
    return int(head[8:16].view(np.uint64)[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[512, 2048, 8192])
    ap.add_argument("--length", type=int, default=120)
    ap.add_argument("--check-up-to", type=int, default=2048)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    torch.cuda.init()
    ctx = capi.Context(0)
    try:
        for n in a.n:
            names, seqs, planted = sequence_set(n, a.length)
            k = len(set(planted))
            ctx.set_sequences(seqs)
            t0 = time.perf_counter()
            sim, ranges = ctx.similarity()
            t_sim = time.perf_counter() - t0
            for _ in range(2):  # the second run is the warm one
                t0 = time.perf_counter()
                guide = capi.build_tree(sim)
                t_guide = time.perf_counter() - t0
            whole, piece = recovered(capi.cluster_cut(guide, count=k)[0], planted)
            line = dict(what="linkage trees on the device against dafs_host_build_tree on the same similarity matrix; warm context, second of two runs",
                        n=n, length_nt=a.length, planted_families=sum(1 for p in set(planted) if planted.count(p) > 1), count=k,
                        similarity_s=round(t_sim, 3), ranges=ranges, host_build_tree_s=round(t_guide, 4),
                        guide=dict(families_whole=whole, largest_piece=piece))
            ctx.stage_timing(True)
            for rule in RULES:
                for _ in range(2):
                    ctx.stage_report()
                    t0 = time.perf_counter()
                    tree = ctx.linkage_tree(rule)
                    t_call = time.perf_counter() - t0
                    st = ctx.stage_report()
                whole, piece = recovered(capi.cluster_cut(tree, count=k)[0], planted)
                r = rescans(rule, sim)
                line[rule] = dict(k_linkage_init_s=round(st["k_linkage_init"][0] / 1e3, 6), k_linkage_joins_s=round(st["k_linkage_joins"][0] / 1e3, 6),
                                  call_s=round(t_call, 4), rescans=r, rescans_per_join=round(r / (n - 1), 3), families_whole=whole,
                                  largest_piece=piece)
                if n <= a.check_up_to:
                    line[rule]["equals_restatement"] = all(np.asarray(x).tobytes() == y.tobytes() for x, y in zip(tree, linkage_ref(sim, rule)))
            ctx.stage_timing(False)
            print(json.dumps(line), flush=True)
            lines.append(line)
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("".join(json.dumps(x) + "\n" for x in lines))
    return 0 if all(x[r].get("equals_restatement", True) for x in lines for r in RULES) else 1


if __name__ == "__main__":
    sys.exit(main())
