#!/usr/bin/env python3
"""Device time of the transfer bootstrap: what k_transfer_sides and k_transfer add to
Context.alignment_bootstrap beside k_nj_batch, and the whole call with and without the transfer sums.

  python tools/time_transfer.py [--n 128 512 2048] [--replicates 100] [--out profiles/<name>.json]

Per n: n = 128 is the c3 alignment (pipeline.run on random_set(128, 150)), the other sizes are the synthetic rows of
tools/time_bootstrap.py (300 columns that differ from one ancestor in a fifth of their cells).  Model jc.  Warm context.  The
kernels: milliseconds over all launches of the last of three calls with transfer=True (HIP events of the library's stage
recorder).  The whole call: recorder off, five calls each with and without transfer=True, alternating; all ten times are
written.  The counted work of k_transfer: pairs (split, replicate node), the 8-byte and 2-byte words a pair reads, and the
atomics.  For scale, at n = 128 the seconds of the numpy restatement (tests/transfer_ref.py) on the same replicate trees, which
must give the same sums.  Prints one JSON line per n (and writes them to --out)."""
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
from dafs_amd import capi, pipeline, synth  # noqa: E402

KERNELS = ("k_boot_pack", "k_boot_dist", "k_nj_batch", "k_transfer_sides", "k_transfer")


def synthetic_rows(n, columns=300):
    rng = np.random.default_rng(n)
    ancestor = rng.integers(0, 4, columns)
    return np.where(rng.random((n, columns)) < 0.2, rng.integers(0, 4, (n, columns)), ancestor[None, :]).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[128, 512, 2048])
    ap.add_argument("--replicates", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(line):
        print(json.dumps(line), flush=True)
        lines.append(line)
        if a.out:  # after every line: a run that is cut short keeps what it measured
            with open(a.out, "w") as fh:
                fh.write("".join(json.dumps(x) + "\n" for x in lines))

    torch.cuda.init()
    ctx = capi.Context(0)
    B = a.replicates
    try:
        for n in a.n:
            if n == 128:
                recs = synth.random_set(128, 150)
                cell = capi.encode_cells(pipeline.run([r[0] for r in recs], [r[1] for r in recs], ctx=ctx).rows)
                rows = "c3"
            else:
                cell, rows = synthetic_rows(n), "synthetic"
            tree = ctx.alignment_tree(cell)
            plain = lambda: ctx.alignment_bootstrap(cell, B=B, tree=tree)  # noqa: E731
            with_sums = lambda: ctx.alignment_bootstrap(cell, B=B, tree=tree, transfer=True)  # noqa: E731
            plain(), with_sums()  # warm
            t_plain, t_sums = [], []
            for _ in range(5):
                for call, into in ((plain, t_plain), (with_sums, t_sums)):
                    t0 = time.perf_counter()
                    call()
                    into.append(round(time.perf_counter() - t0, 5))
            ctx.stage_timing(True)
            try:
                for _ in range(3):
                    ctx.stage_report()
                    support, rep_left, rep_right, transfer = ctx.alignment_bootstrap(cell, B=B, tree=tree, trees=True, transfer=True)
                    st = ctx.stage_report()
            finally:
                ctx.stage_timing(False)
            depth = capi.split_depth(tree[0], tree[1])
            shown = support >= 0
            splits = int(shown.sum())
            line = dict(what="Context.alignment_bootstrap, model jc, without and with transfer=True; warm context; kernels of the last of three "
                             "calls with the sums: [ms over all launches, launches]; whole calls alternating, recorder off",
                        n=n, columns=int(cell.shape[1]), rows=rows, replicates=B, kernels={k: [round(st[k][0], 4), int(st[k][2])] for k in KERNELS if k in st},
                        plain_call_s=t_plain, transfer_call_s=t_sums, splits=splits,
                        pairs=splits * (2 * n - 2) * B, words_per_pair=dict(bytes8=2, bytes2=3), atomics=splits * B,
                        same_support=bool((support == plain()).all()),
                        inside_bounds=bool(((transfer >= 0) == shown).all() and (B - support[shown] <= transfer[shown]).all() and
                                           (transfer[shown] <= (B - support[shown]) * (depth[shown] - 1)).all()),
                        lowest_percent=int(min((200 * int(s) + B) // (2 * B) for s in support[shown])),
                        lowest_tbe=int(min(capi.transfer_percent(t, d, B) for t, d in zip(transfer[shown], depth[shown]))))
            if n <= 128:
                import transfer_ref
                t0 = time.perf_counter()
                want, _ = transfer_ref.transfer_ref(tree[0], tree[1], rep_left, rep_right)
                line["numpy_restatement_s"] = round(time.perf_counter() - t0, 3)
                line["same_as_restatement"] = bool((want == transfer).all())
            emit(line)
    finally:
        ctx.close()
    return 0 if all(x["same_support"] and x["inside_bounds"] and x.get("same_as_restatement", True) for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
