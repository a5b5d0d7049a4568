#!/usr/bin/env python3
"""Time dafs_hip_alignment_reliability alone on the final alignment of a run.

  python tools/time_reliability.py [c3] [c5]

c3 = random_set(128, 150), c5 = random_set(512, 400) (bench.py's configurations).  After one full run on a context, the
annotation is taken five times: wall-clock per call and the device time of each of its kernels (stage timing).  Prints
one JSON line per configuration."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dafs_amd import capi, pipeline, synth  # noqa: E402

CONFIGS = {"c3": (128, 150), "c5": (512, 400)}


def main(names):
    for cfg in names:
        n, length = CONFIGS[cfg]
        recs = synth.random_set(n, length, seed=12345)
        ctx = capi.Context(0)
        t0 = time.perf_counter()
        res = pipeline.run([r[0] for r in recs], [r[1] for r in recs], ctx=ctx)
        run_s = time.perf_counter() - t0
        seq = np.arange(n, dtype=np.uint32)
        mask = np.array([[ch != "-" for ch in row] for row in res.rows], np.uint8)
        first = ctx.alignment_reliability(seq, mask, res.ss)  # warm-up
        ctx.stage_timing(True)
        ctx.stage_report()
        walls = []
        for _ in range(5):
            t = time.perf_counter()
            r = ctx.alignment_reliability(seq, mask, res.ss)
            walls.append((time.perf_counter() - t) * 1e3)
            assert r["residue"].tobytes() == first["residue"].tobytes()
        st = ctx.stage_report()
        ctx.stage_timing(False)
        ctx.close()
        kern = {k: dict(ms_per_call=v[0] / 5, longest_ms=v[1], launches=v[2]) for k, v in st.items() if k.startswith("k_rel_")}
        print(json.dumps(dict(config=cfg, n=n, columns=int(mask.shape[1]), residues=int(mask.sum()),
                              row_visits=int(mask.sum()) * (n - 1), run_s=round(run_s, 2), wall_ms=[round(w, 3) for w in walls],
                              kernels=kern, expected_accuracy=first["expected_accuracy"])), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or ["c3", "c5"])
