"""Raw launches of the pair kernels for tests: dafs_hipk_pairhmm3_launch / dafs_hipk_pairhmm5_launch driven the way
bench.py drives them (torch allocates, the library launches on torch's stream), several launches in sequence on ONE
scratch allocation, in one child process.  A helper module, not a conftest.

The parent describes the launches (spec), run() hands them to a child -- this file run as a program -- and returns what
each launch left; check() compares one launch with the oracle, bit for bit.

Per launch: the model (0 ProbCons, 1 CONTRAlign), th, the sequences and an explicit task list [(x, y), ...] in the order
given (sequence x gives the rows; x > y is allowed), an optional nwaves that overrides plan.nwaves after the plan call,
pool_cap (the pool is allocated with `tail` more entries behind it) and what the scratch holds when the launch starts:
  a 32-bit pattern   every word of plan.scratch_bytes is set to it
  "keep"             whatever the previous launch of this child left
  "spread"           "keep", after every wavefront's region that the previous launch left untouched (it still holds that
                     launch's fill pattern: the wavefront took no batch) has been overwritten with a copy of a region that
                     a wavefront worked in; the child fails unless at least one region was worked in.  Every wavefront of
                     this launch then starts on a slab and on lists that another pair left behind.
The words behind plan.scratch_bytes (a tail of `scratch_tail` words, and whatever a larger launch of the same child
used) are set to the canary before every launch, and the pool, the row pointers, pair_off, pair_nnz and sim are filled
with it.  DAFS_HIP_FORCE_GROUP, DAFS_HIP_FORCE_WIDTH and DAFS_HIP_EMIT_WINDOW reach the library through the child's
environment (run(env=...)), for every launch of the child, or per launch: spec(force=(group, width)) sets the first two
around that launch's plan call and spec(window=positions) the third around its launch, and the child puts back what its
environment held before (the library reads all three with getenv on every call).  One child can so run many instances.

The child synchronises after every launch and stops at the first non-zero return code or HIP error: it starts nothing
further and exits non-zero with the message."""
import json
import os
import subprocess
import sys

import numpy as np

CANARY = 0x5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANES = (2, 5)  # planes of a wavefront's scratch region, by model
_ENV = ("DAFS_HIP_FORCE_GROUP", "DAFS_HIP_FORCE_WIDTH", "DAFS_HIP_EMIT_WINDOW")

_WANT = {}


def want(oracle, s1, s2, th, model):
    """the oracle's answer for one task, computed once: (rowptr, col, val, order of the transposed half, sim)"""
    th = float(np.float32(th))
    key = (s1, s2, th, model)
    if key not in _WANT:
        rp, col, val = oracle.align_calculate(s1, s2, th, model)
        rows = np.repeat(np.arange(len(s1), dtype=np.uint32), np.diff(rp))
        order = np.lexsort((rows, col))  # transposed rows: keyed by column, rows ascending (as in _check_set)
        sim = np.float32(oracle.similarity(rp, col, val, len(s1), len(s2)))
        _WANT[key] = (rp, col, val, rows, order, sim)
    return _WANT[key]


def nnz(oracle, seqs, tasks, th, model):
    return [len(want(oracle, seqs[x], seqs[y], th, model)[1]) for x, y in tasks]


def spec(oracle, model, th, seqs, tasks, scratch, nwaves=None, pool_cap=None, plan_for=None, force=None, window=None):
    """One launch.  pool_cap defaults to what the oracle says the tasks need plus 64 entries; plan_for = (ntasks,
    max_len1, max_len2) replaces the launch's own numbers in the plan call (two launches that must share a geometry);
    force = (group, width) and window = positions hold for this launch alone (see above)."""
    tasks = [(int(x), int(y)) for x, y in tasks]
    assert tasks and all(x != y for x, y in tasks)
    assert scratch in ("keep", "spread") or 0 <= scratch <= 0xFFFFFFFF
    if pool_cap is None:
        pool_cap = 2 * sum(nnz(oracle, seqs, tasks, th, model)) + 64
    assert force is None or (len(force) == 2 and all(int(v) > 0 for v in force))
    assert window is None or int(window) > 0
    return {"model": model, "th": float(np.float32(th)), "seqs": list(seqs), "tasks": tasks, "scratch": scratch, "nwaves": nwaves,
            "pool_cap": int(pool_cap), "plan_for": plan_for, "force": force and [int(v) for v in force], "window": window and int(window)}


def run(tmp_path, launches, env=None, tail=4096, scratch_tail=4096, timeout=120):
    """Runs the launches in one child; returns one dict of arrays per launch (the launch's spec under "spec")."""
    job, out = str(tmp_path / "pair_raw_job.json"), str(tmp_path / "pair_raw_out.npz")
    with open(job, "w") as f:
        json.dump({"tail": tail, "scratch_tail": scratch_tail, "launches": launches}, f)
    child_env = {k: v for k, v in os.environ.items() if k not in _ENV}
    for k, v in (env or {}).items():
        assert k in _ENV, k
        if v is not None:
            child_env[k] = str(v)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), job, out], cwd=ROOT, env=child_env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-4000:]  # a handled status is no failure of the child; a fault or a refused launch is
    z = np.load(out)
    res = []
    for k, L in enumerate(launches):
        d = {name[len("%d_" % k):]: z[name] for name in z.files if name.startswith("%d_" % k)}
        d["spec"] = L
        d["tail"] = tail
        res.append(d)
    return res


def check_heads(oracle, out, p, rpo):
    """Task p of a launch: row pointers (both matrices), pair_nnz and sim; returns the task's row-pointer words."""
    L = out["spec"]
    x, y = L["tasks"][p]
    s1, s2 = L["seqs"][x], L["seqs"][y]
    L1, L2 = len(s1), len(s2)
    rp, col, val, rows, order, sim = want(oracle, s1, s2, L["th"], L["model"])
    got = out["rowptr"][rpo:rpo + L1 + L2 + 2]
    assert np.array_equal(got[:L1 + 1], rp), (p, x, y, "rowptr")
    assert got[L1 + 1] == 0, (p, x, y, "first transposed row pointer")
    assert np.array_equal(got[L1 + 2:], np.cumsum(np.bincount(col, minlength=L2)).astype(np.uint32)), (p, x, y, "transposed rowptr")
    assert int(out["pair_nnz"][p]) == len(col), (p, x, y, "nnz", int(out["pair_nnz"][p]), len(col))
    assert out["sim"][p:p + 1].tobytes() == np.float32(sim).tobytes(), (p, x, y, "sim", out["sim"][p:p + 1].view(np.float32), sim)
    return L1 + L2 + 2


def check_entries(oracle, out, p):
    """Task p of a launch: columns and value bits of the row half and of the transposed half; returns (off, nnz)."""
    L = out["spec"]
    x, y = L["tasks"][p]
    rp, col, val, rows, order, sim = want(oracle, L["seqs"][x], L["seqs"][y], L["th"], L["model"])
    k, o = len(col), int(out["pair_off"][p])
    h_col, h_val = out["col"], out["val"]
    assert np.array_equal(h_col[o:o + k], col), (p, x, y, "col")
    assert h_val[o:o + k].tobytes() == val.tobytes(), (p, x, y, "val")
    assert np.array_equal(h_col[o + k:o + 2 * k], rows[order]), (p, x, y, "tcol")
    assert h_val[o + k:o + 2 * k].tobytes() == val[order].tobytes(), (p, x, y, "tval")
    return o, k


def check(oracle, out, seqs, tasks, th, model):
    """One launch against the oracle.  Per task: the L1 + 1 row pointers, the zero and the L2 cumulative column counts
    behind them, columns and value bits of both halves of the pair's pool region, pair_nnz and the bits of sim.  For the
    launch: status 0, pool_top = 2 * sum nnz, the regions disjoint, and the canary in every pool word outside them, in
    the pool's tail and in the scratch behind plan.scratch_bytes."""
    L = out["spec"]
    assert L["seqs"] == list(seqs) and L["tasks"] == [(int(x), int(y)) for x, y in tasks] and L["model"] == model
    assert np.float32(L["th"]) == np.float32(th)
    assert int(out["status"][0]) == 0, out["status"]
    pool_cap = L["pool_cap"]
    h_col, h_val = out["col"], out["val"]
    assert len(h_col) == len(h_val) == pool_cap + out["tail"]
    untouched = np.ones(len(h_col), bool)
    rpo = total = 0
    for p in range(len(tasks)):
        rpo += check_heads(oracle, out, p, rpo)
        o, k = check_entries(oracle, out, p)
        assert o + 2 * k <= pool_cap, (p, o, k)
        assert untouched[o:o + 2 * k].all(), (p, "regions overlap")
        untouched[o:o + 2 * k] = False
        total += k
    assert rpo == len(out["rowptr"])
    assert int(out["pool_top"][0]) == 2 * total, (out["pool_top"], total)
    check_canaries(out, untouched)


def check_canaries(out, untouched):
    pool_cap = out["spec"]["pool_cap"]
    h_col, h_val = out["col"], out["val"]
    assert np.all(h_col[untouched] == CANARY) and np.all(h_val[untouched] == CANARY)
    assert np.all(h_col[pool_cap:] == CANARY) and np.all(h_val[pool_cap:] == CANARY)
    assert len(out["scratch_tail"]) > 0 and np.all(out["scratch_tail"] == CANARY), "scratch behind plan.scratch_bytes"


# ---------------------------------------------------------------------------------------------------------------------
# the child
# ---------------------------------------------------------------------------------------------------------------------
def _i32(word):
    return word - (1 << 32) if word >= (1 << 31) else word


class _setenv:
    """names set to values (None: left alone) for the block, then whatever they held before"""

    def __init__(self, **kw):
        self.kw = {k: str(v) for k, v in kw.items() if v is not None}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)  # os.environ calls putenv: the library's getenv sees it

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _child(job_path, out_path):
    import ctypes as C
    import torch  # before the library: both then share torch's HIP runtime, as in bench.py
    torch.cuda.init()
    sys.path.insert(0, ROOT)
    from dafs_amd import capi
    with open(job_path) as f:
        job = json.load(f)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    tail, scratch_tail = job["tail"], job["scratch_tail"]
    canary = _i32(CANARY)

    # the plans first: one scratch allocation serves every launch
    preps = []
    for L in job["launches"]:
        seqs = L["seqs"]
        lens = np.array([len(s) for s in seqs], np.uint32)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
        px = np.array([t[0] for t in L["tasks"]])
        py = np.array([t[1] for t in L["tasks"]])
        n = len(px)
        tasks = np.zeros((n, 4), np.uint32)
        tasks[:, 0] = off[px]; tasks[:, 1] = lens[px]; tasks[:, 2] = off[py]; tasks[:, 3] = lens[py]
        rp_sizes = (lens[px] + 1 + lens[py] + 1).astype(np.uint64)
        rp_off = np.concatenate([[0], np.cumsum(rp_sizes)])[:-1].astype(np.uint64)
        plan = capi.PairhmmPlan()
        nt, m1, m2 = L["plan_for"] or (n, int(lens[px].max()), int(lens[py].max()))
        assert nt >= n and m1 >= int(lens[px].max()) and m2 >= int(lens[py].max())
        fg, fw = L.get("force") or (None, None)
        with _setenv(DAFS_HIP_FORCE_GROUP=fg, DAFS_HIP_FORCE_WIDTH=fw):
            capi.check((capi.pairhmm5_plan if L["model"] else capi.pairhmm_plan)(nt, m1, m2, plan))
        planned = plan.nwaves
        if L["nwaves"]:
            plan.nwaves = L["nwaves"]  # the scratch stays the planner's; the launch refuses an nwaves it does not cover
        preps.append((seqs, n, tasks, rp_off, int(rp_sizes.sum()), plan, planned))
    words = max(p[5].scratch_bytes for p in preps) // 4
    scratch = torch.full((words + scratch_tail,), canary, dtype=torch.int32, device=dev)

    res = {}
    prev = None  # (fill pattern, wavefronts, words per wavefront) of the launch before
    for k, (L, (seqs, n, tasks, rp_off, rp_total, plan, planned)) in enumerate(zip(job["launches"], preps)):
        contra = bool(L["model"])
        pool_cap = L["pool_cap"]
        sw = plan.scratch_bytes // 4
        region = PLANES[contra] * plan.slab_steps * plan.width * 64
        worked = -1
        if L["scratch"] == "spread":
            if prev is None or prev[0] is None:
                sys.exit("launch %d: nothing to spread (the launch before it must start from a fill pattern)" % k)
            fill, nw, reg = prev
            view = scratch[:nw * reg].view(nw, reg)
            touched = (view != _i32(fill)).any(dim=1)
            worked = int(touched.sum().item())
            if worked == 0:
                sys.exit("launch %d: the launch before it worked in no wavefront's region" % k)
            src = view[int(torch.nonzero(touched)[0].item())].clone()
            view[~touched] = src
        elif L["scratch"] != "keep":
            scratch[:sw].fill_(_i32(L["scratch"]))
        scratch[sw:].fill_(canary)
        d_codes = torch.from_numpy(np.concatenate([capi.encode(s) for s in seqs])).to(dev)
        d_tasks = torch.from_numpy(tasks.view(np.int32)).to(dev)
        d_rp_off = torch.from_numpy(rp_off.view(np.int64)).to(dev)
        counters = torch.zeros(4, dtype=torch.int64, device=dev)  # [pool_top, queue, status, -]
        rowptr = torch.full((rp_total,), canary, dtype=torch.int32, device=dev)
        col = torch.full((pool_cap + tail,), canary, dtype=torch.int32, device=dev)
        val = torch.full((pool_cap + tail,), canary, dtype=torch.int32, device=dev)
        pair_off = torch.full((n,), canary, dtype=torch.int64, device=dev)
        pair_nnz = torch.full((n,), canary, dtype=torch.int32, device=dev)
        sim = torch.full((n,), canary, dtype=torch.int32, device=dev)
        a = capi.Pairhmm5Args() if contra else capi.Pairhmm3Args()
        a.codes = d_codes.data_ptr(); a.tasks = d_tasks.data_ptr(); a.ntasks = n; a.th = L["th"]
        a.scratch = scratch.data_ptr()
        a.pool_top = counters.data_ptr(); a.queue = counters.data_ptr() + 8; a.status = counters.data_ptr() + 16
        a.rp_off = d_rp_off.data_ptr(); a.rowptr_pool = rowptr.data_ptr()
        a.ent_col = col.data_ptr(); a.ent_val = val.data_ptr(); a.pool_cap = pool_cap
        a.pair_off = pair_off.data_ptr(); a.pair_nnz = pair_nnz.data_ptr(); a.sim = sim.data_ptr()
        (capi.pairhmm5_default_model if contra else capi.pairhmm3_default_model)(C.byref(a.model))
        try:
            torch.cuda.synchronize()
            with _setenv(DAFS_HIP_EMIT_WINDOW=L.get("window")):
                rc = (capi.pairhmm5_launch if contra else capi.pairhmm3_launch)(C.byref(a), C.byref(plan), C.c_void_p(stream.cuda_stream))
            if rc:
                sys.exit("launch %d: %s" % (k, capi._strerror(rc).decode()))
            torch.cuda.synchronize()
            h_counters = counters.cpu().numpy()
            out = {"status": h_counters.view(np.int32)[4:5], "pool_top": h_counters.view(np.uint64)[0:1],
                   "col": col.cpu().numpy().view(np.uint32), "val": val.cpu().numpy().view(np.uint32),
                   "rowptr": rowptr.cpu().numpy().view(np.uint32), "pair_off": pair_off.cpu().numpy(),
                   "pair_nnz": pair_nnz.cpu().numpy().view(np.uint32), "sim": sim.cpu().numpy().view(np.uint32),
                   "scratch_tail": scratch[sw:].cpu().numpy().view(np.uint32),
                   "geometry": np.array([plan.group, plan.width, plan.nwaves, planned, plan.slab_steps, plan.scratch_bytes, max(worked, 0)], np.uint64)}
        except Exception as e:  # a HIP error: nothing further is started
            sys.exit("launch %d: %r" % (k, e))
        for name, v in out.items():
            res["%d_%s" % (k, name)] = v
        prev = (L["scratch"] if isinstance(L["scratch"], int) else None, plan.nwaves, region)
    np.savez(out_path, **res)


GEOMETRY = ("group", "width", "nwaves", "planned_nwaves", "slab_steps", "scratch_bytes", "spread_worked")


def geometry(out):
    return dict(zip(GEOMETRY, (int(v) for v in out["geometry"])))


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
