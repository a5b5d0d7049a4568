"""dafs_hip_phase1_sharded (capi_shard.cpp) at the world sizes and inputs the process-spawning
test (test_dist_gpu.py) cannot afford: ranks without a pair, ranks without a sequence to fold, parts that are empty on
every rank, the skipped third exchange, and strides that differ between the ranks and are 0 on some.

Context.phase1_sharded takes the collective as a Python callable, so a whole world runs as threads of one process, one
Context per rank, all on the one GPU: ctypes releases the GIL around the call and the library's only globals are
thread_local.  Every rank's stores are compared, byte for byte, with those of a single-context phase 1 on the same input.
The worlds run in one child process for this file (store_dev_raw.run_checks); every test reports how one of them ended."""
import threading

import pytest

import store_dev_cases as sc
import store_dev_raw as raw
from test_store_dev_gpu import context, same_pp

pytestmark = pytest.mark.gpu
DEFAULTS = {"align": 0, "th_a": 0.01, "w_pct_a": 0.25, "w_pct_s": 0.25, "fold_th": 0.01}
BARRIER_S, JOIN_S = 60, 120  # upper bounds that end trouble; the phase itself takes well under a second


def stores(ctx):
    """mp(0), mp(1), bp(0), bp(1), sim of a context; None for a store it does not hold"""
    from dafs_amd import capi
    out = []
    for fetch in (lambda: ctx.mp(0), lambda: ctx.mp(1), lambda: ctx.bp(0), lambda: ctx.bp(1), ctx.sim):
        try:
            out.append(fetch())
        except capi.DafsHipError as e:
            assert "code -1" in str(e), e
            out.append(None)
    return out


def same_stores(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        if (g is None) != (w is None):
            return "store %d: held by one side only" % k
        if g is None:
            continue
        if not (same_pp(g, w) if k < 2 else sc.same_rows(g, w) if k < 4 else g.tobytes() == w.tobytes()):
            return "store %d differs" % k
    return None


def single(seqs, o):
    ctx = context(seqs)
    try:
        ctx.fold_posteriors(o["fold_th"])
        ctx.align_posteriors(o["align"], o["th_a"], fetch=False)
        ctx.consistency_match(o["w_pct_a"])
        ctx.consistency_bp(o["w_pct_s"])
        return stores(ctx)
    finally:
        ctx.close()


def run_world(seqs, world, o):
    """the sharded phase on `world` ranks, one thread and one context each; returns every rank's stores"""
    import torch
    from dafs_amd import dist
    ctxs = [context(seqs) for _ in range(world)]
    barrier = threading.Barrier(world, timeout=BARRIER_S)
    published, errors, exchanges = [None] * world, [None] * world, [0] * world

    def collective(rank):
        def allgather(send, recv, nbytes):
            published[rank] = (send, nbytes)
            barrier.wait()
            out = torch.as_tensor(dist._DeviceBytes(recv, world * nbytes))
            for r, (ptr, n) in enumerate(published):
                assert n == nbytes, "rank %d sends %d bytes, rank %d %d" % (r, n, rank, nbytes)
                out[r * nbytes:(r + 1) * nbytes].copy_(torch.as_tensor(dist._DeviceBytes(ptr, n)))
            torch.cuda.synchronize()
            barrier.wait()  # nobody reuses send before everyone has read it
            exchanges[rank] += 1
        return allgather

    def work(rank):
        try:
            ctxs[rank].phase1_sharded(rank, world, o["align"], o["th_a"], o["w_pct_a"], o["w_pct_s"], o["fold_th"], collective(rank))
        except BaseException as e:  # noqa: BLE001
            errors[rank] = e
            barrier.abort()  # the others leave their exchange with DAFS_HIP_ECOMM

    threads = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(JOIN_S)
    if any(t.is_alive() for t in threads):
        raise raw.Stop("a rank of world %d is still running" % world)
    try:
        failed = [(r, e) for r, e in enumerate(errors) if e is not None]
        if failed:
            first = [f for f in failed if "code -7" not in str(f[1])] or failed  # the cause, not the ranks it took along
            raise AssertionError("rank %d of %d: %r" % (first[0][0], world, first[0][1])) from first[0][1]
        return [stores(c) for c in ctxs], exchanges
    finally:
        for c in ctxs:
            c.close()


def world_check(name):
    def check():
        make, world, opts = sc.shard_runs()[name]
        o = dict(DEFAULTS, **opts)
        names, seqs = make()
        want = single(seqs, o)
        assert want[0] is not None and want[2] is not None and want[4] is not None
        assert (want[1] is None) == (o["w_pct_a"] == 0.0) and (want[3] is None) == (o["w_pct_s"] == 0.0)
        if o["fold_th"] >= 1.0:
            assert all(len(r[1]) == 0 for r in want[2]), "a base pair above a threshold of %g" % o["fold_th"]
        if o["th_a"] >= 1.0:
            assert not want[0].nnz.any() and not want[1].nnz.any()
        got, exchanges = run_world(seqs, world, o)
        # sizes and slab for each of the two or three stores that travel
        assert exchanges == [2 * (3 if o["w_pct_a"] != 0.0 else 2)] * world, exchanges
        for rank, g in enumerate(got):
            assert same_stores(g, want) is None, (name, rank, same_stores(g, want))
    return check


CHECKS = {name: world_check(name) for name in sc.shard_runs()}


@pytest.fixture(scope="module")
def outcome(tmp_path_factory):
    return raw.run_checks("test_shard_worlds_gpu", tmp_path_factory.mktemp("shard_worlds"))


@pytest.mark.parametrize("name", list(CHECKS))
def test_world(outcome, name):
    assert outcome.get(name, "not run: " + outcome["__child__"]) == "ok"
