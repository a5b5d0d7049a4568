"""The reference and the cases of the device store exchange tests (store_dev_cases.py) do what they are for; no GPU.
slice_mp against dense matrices, the splits and block orders, the sizes that put k_scan_excl beyond one element per
thread, and -- through the oracle -- that a threshold of 2 empties a store and phase 1 still completes, which the sharded
worlds of test_shard_worlds_gpu.py rely on."""
import ctypes as C

import numpy as np
import pytest

import store_dev_cases as sc

HAND = list(sc.HAND)


def _dense(m, ncols):
    rp, col, val = m
    d = np.zeros((len(rp) - 1, ncols), np.float32)
    for i in range(len(rp) - 1):
        d[i, col[rp[i]:rp[i + 1]]] = val[rp[i]:rp[i + 1]]
    return d


@pytest.mark.parametrize("name", HAND)
def test_slice_mp_is_the_fetch_layout(name):
    """the whole store through slice_mp, read back with the layout written down here: per pair both row-pointer blocks and
    both halves of the entries, the second the transpose of the first"""
    case = sc.HAND[name]()
    pp = sc.case_pp(case)
    nnz, rp, col, val = sc.slice_mp(pp, case.lens, 0, len(pp))
    assert len(rp) == sum(case.lens[x] + 1 + case.lens[y] + 1 for x, y in case.pairs) and len(col) == len(val) == 2 * int(nnz.sum())
    r0 = e0 = 0
    for p, (x, y) in enumerate(case.pairs):
        lx, ly, k = case.lens[x], case.lens[y], int(nnz[p])
        want = _dense(case.mps[(x, y)], ly)
        assert k == np.count_nonzero(want)
        fwd = (rp[r0:r0 + lx + 1], col[e0:e0 + k], val[e0:e0 + k])
        bwd = (rp[r0 + lx + 1:r0 + lx + ly + 2], col[e0 + k:e0 + 2 * k], val[e0 + k:e0 + 2 * k])
        assert fwd[0][0] == 0 and fwd[0][-1] == k and bwd[0][0] == 0 and bwd[0][-1] == k
        assert _dense(fwd, ly).tobytes() == want.tobytes() and _dense(bwd, lx).tobytes() == want.T.copy().tobytes(), (x, y)
        for m in (fwd, bwd):  # columns ascend within a row
            assert all(np.all(np.diff(m[1][m[0][i]:m[0][i + 1]].astype(np.int64)) > 0) for i in range(len(m[0]) - 1))
        r0 += lx + ly + 2
        e0 += 2 * k


@pytest.mark.parametrize("name", HAND)
def test_the_slices_of_every_split_are_the_whole(name):
    case = sc.HAND[name]()
    pp = sc.case_pp(case)
    whole = sc.slice_mp(pp, case.lens, 0, len(pp))
    for split in sc.splits(len(pp)):
        assert split[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(split, split[1:])) and sum(split[-1]) == len(pp)
        parts = [sc.slice_mp(pp, case.lens, f, c) for f, c in split]
        for k in range(4):
            assert np.concatenate([p[k] for p in parts]).tobytes() == whole[k].tobytes(), (split[:3], k)


@pytest.mark.parametrize("npairs", [1, 2, 3, 6, 28, 36, 136, 1081])
def test_splits_reach_the_edges(npairs):
    todo = sc.ranges(npairs)
    assert len(set(todo)) == len(todo) and all(0 <= f and 0 <= c and f + c <= npairs for f, c in todo)
    for r in [(0, npairs), (0, 0), (npairs, 0), (0, 1), (npairs - 1, 1)]:
        assert r in todo
    assert any(c == 0 for f, c in todo) and any(c > 0 and f + c == npairs and (f > 0 or npairs == 1) for f, c in todo)
    assert all((p, 1) in todo for p in range(npairs))  # the worlds npairs and npairs + 3 are single pairs
    empty_ranks = [r for r in sc.world_split(npairs, npairs + 3) if r[1] == 0]
    assert len(empty_ranks) == 3 and (npairs < 3 or any(0 < f < npairs for f, _ in empty_ranks))


def test_world_splits_are_the_library_s_pair_ranges():
    from dafs_amd import capi, dist
    f = capi.lib.dafs_hip_pair_range
    f.restype = None
    f.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    for npairs in (1, 10, 36, 1081):
        for w in sc.WORLDS + (npairs, npairs + 3):
            got = sc.world_split(npairs, w)
            assert [(b, b + c) for b, c in got] == dist.pair_ranges(npairs, w)
            for r, (first, count) in enumerate(got):
                b, e = C.c_uint64(), C.c_uint64()
                f(npairs, w, r, C.byref(b), C.byref(e))
                assert (b.value, e.value) == (first, first + count), (npairs, w, r)


def test_many_pairs():
    case = sc.many_pairs()
    assert case.n == 47 and len(case.pairs) == 1081 > 1024 and min(case.lens) == 1 and max(case.lens) == 6
    nnz = case.set_mp_args()[0]
    assert all(nnz[p] == 0 for p in sc.MANY_EMPTY) and all(nnz[p] > 0 for p in sc.MANY_FULL)
    assert 0.1 < np.mean(nnz == 0) < 0.3 and 2.0 < nnz[nnz > 0].mean() < 4.0
    # a scan of 1024 threads over these counts: chunks of two, so threads 541 .. 1023 have none (b == e == n)
    chunk = (1081 + 1023) // 1024
    assert chunk == 2 and min(541 * chunk, 1081) == 1081
    for first, count in sc.MANY_EXTRA:
        assert first + count <= 1081
    assert sorted(c for _, c in sc.MANY_EXTRA) == [1023, 1024, 1025, 1025]


@pytest.mark.parametrize("n", sc.BP_ONLY)
def test_bp_only(n):
    case = sc.bp_only(n)
    assert len(case.lens) == len(case.bps) == len(case.seqs) == n and set(case.lens) == {1, 2, 3, 4}
    counts = [len(r[1]) for r in case.bps]
    assert counts[0] == 0 and counts[-1] == 0 and set(counts) == {0, 1, 2, 3}
    for L, s, (rp, col, val) in zip(case.lens, case.seqs, case.bps):
        assert len(s) == L and len(rp) == L + 1 and rp[-1] == len(col) == len(val)
        rows = np.repeat(np.arange(L), np.diff(rp.astype(np.int64)))
        assert np.all(col > rows) and np.all(col < L)
    assert (n + 1023) // 1024 == (1 if n <= 1024 else 2 if n <= 2048 else 3)


@pytest.mark.parametrize("n", [2, 8, 9, 17, 1025])
def test_block_orders(n):
    orders = sc.block_orders(n)
    assert set(orders) == {"identity", "reversed", "world_2", "world_3", "world_n+2", "shuffle"}
    for name, order in orders.items():
        assert sorted(order) == list(range(n)), name
    assert orders["identity"] == orders["world_n+2"] == list(range(n))
    if n > 3:
        assert len({tuple(o) for o in orders.values()}) == 5
        assert orders["world_3"][:2] == [0, 3] and orders["world_2"][:2] == [0, 2]


@pytest.mark.parametrize("name", ["lengths", "chunks_17"])
def test_slice_bp_unpermuted_gives_the_rows_back(name):
    case = sc.HAND[name]()
    ident = sc.slice_bp(case.bps, range(case.n))
    for oname, order in sc.block_orders(case.n).items():
        rp, col, val = sc.slice_bp(case.bps, order)
        assert len(rp) == len(ident[0]) and len(col) == len(ident[1])
        assert sc.same_rows(sc.unslice_bp(case.lens, order, rp, col, val), case.bps), oname
        if order != list(range(case.n)):
            assert col.tobytes() != ident[1].tobytes(), oname  # the order matters to the bytes
            twice = [order[x] for x in order]  # the order applied twice is another order
            if twice != order:
                assert sc.slice_bp(case.bps, twice)[1].tobytes() != col.tobytes(), oname


def test_computed_inputs():
    names, seqs = sc.computed()
    lens = [len(s) for s in seqs]
    assert len(seqs) == 9 and lens[6:] == [1, 2, 97] and all(30 <= L <= 50 for L in lens[:6]) and len(set(names)) == 9
    # align_posteriors processes the pairs longest first (stable): here that is not the pair order, so the exports of a
    # computed store gather its counts, scores and entries through a task table that is not the identity
    cost = [lens[x] * lens[y] for x in range(9) for y in range(x + 1, 9)]
    assert sorted(range(36), key=lambda p: -cost[p]) != list(range(36)) and max(cost) > 1000 * min(cost)
    assert [len(s) for s in sc.two_seqs()[1]] == [1, 30]
    assert sorted(len(s) for s in sc.five_seqs()[1]) == [1, 2, 17, 33, 80]
    runs = sc.shard_runs()
    assert {(k.split("-")[0], v[1]) for k, v in runs.items()} == {("two", 1), ("two", 2), ("two", 3), ("two", 4), ("five", 4), ("five", 7),
                                                                  ("five", 10), ("computed", 2), ("computed", 5), ("computed", 3)}
    # ranks without a pair, without a sequence to fold, with neither
    for world, neither in ((2, 0), (3, 0), (4, 1)):
        ranks = sc.world_split(1, world)
        assert sum(1 for r, (_, c) in enumerate(ranks) if c == 0 and r >= 2) == neither
    assert all(c > 0 for _, c in sc.world_split(10, 7)) and all(c == 1 for _, c in sc.world_split(10, 10))
    # strides that differ between the ranks, 0 on some: the pair counts and the folded sequences of world 5 on 9 sequences
    assert len({c for _, c in sc.world_split(36, 5)}) > 1


def test_a_threshold_of_two_keeps_nothing_and_phase_1_completes(oracle):
    """what the last two sharded worlds rely on: above a threshold of 2.0 the oracle keeps no base pair and no matching
    probability, and its phase 1 on the empty stores completes (every similarity 0, relaxed stores empty)"""
    names, seqs = sc.computed()
    bps = []
    for s in seqs:
        L = len(s)
        rp = np.zeros(L + 1, np.uint32); col = np.zeros(L * L + 1, np.uint32); val = np.zeros(L * L + 1, np.float32)
        assert oracle.lib.orc_fold_calculate(s.encode(), L, None, 2.0, rp.ctypes.data, col.ctypes.data, val.ctypes.data) == 0
        assert not rp.any()
        bps.append((rp, col[:0].copy(), val[:0].copy()))
    n = len(seqs)
    for x in range(n):
        for y in range(x + 1, n):
            for model in (0, 1):
                rp, col, val = oracle.align_calculate(seqs[x], seqs[y], 2.0, model)
                assert len(col) == 0 and not rp.any()
    for prm, bp in ((oracle.params(th_a=2.0), None), (oracle.params(fold_model=1), bps)):  # fold_model 1: the rows are supplied
        pl = oracle.pipeline(list(names), list(seqs), prm, bp=bp)
        pl.phase1()
        if bp is None:
            assert all(len(pl.mp(a, b)[1]) == 0 for a in range(n) for b in range(n) if a != b)
            assert np.array_equal(pl.sim(), np.eye(n, dtype=np.float32))
        else:
            assert all(len(pl.bp(x)[1]) == 0 for x in range(n))
            assert any(len(pl.mp(a, b)[1]) > 0 for a in range(n) for b in range(a + 1, n))
        pl.close()
