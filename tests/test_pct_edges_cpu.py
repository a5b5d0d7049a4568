"""The hand-made stores of pct_cases.py do what they are for -- on the oracle alone, no device.  test_pct_edges_gpu.py
compares the kernels with the oracle on these cases; what is asserted here keeps a later change of the builders, of the
seeds or of consistency_parts' pool guesses from hollowing those comparisons out silently."""
import numpy as np
import pytest

import pct_cases as pc


def _nnz(m):
    return int(m[0][-1])


@pytest.mark.parametrize("make", pc.ALL, ids=pc.IDS)
def test_stores_are_well_formed(make):
    case = make()
    for (x, y), (rp, col, val) in case.mps.items():
        assert len(rp) == case.lens[x] + 1 and rp[0] == 0 and len(col) == len(val) == rp[-1]
        for i in range(case.lens[x]):
            c = col[rp[i]:rp[i + 1]].astype(np.int64)
            assert np.all(np.diff(c) > 0) and (len(c) == 0 or c[-1] < case.lens[y])
        assert np.all(val > 0) and np.all(val <= 1)
    for x, (rp, col, val) in enumerate(case.bps):
        assert len(rp) == case.lens[x] + 1 and rp[0] == 0 and len(col) == len(val) == rp[-1]
        for i in range(case.lens[x]):
            c = col[rp[i]:rp[i + 1]].astype(np.int64)
            assert np.all(np.diff(c) > 0) and (len(c) == 0 or (c[0] > i and c[-1] < case.lens[x]))
        assert np.all(val > 0) and np.all(val <= 1)


def test_long_rows(oracle):
    case = pc.long_rows()
    fwd = set(int(v) for v in pc.row_lengths(case.mp(0, 1)))
    assert {0, 1, 15, 16, 17, 31, 32, 33, 40} <= fwd
    # a wavefront of k_pct_rows holds output rows 4q .. 4q + 3: each one of pair (0, 1) pairs a long row with a short or empty one
    for q in range(5):
        four = pc.row_lengths(case.mp(0, 1))[4 * q:4 * q + 4]
        assert four.max() > 16 and four.min() <= 1
    tr = pc.transposed_row_lengths(case.mp(1, 2), 24)  # the rows of mp[2][1]
    assert tr[3] == 33 and tr[20] == 17 and 0 < tr.min() < 16
    bpl = set(int(v) for x in range(3) for v in pc.row_lengths(case.bps[x]))
    assert {0, 1, 16, 17, 33} <= bpl
    # the long rows are read: the long bp[1][0] is opened by a row of another sequence (mp[0][1][i] names k = 0), the long
    # rows of mp[2][1] are c-rows of sequence 1's transform (a base pair of sequence 2 ends in column 3)
    assert 0 in case.mp(0, 1)[1][:40] and 3 in case.bps[2][1]
    for w in case.weights:
        ref = pc.reference(oracle, case, *w)
        assert all(_nnz(ref.mp[p]) > 0 for p in case.pairs)
        assert sum(_nnz(b) for b in ref.bp) > 0


@pytest.mark.parametrize("n", [16, 17, 33])
def test_chunks(oracle, n):
    case = pc.chunks(n)
    assert case.n == n and len(set(case.lens)) > 1 and min(case.lens) >= 9 and max(case.lens) <= 24
    nnz = {p: _nnz(case.mp(*p)) for p in case.pairs}
    empty_pairs = [p for p in case.pairs if nnz[p] == 0]
    assert 0 < len(empty_pairs) < len(case.pairs) // 4
    assert any(0 in pc.row_lengths(case.mp(*p)) for p in case.pairs if nnz[p])
    per_row = sum(nnz.values()) / sum(case.lens[x] for x, y in case.pairs if nnz[(x, y)])
    assert 2.0 < per_row < 4.0
    if n > 16:  # the chunks behind the first have something to add: the last sequence's pairs are not all empty
        assert sum(nnz[(x, n - 1)] for x in range(n - 1)) > 0
    ref = pc.reference(oracle, case)
    for x, y in case.pairs:
        assert ref.sim[x, y] == ref.sim[y, x] and (ref.sim[x, y] == 0) == (nnz[(x, y)] == 0)
        if nnz[(x, y)]:
            assert _nnz(ref.mp[(x, y)]) > 0, (x, y)
    assert all(_nnz(b) > 0 for b in ref.bp)


def test_lengths(oracle):
    case = pc.lengths()
    assert case.lens == (1, 2, 15, 16, 17, 31, 32, 33)
    ref = pc.reference(oracle, case)
    assert all(_nnz(ref.mp[p]) > 0 for p in case.pairs)


@pytest.mark.parametrize("make", [pc.lengths, lambda: pc.chunks(17)], ids=["lengths", "chunks_17"])
def test_task_table_has_padding(make):
    """pct_task_order (DAFS_HIP_PCT_YORDER=1) pads its table to a multiple of 8 workgroups: these cases leave padding entries"""
    assert make().row_blocks() % 8 != 0


def test_empty(oracle):
    case = pc.empty()
    assert all(_nnz(m) == 0 for m in case.mps.values()) and all(_nnz(b) > 0 for b in case.bps)
    for w in case.weights:
        ref = pc.reference(oracle, case, *w)
        assert not ref.sim[~np.eye(4, dtype=bool)].any()  # hence every weight of the matching transform, and sum_w, is 0
        assert all(_nnz(m) == 0 for m in ref.mp.values())
        # the base-pairing transform keeps the term y == x (sim[x][x] = 1): nothing but the input's own pairs
        for got, had in zip(ref.bp, case.bps):
            assert np.array_equal(got[0], had[0]) and np.array_equal(got[1], had[1])


@pytest.mark.parametrize("make", [pc.wide_1000, pc.wide_top], ids=["wide_1000", "wide_top"])
def test_wide(oracle, make):
    case = make()
    L = case.lens[2]
    assert case.lens[:2] == (40, 33) and L == max(case.lens)
    for x in (0, 1):
        assert {0, 1, L - 2, L - 1} <= set(int(c) for c in case.mp(x, 2)[1])
    rp, col, _ = case.bps[2]
    assert col[rp[0]:rp[1]][-1] == L - 1 and list(col[rp[L - 3]:rp[L - 2]]) == [L - 2]
    ref = pc.reference(oracle, case)
    for x in (0, 1):  # the top of the accumulator row is written and kept, in both transforms
        kept = set(int(c) for c in ref.mp[(x, 2)][1])
        assert {0, L - 1} <= kept, (x, sorted(kept)[:3], sorted(kept)[-3:])
    assert L - 1 in ref.bp[2][1] and L - 2 in ref.bp[2][1]


def test_limits_are_the_kernels():
    """MATCH_TOP and BP_TOP restate pct_match_lds_bytes / pct_bp_lds_bytes with the row_cap of pct_match_launch /
    pct_bp_launch (pct.hip) for a family of three against kPctLdsBytes = 150 KiB"""
    def match_bytes(L, fam=3):
        row_cap = L + ((28 - L) & 31)
        return fam * 32 + ((fam + 1) & ~1) * 4 + 16 * (row_cap + 16 + (16 * 2 + 20 + 16)) * 4 + 64

    def bp_bytes(L, fam=3):
        row_cap = L + ((12 - L) & 31)
        return fam * 32 + ((fam + 1) & ~1) * 4 + 16 * (row_cap * 4 + 16 * 8 + 20 * 4 + 16 * 4) + 64

    cap = 150 * 1024
    assert match_bytes(pc.MATCH_TOP) <= cap < match_bytes(pc.MATCH_TOP + 1) and pc.MATCH_TOP == 2300
    assert bp_bytes(pc.BP_TOP) <= cap < bp_bytes(pc.BP_TOP + 1) and pc.BP_TOP == 2316
    assert match_bytes(pc.MATCH_TOP) > 64 * 1024 and match_bytes(1000) > 64 * 1024  # the LDS opt-in matters in both wide cases


def test_overflow(oracle):
    case = pc.overflow()
    ref = pc.reference(oracle, case)
    nnz_in = sum(_nnz(m) for m in case.mps.values())
    nnz_out = sum(_nnz(ref.mp[p]) for p in case.pairs)
    # capi_pct.cpp, consistency_match: `uint64_t cap = std::max<uint64_t>(raw.pool_used * 2 + 1024, out.pool_cap_hint);`
    # (pool_used counts every entry twice, rows and transposed rows, and so does k_pct_emit's 2 * nnz; a fresh context's hint is 0)
    first_mp = 2 * (2 * nnz_in) + 1024
    assert (nnz_in, nnz_out) == (8000, 24000)
    assert 2 * nnz_out > first_mp, "the matching pool's first guess holds the result: the case needs resizing"
    bp_in = sum(_nnz(b) for b in case.bps)
    bp_out = sum(_nnz(b) for b in ref.bp)
    # capi_pct.cpp, consistency_bp: `uint64_t cap = std::max<uint64_t>(4 * in.total_nnz + 1024, 16ull * c->off[n]);`
    first_bp = max(4 * bp_in + 1024, 16 * sum(case.lens))
    assert (bp_in, bp_out) == (12, 4680)
    assert bp_out > first_bp, "the base-pairing pool's first guess holds the result: the case needs resizing"
