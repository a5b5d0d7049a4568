"""GPU parity of sweep 4 of the pair kernels (pair_sweeps.h): the entries of a pair are staged window by window in LDS
and copied out coalesced.  Every case goes bit for bit against the oracle through test_pairhmm_gpu's checker (row
pointers, columns and values of both matrices, similarity); the oracle also confirms that each set still puts the
window edges where the case wants them."""
import os
import random

import numpy as np
import pytest

import pair_raw
from dafs_amd import synth
from test_pair_records_gpu import LOW_COMPLEXITY
from test_pairhmm_gpu import _check_set

pytestmark = pytest.mark.gpu

_NNZ = {}


def _nnz(oracle, seqs, th, model=0):
    """entries of every pair of the set (oracle), computed once per set"""
    key = (tuple(seqs), th, model)
    if key not in _NNZ:
        n = len(seqs)
        _NNZ[key] = [len(oracle.align_calculate(seqs[i], seqs[j], th, model)[1]) for i in range(n) for j in range(i + 1, n)]
    return _NNZ[key]


def _run(oracle, seqs, th=0.01, group=None, model=0, window=None, width=None):
    env = {"DAFS_HIP_EMIT_WINDOW": window, "DAFS_HIP_FORCE_WIDTH": width}
    for k, v in env.items():
        if v is not None:
            os.environ[k] = str(v)
    try:
        _check_set(oracle, seqs, th=th, force_group=group, model=model)
    finally:
        for k in env:
            os.environ.pop(k, None)


def _rand(n, seed):
    r = random.Random(seed)
    return "".join(r.choice("ACGU") for _ in range(n))


@pytest.mark.parametrize("window", [16, 64, 128])
@pytest.mark.parametrize("group", [16, 32, 64])
def test_window_crossings_at_a_forced_small_window(oracle, group, window):
    """Window edges inside a record's run of entries, inside a row and inside a column; the seam between the row half and
    the transposed half on a window edge (nnz = 384 = 24 * 16 = 6 * 64 = 3 * 128) and inside a window (the other pairs).
    G = 64 at window 16 is rounded up to 64."""
    nnz = _nnz(oracle, LOW_COMPLEXITY, 0.01)
    assert all(2 * k > 3 * 128 for k in nnz), nnz  # at least four windows at every size
    assert 384 in nnz, nnz
    assert any(k % 16 for k in nnz), nnz
    _run(oracle, LOW_COMPLEXITY, group=group, window=window)
    _run(oracle, LOW_COMPLEXITY, group=group, window=window, model=1)


@pytest.mark.parametrize("th", [0.01, 0.002])
@pytest.mark.parametrize("group", [None, 16, 32, 64])
def test_several_windows_at_the_derived_size(oracle, group, th):
    seqs = [s for _, s in synth.random_set(4, 150, seed=12345)]
    assert all(2 * k > 1024 for k in _nnz(oracle, seqs, th)), _nnz(oracle, seqs, th)
    _run(oracle, seqs, th=th, group=group)


def test_empty_and_nearly_empty_pairs(oracle):
    seqs = [s for _, s in synth.random_set(6, 40, seed=7)]
    few = _nnz(oracle, seqs, 0.9)
    assert min(few) >= 1 and max(few) <= 14, few
    assert not any(_nnz(oracle, seqs, 0.9, 1))  # CONTRAlign: nothing to copy out, row pointers all zero
    for model in (0, 1):
        for group in (None, 16, 64):
            _run(oracle, seqs, th=0.9, group=group, model=model)


@pytest.mark.parametrize("group", [16, 32, 64])
def test_groups_that_run_out_at_different_times(oracle, group):
    """Three pairs of very unequal size in one or two wavefronts; under G = 32 and 64 the last group of a wavefront is
    inactive.  Then one pair alone: one active group."""
    seqs = ["ACGU" * 3, "ACGU" * 15, "GGGAAACCC"]
    assert sorted(_nnz(oracle, seqs, 0.01)) == [31, 137, 160], _nnz(oracle, seqs, 0.01)
    for model in (0, 1):
        _run(oracle, seqs, group=group, model=model)
        _run(oracle, seqs, group=group, model=model, window=32)
        _run(oracle, seqs[:2], group=group, model=model)


def test_width_w_and_w_minus_1(oracle):
    """G = 32, W = 3: a wavefront runs two columns per lane while its longest second sequence has at most
    G (W - 1) - 1 = 63 residues, three from 64 on."""
    first = _rand(50, 1)
    for n in (62, 63, 64):
        _run(oracle, [first, _rand(n, n)], group=32, width=3, window=32)
    _run(oracle, [first, _rand(62, 62), _rand(63, 63), _rand(64, 64)], group=32, width=3, window=32)


def test_pool_too_small_is_a_status(oracle, tmp_path):
    """The raw launch, as bench.py drives it, with half the pool the pairs need: DAFS_HIP_EOVERFLOW, the pairs whose
    reservation fitted are complete, nothing else in the pool is touched, and neither is the tail of the allocations
    behind pool_cap.  A child process, so that torch starts the HIP runtime before the library is loaded."""
    seqs = [_rand(40, 11), _rand(41, 12), _rand(39, 13)]
    th = 0.01
    pairs = [(0, 1), (0, 2), (1, 2)]
    want = [oracle.align_calculate(seqs[i], seqs[j], th, 0) for i, j in pairs]
    need = 2 * sum(len(w[1]) for w in want)
    pool_cap = need // 2
    tail = 4096
    CANARY = 0x5A5A5A5A
    # run() asserts that the child's return code is 0: a handled status, not a fault
    got = pair_raw.run(tmp_path, [pair_raw.spec(oracle, 0, th, seqs, pairs, CANARY, pool_cap=pool_cap)], tail=tail)[0]
    assert int(got["status"][0]) == -5, got["status"]  # DAFS_HIP_EOVERFLOW
    h_col, h_val = got["col"], got["val"]
    h_off, h_nnz = got["pair_off"], got["pair_nnz"]
    untouched = np.ones(pool_cap + tail, bool)
    fitted = 0
    for p, (rp, wcol, wval) in enumerate(want):
        k = len(wcol)
        assert int(h_nnz[p]) == k
        o = int(h_off[p])
        if o + 2 * k > pool_cap:
            continue
        fitted += 1
        assert np.array_equal(h_col[o:o + k], wcol)
        assert h_val[o:o + k].tobytes() == wval.tobytes()
        rows = np.repeat(np.arange(len(rp) - 1, dtype=np.uint32), np.diff(rp))
        order = np.lexsort((rows, wcol))
        assert np.array_equal(h_col[o + k:o + 2 * k], rows[order])
        assert h_val[o + k:o + 2 * k].tobytes() == wval[order].tobytes()
        untouched[o:o + 2 * k] = False
    assert 1 <= fitted < 3, fitted
    assert np.all(h_col[untouched] == CANARY) and np.all(h_val[untouched] == CANARY)
    assert np.all(h_col[pool_cap:] == CANARY) and np.all(h_val[pool_cap:] == CANARY)
