"""GPU tests of dafs_hip_update_basepairing (Context.update_basepairing: --bp-update / --bp-update1) and of the multi-row
average behind Context.consensus_structure(..., want_p=True), on the hand-made alignments of bp_update_cases.py, cell by cell
against orc_pipeline_update_basepairing / orc_pipeline_average_basepairing.  Every comparison is bit for bit; what the
cases hold and that the oracle's entry points are the reference's functions is test_bp_update_cpu.py's part."""
import numpy as np
import pytest

import bp_update_cases as B
from dafs_amd import capi

pytestmark = pytest.mark.gpu
NONE = B.NONE
FORMS = [{"DAFS_HIP_CF_THREADS": "64"}, {"DAFS_HIP_CF_NORING": "1"}]


@pytest.fixture(scope="module")
def want(oracle):
    """per case the oracle's plain average of the supplied free rows and its updated matrix (computed once, read-only), and
    for mid and wide the chain decode, update, decode"""
    out = {}
    for key in B.KEYS:
        c = B.CASES[key]
        pl = B.oracle_pipeline(oracle, c)
        w = dict(avg=pl.average_basepairing(c.idx, c.mask), upd=pl.update_basepairing(c.idx, c.mask, c.ss))
        if key in ("mid", "wide"):
            w["s0"], w["ss0"] = oracle.nussinov(w["avg"], None, B.TH)
            w["upd0"] = pl.update_basepairing(c.idx, c.mask, w["ss0"])
            w["s1"], w["ss1"] = oracle.nussinov(w["upd0"], None, B.TH)
        pl.close()
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.flags.writeable = False
        out[key] = w
    return out


def _context(case, rows=None):
    c = capi.Context(0)
    c.set_sequences(case.seqs)
    if rows is not None:
        c.set_bp(rows)
    return c


def _same(got, want, at):
    assert got.shape == want.shape and got.dtype == want.dtype, at
    assert got.tobytes() == want.tobytes(), (at, int((got != want).sum()), float(np.abs(got - want).max()))


@pytest.mark.parametrize("key", B.KEYS)
def test_update_matrix(want, key):
    """sequences only: the call folds for itself"""
    case = B.CASES[key]
    c = _context(case)
    try:
        _same(c.update_basepairing(case.idx, case.mask, case.ss), want[key]["upd"], key)
    finally:
        c.close()


@pytest.mark.parametrize("key", B.KEYS)
def test_plain_average(oracle, want, key):
    case = B.CASES[key]
    c = _context(case, B.free_rows(oracle, case))
    try:
        _same(c.consensus_structure(case.idx, case.mask, B.TH, want_p=True)[2], want[key]["avg"], key)
    finally:
        c.close()


def test_by_row_store_does_not_leak_between_calls(want):
    """wide, small, wide on one context that holds the sequences of both, nothing set in between: c->bp_rows is written
    anew by every call, the short rows after the long ones and the long ones after the short.  The oracle folds a row by
    its residues, so its answers are those of a context of the case's own (test_update_matrix)."""
    wide, small = B.CASES["wide"], B.CASES["small"]
    shifted = small.idx + np.uint32(len(wide.seqs))
    c = capi.Context(0)
    try:
        c.set_sequences(wide.seqs + small.seqs)
        for idx, case in ((wide.idx, wide), (shifted, small), (wide.idx, wide)):
            first = c.update_basepairing(idx, case.mask, case.ss)
            _same(first, want[case.key]["upd"], case.key)
            _same(c.update_basepairing(idx, case.mask, case.ss), first, case.key)
    finally:
        c.close()


@pytest.mark.parametrize("env", FORMS, ids=["threads64", "noring"])
@pytest.mark.parametrize("key", ["mid", "wide"])
def test_fold_forms(want, monkeypatch, key, env):
    case = B.CASES[key]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = _context(case)
    try:
        _same(c.update_basepairing(case.idx, case.mask, case.ss), want[key]["upd"], (key, env))
    finally:
        c.close()


@pytest.mark.parametrize("key", ["mid", "wide"])
def test_the_two_decodes_around_an_update(oracle, want, key):
    """decode the plain average, update under that structure, decode the result: pipeline.py's --bp-update step and
    _final_structure"""
    case, w = B.CASES[key], want[key]
    assert int(np.sum(w["ss0"] != NONE)) >= 1
    c = _context(case, B.free_rows(oracle, case))
    try:
        s0, ss0, _ = c.consensus_structure(case.idx, case.mask, B.TH)
        assert ss0.tobytes() == w["ss0"].tobytes() and np.float32(s0).tobytes() == np.float32(w["s0"]).tobytes()
        p = c.update_basepairing(case.idx, case.mask, ss0)
        _same(p, w["upd0"], key)
        s1, ss1 = c.nussinov(p, None, B.TH)
        assert ss1.tobytes() == w["ss1"].tobytes() and np.float32(s1).tobytes() == np.float32(w["s1"]).tobytes()
    finally:
        c.close()


def _raw(c, idx, mask, ss, out):
    idx = np.ascontiguousarray(idx, np.uint32); mask = np.ascontiguousarray(mask, np.uint8); ss = np.ascontiguousarray(ss, np.uint32)
    return capi._update_basepairing(c._h, mask.shape[0], mask.shape[1], idx.ctypes.data, mask.ctypes.data, ss.ctypes.data, out.ctypes.data)


def test_refusals_leave_the_output_and_the_context_alone(want):
    case = B.CASES["small"]
    short = case.mask.copy()
    short[1, np.flatnonzero(short[1])[0]] = 0  # one residue of the second row is not placed
    beyond = case.idx.copy()
    beyond[2] = len(case.seqs)  # a sequence index beyond the context
    c = _context(case)
    try:
        for idx, mask in ((case.idx, short), (beyond, case.mask)):
            out = np.full((case.L, case.L), -7.5, np.float32)
            assert _raw(c, idx, mask, case.ss, out) == -1  # DAFS_HIP_EINVAL
            assert np.all(out == -7.5)
            with pytest.raises(capi.DafsHipError):
                c.update_basepairing(idx, mask, case.ss)
            _same(c.update_basepairing(case.idx, case.mask, case.ss), want["small"]["upd"], "small")
        c.fold_begin()  # a batch in flight owns the folding workspaces
        out = np.full((case.L, case.L), -7.5, np.float32)
        assert _raw(c, case.idx, case.mask, case.ss, out) == -1
        assert np.all(out == -7.5)
        with pytest.raises(capi.DafsHipError):
            c.update_basepairing(case.idx, case.mask, case.ss)
        c.fold_end()
        _same(c.update_basepairing(case.idx, case.mask, case.ss), want["small"]["upd"], "small")
    finally:
        c.close()
