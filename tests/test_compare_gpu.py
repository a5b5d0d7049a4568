"""GPU tests of the alignment comparison (dafs_hip_alignment_compare and Context.alignment_compare) against the restatement of
DESIGN.md section 19 in tests/compare_ref.py: integers by value, quotients as float(a) / float(b)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import compare_ref as cr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = cr.NONE


@pytest.fixture(scope="module")
def ctx():
    """a fresh context on which no sequences are ever set: the call reads the two alignments alone"""
    from dafs_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _nested(rs, length):
    """a random nested structure as a partner array in left-column form"""
    ss, stack = [NONE] * length, []
    for c in range(length):
        u = rs.rand()
        if u < 0.3:
            stack.append(c)
        elif u < 0.6 and stack:
            ss[stack.pop()] = c
    return ss


def _case(n, len_r, seed):
    """Random sequences with 30 % gaps in R.  T has len_r + 7 columns: a random half of the rows get their gap positions drawn
    again, the rest keep R's with two runs shifted right by different amounts, so shared is neither 0 nor everything.  Masks at
    80 % on both sides, a random nested structure on each side, a random PP class on nine residues in ten."""
    rs = np.random.RandomState(seed)
    len_t = len_r + 7
    cell_r = np.full((n, len_r), 5, np.uint8)
    cell_t = np.full((n, len_t), 5, np.uint8)
    pp = np.full((n, len_t), 255, np.uint8)
    redraw = rs.rand(n) < 0.5
    for r in range(n):
        at_r = np.nonzero(rs.rand(len_r) >= 0.30)[0]
        codes = rs.randint(0, 5, len(at_r))
        if redraw[r]:
            at_t = np.sort(rs.choice(len_t, len(at_r), replace=False))
        else:
            first, second = sorted(rs.randint(0, 8, 2))
            cut = rs.randint(0, len(at_r) + 1)
            at_t = at_r + np.where(np.arange(len(at_r)) < cut, first, second)
        cell_r[r, at_r] = codes
        cell_t[r, at_t] = codes
        pp[r, at_t] = np.where(rs.rand(len(at_t)) < 0.9, rs.randint(0, 11, len(at_t)), 255)
    return dict(cell_r=cell_r, cell_t=cell_t, use_r=rs.rand(len_r) < 0.8, use_t=rs.rand(len_t) < 0.8, ss_r=np.array(_nested(rs, len_r), np.uint32),
                ss_t=np.array(_nested(rs, len_t), np.uint32), pp=pp)


def _want(case, masks=True, matrix=True):
    rows_r, rows_t = case["cell_r"].tolist(), case["cell_t"].tolist()
    use_r, use_t = (case["use_r"].tolist(), case["use_t"].tolist()) if masks else (None, None)
    want = cr.compare(rows_r, rows_t, use_r, use_t, case["ss_r"].tolist(), case["ss_t"].tolist(), case["pp"].tolist())
    if matrix:
        want["pair_shared"], want["pair_refp"], want["pair_testp"] = cr.pair_counts(cr.keys(rows_r, rows_t, use_r, use_t))
    return want


def _same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


INTS = ("residues", "k", "m", "shared", "refp", "testp", "colref", "colshared", "pp_residues", "pp_ref", "pp_shared", "tp", "nref", "ntest")
TOTALS = ("total_shared", "total_refp", "total_testp", "tc_reproduced", "tc_columns", "total_tp", "total_nref", "total_ntest")
QUOTIENTS = ("sps", "ppv", "tc", "sensitivity", "ss_ppv", "f")


def _check(got, want):
    """got: a Comparison, or the dict a child process saved from one"""
    get = got.get if isinstance(got, dict) else lambda k: getattr(got, k)
    for k in INTS:
        assert [int(x) for x in get(k)] == want[k], k
    for k in TOTALS:
        assert int(get(k)) == want[k], k
    assert [bool(x) for x in get("reproduced")] == want["reproduced"]
    for k in QUOTIENTS:
        assert _same_float(float(get(k)), want[k]), k
    for k in ("row_sps", "row_ppv", "pp_accuracy"):
        assert all(_same_float(float(x), y) for x, y in zip(get(k), want[k])) and len(get(k)) == len(want[k]), k
    if "pair_shared" in want:
        for k in ("pair_shared", "pair_refp", "pair_testp"):
            assert np.asarray(get(k)).tolist() == want[k], k
            # the other route: a row of a pair matrix sums to the row's count from cnt
            assert np.asarray(get(k), np.uint64).sum(axis=1).tolist() == want[k[5:]], k


def _run(ctx, case, masks=True, matrix=True):
    return ctx.alignment_compare(case["cell_r"], case["cell_t"], use_ref=case["use_r"] if masks else None, use_test=case["use_t"] if masks else None,
                                 ss_ref=case["ss_r"], ss_test=case["ss_t"], pp=case["pp"], matrix=matrix)


# 17, 64, 65, 130 cross the 16- and 64-row tile edges, 130 has a tile wholly below the diagonal; 63, 64, 65 cross the wavefront
# of the map kernel, 200 (and its 207) needs several of its steps
@pytest.mark.parametrize("len_r", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("n", [2, 3, 17, 64, 65, 130])
def test_random_alignments_equal_the_restatement(ctx, n, len_r):
    case = _case(n, len_r, seed=1000 * n + len_r)
    want = _want(case)
    got = _run(ctx, case)
    _check(got, want)
    if len_r >= 63 and n >= 3:  # the inputs do what they are meant to
        assert 0 < want["total_shared"] < want["total_refp"] and want["total_nref"] > 0
    # without the matrices nothing else changes; text rows give the same cells
    plain = _run(ctx, case, matrix=False)
    assert not hasattr(plain, "pair_shared")
    _check(plain, {k: v for k, v in want.items() if not k.startswith("pair_")})
    if n == 17:
        text = [["".join("ACGUN-"[v] for v in row) for row in case[k]] for k in ("cell_r", "cell_t")]
        again = ctx.alignment_compare(text[0], text[1], use_ref=case["use_r"], use_test=case["use_t"], matrix=True)
        assert not hasattr(again, "tp") and not hasattr(again, "pp_ref")
        assert again.pair_shared.tolist() == want["pair_shared"] and again.shared.tolist() == want["shared"]


def test_without_masks(ctx):
    case = _case(65, 65, seed=5)
    _check(_run(ctx, case, masks=False), _want(case, masks=False))


def test_known_answer(ctx):
    from dafs_amd import capi
    got = ctx.alignment_compare(["ACGU-", "AC-U-", "-CGUA"], ["ACGU--", "A-CU--", "--CGUA"], ss_ref=cr.brackets("(..)."),
                                ss_test=cr.brackets("(..).."), matrix=True)
    assert list(zip(got.shared.tolist(), got.refp.tolist(), got.testp.tolist())) == [(2, 6, 5), (3, 5, 5), (1, 5, 4)]
    assert (got.total_shared, got.total_refp, got.total_testp) == (3, 8, 7) and got.sps == 0.375 and got.ppv == 3.0 / 7.0
    assert got.k.tolist() == [2, 3, 2, 3, 1] and got.colshared.tolist() == [1, 1, 0, 1, 0]
    assert got.reproduced.tolist() == [True, False, False, False, False] and got.tc == 0.25
    pairs = {(r, s): (int(got.pair_shared[r, s]), int(got.pair_refp[r, s]), int(got.pair_testp[r, s])) for r in range(3) for s in range(r + 1, 3)}
    assert pairs == {(0, 1): (2, 3, 3), (0, 2): (0, 3, 2), (1, 2): (1, 2, 2)}
    assert list(zip(got.tp.tolist(), got.nref.tolist(), got.ntest.tolist())) == [(1, 1, 1), (1, 1, 1), (0, 0, 0)]
    # the symmetric form of a structure is the same structure
    sym = [3, capi.NONE, capi.NONE, 0, capi.NONE]
    assert ctx.alignment_compare(["ACGU-", "AC-U-", "-CGUA"], ["ACGU--", "A-CU--", "--CGUA"], ss_ref=sym, ss_test=cr.brackets("(..)..")).total_tp == 2


def test_an_alignment_agrees_with_itself(ctx):
    case = _case(65, 200, seed=9)
    got = ctx.alignment_compare(case["cell_r"], case["cell_r"], use_ref=case["use_r"], use_test=case["use_r"], ss_ref=case["ss_r"],
                                ss_test=case["ss_r"], matrix=True)
    assert got.sps == 1.0 and got.ppv == 1.0 and got.tc == 1.0
    assert got.tp.tolist() == got.nref.tolist() == got.ntest.tolist() and got.total_tp > 0 and got.f == 1.0
    assert (got.pair_shared == got.pair_refp).all() and (got.pair_shared == got.pair_testp).all()
    assert got.shared.tolist() == got.refp.tolist() == got.testp.tolist()


CHILD = ("import sys, numpy as np; sys.path.insert(0, %r); from dafs_amd import capi; ctx = capi.Context(0); c = dict(np.load(sys.argv[1])); "
         "g = ctx.alignment_compare(c['cell_r'], c['cell_t'], use_ref=c['use_r'], use_test=c['use_t'], ss_ref=c['ss_r'], ss_test=c['ss_t'], pp=c['pp'], "
         "matrix=True); ctx.close(); np.savez(sys.argv[2], **{k: np.asarray(v) for k, v in vars(g).items()})" % ROOT)


def test_chunking_and_bands_change_no_bit(tmp_path):
    """130 x 200 with an LDS stage of 1 column (the smallest), of 7 (200 = 28 * 7 + 4 and 207 = 29 * 7 + 4: a ragged last chunk on
    both sides) and the default, and with one workgroup per launch, each in a process of its own: the library reads the switches
    when it is called, but a process keeps its environment"""
    case = _case(130, 200, seed=77)
    np.savez(str(tmp_path / "case.npz"), **case)
    want = _want(case)
    outs = []
    for name, value in ((None, None), ("DAFS_CMP_CHUNK_COLS", "1"), ("DAFS_CMP_CHUNK_COLS", "7"), ("DAFS_CMP_BAND_BLOCKS", "1")):
        env = {k: v for k, v in os.environ.items() if k not in ("DAFS_CMP_CHUNK_COLS", "DAFS_CMP_BAND_BLOCKS")}
        if name:
            env[name] = value
        out = str(tmp_path / ("out_%s_%s.npz" % (name, value)))
        subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "case.npz"), out], check=True, timeout=120, env=env)
        outs.append(dict(np.load(out)))
        _check(outs[-1], want)
    for other in outs[1:]:
        assert sorted(other) == sorted(outs[0])
        for k in outs[0]:
            assert outs[0][k].tobytes() == other[k].tobytes(), k


def test_refusals_leave_outputs_and_context(ctx):
    import ctypes as C
    from dafs_amd import capi
    case = _case(12, 30, seed=41)
    good = _run(ctx, case)
    bad = case["cell_t"].copy()
    r = int(np.argmax((bad <= 4).sum(axis=1) > 0))
    c = int(np.nonzero(bad[r] <= 4)[0][0])
    bad[r, c] = (bad[r, c] + 1) % 5  # row r + 1 holds another residue
    with pytest.raises(capi.DafsHipError, match="row %d " % (r + 1)):
        ctx.alignment_compare(case["cell_r"], bad)
    missing = case["cell_t"].copy()
    missing[r, c] = 5  # or one residue fewer
    with pytest.raises(capi.DafsHipError, match="row %d " % (r + 1)):
        ctx.alignment_compare(case["cell_r"], missing)
    # the library itself: the outputs stay as they were
    marks = dict(shared=np.full(12, 77, np.uint64), total=np.full(3, 77, np.uint64), score=np.full(3, 7.0), k=np.full(30, 77, np.uint32),
                 pair_shared=np.full((12, 12), 77, np.uint32))

    def call(n, len_r, len_t, cell_t, **extra):
        arrays = dict(marks, **extra)
        out = capi.CompareOut(**{k: v.ctypes.data for k, v in arrays.items()})
        return capi._alignment_compare(ctx._h, n, len_r, len_t, case["cell_r"].ctypes.data, cell_t.ctypes.data, None, None, None, None, None, C.byref(out))

    high = case["cell_t"].copy()
    high[3, 3] = 6
    assert call(12, 30, 37, bad) == -1 and "row %d " % (r + 1) in capi._last_error().decode()
    assert call(12, 30, 37, missing) == -1 and call(12, 30, 37, high) == -1
    # sizes beyond the limits are refused from the sizes alone, before a cell is read
    cell_t = case["cell_t"]
    assert call(1, 30, 37, cell_t) == -1 and call((1 << 20) + 1, 30, 37, cell_t) == -1
    assert call(12, (1 << 20) + 1, 37, cell_t) == -1 and call(12, 30, (1 << 20) + 1, cell_t) == -1 and call(12, 0, 37, cell_t) == -1
    assert call(12, 1 << 15, (1 << 15) + 1, cell_t) == -1  # len_r * len_t above 2^30
    assert call(16385, 1, 1, cell_t) == -1  # a pair matrix beyond its limit
    assert call(12, 30, 37, cell_t, tp=np.zeros(12, np.uint64)) == -1  # a structure output without structures
    assert call(12, 30, 37, cell_t, pp_count=np.zeros(33, np.uint64)) == -1
    assert all((v == (7.0 if k == "score" else 77)).all() for k, v in marks.items())
    crossed = case["ss_r"].copy()
    crossed[:4] = [2, 2, NONE, NONE]  # column 2 in two pairs
    with pytest.raises(capi.DafsHipError):
        ctx.alignment_compare(case["cell_r"], case["cell_t"], ss_ref=crossed, ss_test=case["ss_t"])
    pp = case["pp"].copy()
    pp[0, 0] = 11
    with pytest.raises(capi.DafsHipError):
        ctx.alignment_compare(case["cell_r"], case["cell_t"], pp=pp)
    with pytest.raises(ValueError):
        ctx.alignment_compare(case["cell_r"], case["cell_t"], ss_ref=case["ss_r"])
    # the next call is correct
    plain = _run(ctx, case, masks=False)  # call() passes no masks
    assert call(12, 30, 37, cell_t) == 0 and marks["shared"].tolist() == plain.shared.tolist() and marks["pair_shared"].tolist() == plain.pair_shared.tolist()
    again = _run(ctx, case)
    for k, v in vars(good).items():
        assert np.asarray(getattr(again, k)).tobytes() == np.asarray(v).tobytes(), k
    _check(again, _want(case))
    ctx.stage_timing(True)
    try:
        _run(ctx, case)
        names = set(ctx.stage_report())
    finally:
        ctx.stage_timing(False)
    assert names >= {"k_cmp_map", "k_cmp_count_cols", "k_cmp_count", "k_cmp_residue", "k_cmp_columns", "k_cmp_ss", "k_cmp_pairs<shared>",
                     "k_cmp_pairs<occupancy>"}
