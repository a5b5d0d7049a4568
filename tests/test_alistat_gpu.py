"""GPU tests of the alignment statistics (dafs_hip_alignment_identity, dafs_hip_alignment_weights, dafs_host_nr_select and
their Python drivers) against the restatement of DESIGN.md section 18 in tests/alistat_ref.py, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import alistat_ref as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = ar.NONE


@pytest.fixture(scope="module")
def ctx():
    """a fresh context on which no sequences are ever set: the calls read the alignment alone"""
    from dafs_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _random_cells(n, length, seed, gaps=0.30, other=0.05):
    """random cells with 30 % gaps and 5 % N; every row keeps a residue"""
    rs = np.random.RandomState(seed)
    cell = rs.randint(0, 4, (n, length)).astype(np.uint8)
    if n > 1:  # related rows, so that identities spread
        cell[n // 2:] = cell[0]
        redraw = rs.rand(n - n // 2, length) < 0.4
        cell[n // 2:][redraw] = rs.randint(0, 4, int(redraw.sum()))
    draw = rs.rand(n, length)
    cell[draw < gaps] = 5
    cell[(draw >= gaps) & (draw < gaps + other)] = 4
    for r in range(n):
        if (cell[r] > 4).all():
            cell[r, r % length] = r % 4
    return cell


def _want(cell, use=None, cand=None, t=None):
    rows = [[int(v) for v in row] for row in cell]
    res, ident, aligned = ar.counts(rows, use)
    near, ni, nd = ar.nearest(res, ident, cand)
    out = dict(res=res, ident=ident, aligned=aligned, nearest=near, nearest_ident=ni, nearest_den=nd, weights=ar.weights(rows, use))
    if t is not None:
        out["red"] = ar.red_matrix(res, ident, t)
    return out


def _check(got, weights, want):
    for k in ("res", "nearest", "nearest_ident", "nearest_den"):
        assert [int(x) for x in getattr(got, k)] == want[k], k
    if hasattr(got, "ident"):
        assert got.ident.tolist() == want["ident"] and got.aligned.tolist() == want["aligned"]
    if "red" in want:
        assert got.red.tolist() == ar.red_bits(want["red"])
    for r, s in enumerate(want["nearest"]):
        if s == NONE:
            assert np.isnan(got.pid_nearest[r])
        else:
            assert got.pid_nearest[r] == float(want["nearest_ident"][r]) / float(want["nearest_den"][r])
    if weights is not None:
        assert np.asarray(weights, np.float64).tobytes() == np.array(want["weights"], np.float64).tobytes()


# 63, 64, 65 cross the 64-column word; 17, 64, 65, 130 the 16- and 64-row tile edges; 130 has a tile wholly below the diagonal
@pytest.mark.parametrize("length", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 65, 130])
def test_random_alignments_equal_the_restatement(ctx, n, length):
    cell = _random_cells(n, length, seed=100 * n + length)
    want = _want(cell, t=0.75)
    got = ctx.alignment_identity(cell, nr=0.75, matrix=True)
    _check(got, ctx.alignment_weights(cell), want)
    # text rows give the same cells; without the matrices and the bits nothing else changes
    text = ["".join("ACGUN-"[v] for v in row) for row in cell]
    plain = ctx.alignment_identity(text)
    assert not hasattr(plain, "ident") and not hasattr(plain, "red")
    bits = ctx.alignment_identity(cell, nr=0.75, nearest=False)  # the bits alone: no nearest pass
    assert not hasattr(bits, "nearest") and bits.red.tolist() == got.red.tolist() and bits.res.tolist() == got.res.tolist()
    _check(plain, ctx.alignment_weights(text), {k: v for k, v in want.items() if k != "red"})


CHILD = ("import sys, numpy as np; sys.path.insert(0, %r); from dafs_amd import capi; ctx = capi.Context(0); cell = np.load(sys.argv[1]); "
         "use = np.arange(cell.shape[1]) %% 7 != 3; cand = np.arange(cell.shape[0]) %% 3 != 1; "
         "a = ctx.alignment_identity(cell, use=use, cand=cand, nr=0.6, matrix=True); w = ctx.alignment_weights(cell, use=use); ctx.close(); "
         "np.savez(sys.argv[2], res=a.res, ident=a.ident, aligned=a.aligned, nearest=a.nearest, ni=a.nearest_ident, nd=a.nearest_den, red=a.red, w=w)" % ROOT)


def test_chunking_changes_no_bit(tmp_path):
    """130 x 200 (4 words) with an LDS stage of 1, 2 and the default 4 words, each in a process of its own; the first also
    splits every pass into launches of at most 5 workgroups (bands of rows: what keeps a launch of 2^20 rows under 2^32
    work-items)"""
    cell = _random_cells(130, 200, seed=7)
    np.save(str(tmp_path / "cell.npy"), cell)
    outs = []
    for chunk in ("1", "2", None):
        env = {k: v for k, v in os.environ.items() if k != "DAFS_ALI_CHUNK_WORDS"}
        env.pop("DAFS_ALI_BAND_BLOCKS", None)
        if chunk:
            env["DAFS_ALI_CHUNK_WORDS"] = chunk
        if chunk == "1":
            env["DAFS_ALI_BAND_BLOCKS"] = "5"  # 9 x 3 tiles: bands of one block of rows, nine launches per pass
        out = str(tmp_path / ("out%s.npz" % chunk))
        subprocess.run([sys.executable, "-c", CHILD, str(tmp_path / "cell.npy"), out], check=True, timeout=120, env=env)
        outs.append(dict(np.load(out)))
    for other in outs[1:]:
        for k in outs[0]:
            assert outs[0][k].tobytes() == other[k].tobytes(), k
    use = (np.arange(200) % 7 != 3).tolist()
    cand = (np.arange(130) % 3 != 1).tolist()
    want = _want(cell, use, cand, 0.6)
    got = outs[0]
    assert got["ident"].tolist() == want["ident"] and got["aligned"].tolist() == want["aligned"] and got["res"].tolist() == want["res"]
    assert got["nearest"].tolist() == want["nearest"] and got["ni"].tolist() == want["nearest_ident"] and got["nd"].tolist() == want["nearest_den"]
    assert got["red"].tolist() == ar.red_bits(want["red"])
    assert got["w"].tobytes() == np.array(want["weights"], np.float64).tobytes()


def test_ties(ctx):
    from dafs_amd import capi
    # identical rows: every nearest is the smallest other index, every weight 1.0
    # (no N: an N matches nothing, not even an N).  64 rows: 1 / n is a binary fraction, so every step of the weights is exact
    rows = ["ACGU-ACGAU"] * 64
    got = ctx.alignment_identity(rows)
    assert got.nearest.tolist() == [1] + [0] * 63 and (got.pid_nearest == 1.0).all()
    assert ctx.alignment_weights(rows).tolist() == [1.0] * 64
    # 70 rows: 1 / 70 is rounded and the running sums of the definition round again, so the equal weights are 1 within a few
    # ulp, and to the bit what the restatement gives
    rows = ["ACGU-ACGAU"] * 70
    got = ctx.alignment_identity(rows)
    assert got.nearest.tolist() == [1] + [0] * 69 and (got.pid_nearest == 1.0).all()
    w = ctx.alignment_weights(rows)
    assert w.tobytes() == np.array(ar.weights(ar.cells(rows)), np.float64).tobytes() and len(set(w.tolist())) == 1 and abs(w[0] - 1.0) < 1e-14
    # two different fractions compete for row 0: 2/3 (row 1, three residues) against 3/5 (row 2): 2 * 5 > 3 * 3
    rows = ["ACGUA", "AC--C", "ACGCC", "UUUUU"]
    got = ctx.alignment_identity(rows, matrix=True)
    assert (got.ident[0, 1], got.res[1], got.ident[0, 2], got.res[2]) == (2, 3, 3, 5)
    assert got.nearest[0] == 1 and (got.nearest_ident[0], got.nearest_den[0]) == (2, 3)
    _check(got, None, _want(capi.encode_cells(rows)))
    # equal fractions with different counts, 2/4 = 1/2: the smaller index wins, whichever it is
    rows = ["ACGU", "ACAA", "A-C-", "GGGG"]
    got = ctx.alignment_identity(rows, cand=[0, 1, 1, 0])
    assert got.nearest[0] == 1 and (got.nearest_ident[0], got.nearest_den[0]) == (2, 4)
    got = ctx.alignment_identity([rows[0], rows[2], rows[1], rows[3]], cand=[0, 1, 1, 0])
    assert got.nearest[0] == 1 and (got.nearest_ident[0], got.nearest_den[0]) == (1, 2)


def test_masks(ctx):
    from dafs_amd import capi
    cell = _random_cells(20, 40, seed=3)
    cell[4, 1::2] = 5  # row 4 has its residues in the even columns only
    cell[4, 0] = 2
    every_other = np.arange(40) % 2 == 1
    with pytest.raises(capi.DafsHipError):  # none of row 4's residues is used
        ctx.alignment_identity(cell, use=every_other)
    with pytest.raises(capi.DafsHipError):
        ctx.alignment_weights(cell, use=every_other)
    for use in (np.ones(40, bool), ~every_other):
        _check(ctx.alignment_identity(cell, use=use, matrix=True, nr=0.5), ctx.alignment_weights(cell, use=use), _want(cell, use.tolist(), None, 0.5))
    _check(ctx.alignment_identity(cell, use=np.ones(40, bool)), None, _want(cell))
    single = np.zeros(20, bool)
    single[7] = True  # one candidate: everybody's nearest but its own
    got = ctx.alignment_identity(cell, cand=single)
    assert got.nearest.tolist() == [7] * 7 + [NONE] + [7] * 12 and np.isnan(got.pid_nearest[7])
    assert (got.nearest_ident[7], got.nearest_den[7]) == (0, 0)
    _check(got, None, _want(cell, None, single.tolist()))
    cand = np.arange(20) % 4 == 0
    _check(ctx.alignment_identity(cell, cand=cand), None, _want(cell, None, cand.tolist()))


def test_redundancy_at_the_threshold_and_the_subset(ctx):
    from dafs_amd import capi
    # row 1 sits on the threshold with row 0 (ident 3, den 4), row 2 one count below it (2 of 4)
    rows = ["ACGUACGU", "ACGA----", "ACAA----", "ACGUACGU", "ACGUACGA", "UUUUUUUU", "ACGUAC--", "GGGGGGGG", "UUUUUUUA", "ACGAUUUU"]
    got = ctx.alignment_identity(rows, nr=0.75, matrix=True)
    assert (got.ident[0, 1], min(got.res[0], got.res[1])) == (3, 4) and got.bit(0, 1) and got.bit(1, 0)
    assert (got.ident[0, 2], min(got.res[0], got.res[2])) == (2, 4) and not got.bit(0, 2) and not got.bit(2, 0)
    want = _want(capi.encode_cells(rows), t=0.75)
    _check(got, None, want)
    assert all(not got.bit(r, r) for r in range(len(rows)))
    rank = np.random.RandomState(5).permutation(len(rows))
    forced = np.zeros(len(rows), bool)
    forced[[0, 3]] = True  # identical rows, both forced
    kept, by = capi.nr_select(got.red, rank, forced)
    wk, wb = ar.nr_select(want["red"], [int(x) for x in rank], forced.tolist())
    assert kept.tolist() == wk and by.tolist() == wb
    assert kept[0] and kept[3] and 0 < kept.sum() < len(rows)
    for r in np.nonzero(~kept)[0]:
        assert kept[by[r]] and got.bit(r, by[r])
    # a larger one: the rows of a random alignment at a threshold where some fall
    cell = _random_cells(130, 65, seed=11, gaps=0.05, other=0.02)
    t = 0.65
    got = ctx.alignment_identity(cell, nr=t)
    want = _want(cell, t=t)
    rank = np.random.RandomState(6).permutation(130)
    forced = np.zeros(130, bool)
    forced[[2, 100]] = True
    kept, by = capi.nr_select(got.red, rank, forced)
    wk, wb = ar.nr_select(want["red"], [int(x) for x in rank], forced.tolist())
    assert kept.tolist() == wk and by.tolist() == wb and 0 < kept.sum() < 130


def test_refusals_leave_outputs_and_context(ctx):
    from dafs_amd import capi
    cell = _random_cells(12, 30, seed=41)
    good = ctx.alignment_identity(cell, nr=0.5, matrix=True)
    good_w = ctx.alignment_weights(cell)
    high = cell.copy()
    high[3, 3] = 6
    empty = cell.copy()
    empty[5] = 5
    for bad in (high, empty):
        with pytest.raises(capi.DafsHipError):
            ctx.alignment_identity(bad)
        with pytest.raises(capi.DafsHipError):
            ctx.alignment_weights(bad)
    for t in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ctx.alignment_identity(cell, nr=t)
    # the library itself: the outputs stay as they were
    marks = [np.full(12, 77, np.uint32) for _ in range(4)]
    mats = [np.full((12, 12), 77, np.uint32) for _ in range(2)]
    red = np.full((12, 1), 77, np.uint32)
    wt = np.full(12, 7.0)

    def call(n, length, data, t):
        return capi._alignment_identity(ctx._h, n, length, data.ctypes.data, None, None, t, marks[0].ctypes.data, mats[0].ctypes.data,
                                        mats[1].ctypes.data, marks[1].ctypes.data, marks[2].ctypes.data, marks[3].ctypes.data, red.ctypes.data)

    assert call(12, 30, high, 0.5) == -1 and call(12, 30, empty, 0.5) == -1
    for t in (-0.1, 1.5, float("nan")):
        assert call(12, 30, cell, t) == -1
    # sizes beyond the limits are refused from the sizes alone, before a cell is read
    assert call((1 << 20) + 1, 1, cell, 0.0) == -1 and call(1, (1 << 20) + 1, cell, 0.0) == -1 and call(0, 30, cell, 0.0) == -1
    assert capi._alignment_identity(ctx._h, 32769, 1, cell.ctypes.data, None, None, 0.0, None, mats[0].ctypes.data, None, None, None, None, None) == -1
    assert capi._alignment_identity(ctx._h, 65537, 1, cell.ctypes.data, None, None, 0.5, None, None, None, None, None, None, red.ctypes.data) == -1
    assert capi._alignment_weights(ctx._h, 12, 30, high.ctypes.data, None, wt.ctypes.data) == -1
    assert capi._alignment_weights(ctx._h, 12, 30, empty.ctypes.data, None, wt.ctypes.data) == -1
    assert all((m == 77).all() for m in marks + mats + [red]) and (wt == 7.0).all()
    # nr = 0: the bit matrix is not computed and not written
    assert call(12, 30, cell, 0.0) == 0 and (red == 77).all() and marks[0].tolist() == good.res.tolist()
    again = ctx.alignment_identity(cell, nr=0.5, matrix=True)
    for k in ("res", "ident", "aligned", "nearest", "nearest_ident", "nearest_den", "red"):
        assert getattr(again, k).tobytes() == getattr(good, k).tobytes(), k
    assert ctx.alignment_weights(cell).tobytes() == good_w.tobytes()
    assert set(k for k in _stage_names(ctx, cell)) >= {"k_ali_pack", "k_ali_pairs<matrix>", "k_ali_pairs<nearest>", "k_ali_pairs<red>",
                                                      "k_ali_nearest_counts", "k_ali_transpose", "k_ali_count", "k_ali_columns", "k_ali_row_weights"}


def _stage_names(ctx, cell):
    ctx.stage_timing(True)
    try:
        ctx.alignment_identity(cell, nr=0.5, matrix=True)
        ctx.alignment_weights(cell)
        return ctx.stage_report()
    finally:
        ctx.stage_timing(False)
