"""The cases of the node set-up tests are what they claim (node_setup_cases.py), without a GPU: the sources per row, the addends
per batch of 64 and where a batch splits, which rounds of the cooperative form exceed the staging area, that the order of
the sources shows in the sums, that the cut cells hit their bounds exactly -- and that orc_pipeline_node_setup is the start
of orc_pipeline_solve_node."""
import os

import numpy as np
import pytest

import dd_nodes_ref as R
import node_setup_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _which(side):
    return "p_x" if side == 0 else "p_y"


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("n", S.A_ROWS)
def test_a_sources_per_row(n, side):
    """n sources per row of the averaged folding matrix; from 63 rows on, two columns in which one row alone has a residue,
    that row strictly inside a batch of 64"""
    c = R.cached(S.case_a, n, side)
    per = S.addends_per_source(c, _which(side))
    assert per.shape[1] == n
    assert S.addends_per_source(c, "p_z").shape[1] == n
    mask = np.asarray(c.nodes[0][2 * side + 1])
    assert mask.shape[0] == n and mask.shape[1] == 32
    if n > 2:
        for col in (0, 1):
            rows = np.nonzero(mask[:, col])[0]
            assert len(rows) == 1, (col, rows)
            if n >= 63:
                assert 0 < rows[0] % 64 < 63 and rows[0] + 1 < n
                assert per[col, rows[0]] > 0 and per[col].sum() == per[col, rows[0]]  # every other source of this row is a gap
    if n >= 63:
        assert per.sum(axis=1).max() <= S.AVG_STAGE  # plain batches: the staging area is case C's


def _batch_totals(case):
    """[row of p_z, round of 256 sources, wavefront] -> addends of that batch of 64 sources"""
    per = S.addends_per_source(case, "p_z")
    rows, nsrc = per.shape
    rounds = -(-nsrc // 256)
    pad = np.zeros((rows, rounds * 256), np.int64)
    pad[:, :nsrc] = per
    return pad.reshape(rows, rounds, 4, 64).sum(axis=3)


@pytest.mark.parametrize("n1,n2,rounds,last", [(23, 23, 3, 17), (2, 256, 2, 256), (300, 2, 3, 88)])
def test_b_rounds_of_the_cooperative_form(n1, n2, rounds, last):
    c = R.cached(S.case_b, n1, n2)
    assert (n1, n2) in S.B_SHAPES and n1 * n2 >= 512              # nodes_open's rule for the cooperative form
    tot = _batch_totals(c)
    assert tot.shape[1] == rounds and n1 * n2 - 256 * (rounds - 1) == last
    assert tot.max() <= S.AVG_STAGE and tot.max() > 64           # every round is staged, and the batches are not trivial
    # the cell that the cut must clear: one addend, whose share is the cut-off itself
    i0, j0 = c.cut_cell
    hits = [v[(r == i0) & (k == j0)] for r, k, v in S.sources(c, "p_z")]
    hits = np.concatenate(hits)
    assert len(hits) == 1 and np.float32(hits[0] / np.float32(n1 * n2)) == S.CUT
    assert S.average(c, "p_z")[i0, j0] == 0


def test_c_split_counts_and_passes():
    c = R.cached(S.case_c_split)
    per = S.addends_per_source(c, "p_x")
    assert per.shape[1] == 64
    for col, counts in S.C_SPLIT_COUNTS.items():
        assert list(per[col]) == counts, col
        assert sum(counts) > S.AVG_STAGE and S.passes_of(counts) == S.C_SPLIT_PASSES[col], col
    run = np.cumsum(S.C_SPLIT_COUNTS[2])
    assert run[20] == S.AVG_STAGE and np.cumsum(S.C_SPLIT_COUNTS[3])[21] == S.AVG_STAGE + 1
    assert S.passes_of([1060]) == [(0, 1)] and S.passes_of([1024, 1]) == [(0, 1), (1, 2)] and S.passes_of([1023, 1, 1]) == [(0, 2), (2, 3)]


def test_c_rounds_exceed_the_stage_in_round_0_only():
    c = R.cached(S.case_c_rounds)
    assert np.asarray(c.nodes[0][3]).shape[1] >= 24
    tot = _batch_totals(c)
    over = (tot > S.AVG_STAGE).any(axis=2)      # [row, round]: the round goes the one-wavefront way
    both = over[:, 0] & ~over[:, 1] & ~over[:, 2]
    assert both.sum() >= 16, both.sum()         # inside one row of p_z, for most rows
    assert tot[both][:, 1:].max() > 64


def test_c_long_single_sources():
    c = R.cached(S.case_c_long)
    assert S.addends_per_source(c, "p_x")[0, 0] == 1060 and S.addends_per_source(c, "p_z")[0, 0] == 1060
    assert S.addends_per_source(c, "p_x").shape == (S.C_LONG, 1) and S.C_LONG > 513


ORDER_CASES = ([("A", (S.case_a, n, side), (_which(side), "p_z")) for n in S.A_ROWS if n >= 63 for side in (0, 1)]
               + [("B", (S.case_b, n1, n2), ("p_z",)) for n1, n2 in S.B_SHAPES]
               + [("C split", (S.case_c_split,), ("p_x",)), ("C rounds", (S.case_c_rounds,), ("p_z",))])


@pytest.mark.parametrize("name,make,matrices", ORDER_CASES, ids=["%s-%s" % (n, "-".join(str(a) for a in m[1:])) for n, m, _ in ORDER_CASES])
def test_the_order_of_the_sources_shows(oracle, name, make, matrices):
    """summed in float32 in the reference's order the restatement gives the oracle's bytes; in the reversed order at least one
    cell of every matrix the case is about differs -- three or more sources meet in a cell"""
    c = R.cached(*make)
    want = S.reference(oracle, c)[0]
    for m in matrices:
        assert S.most_addends_in_a_cell(c, m) >= 3, m
        assert S.first_matrix_difference(S.average(c, m), want[m]) is None, m
        assert S.first_matrix_difference(S.average(c, m, reverse=True), want[m]) is not None, m


@pytest.mark.parametrize("n", [1, 2])
def test_d_cells_hit_their_bounds(oracle, n):
    c = R.cached(S.case_d, n)
    low, high = S.cut_values(n)
    d = np.float32(n)
    for vals, _ in list(low.values()) + list(high.values()):
        assert len(vals) == n
    raw = lambda vals: np.float32(sum((np.float32(v / d) for v in vals), np.float32(0)))
    assert raw(low["at the cut-off"][0]) == S.CUT
    assert raw(low["one ulp above it"][0]) == np.nextafter(S.CUT, np.float32(1)) and raw(low["one ulp below it"][0]) == np.nextafter(S.CUT, np.float32(0))
    one = np.float32(1)
    assert raw(high["above one"][0]) > one and raw(high["at one"][0]) == one
    assert raw(high["one ulp above one"][0]) == np.nextafter(one, np.float32(2)) and raw(high["one ulp below one"][0]) == np.nextafter(one, np.float32(0))
    want = S.reference(oracle, c)[0]
    for m, cells in c.cells.items():
        mine = S.average(c, m)
        for name, i, j, v in cells:
            assert mine[i, j].tobytes() == np.float32(v).tobytes(), (m, name)
            assert want[m][i, j].tobytes() == np.float32(v).tobytes(), (m, name)
    assert len(c.cells["p_x"]) == 3 and len(c.cells["p_z"]) == 7


SOLVED = [(R.shape_case, 63, 63), (R.shape_case, 63, 65), (R.shape_case, 1, 65), (R.supplied_case, 90, 130), (S.case_e_hand, 65), (S.case_d, 2),
          (R.multirow_case, 5, 100, 120)]


@pytest.mark.parametrize("make", SOLVED, ids=["-".join([m[0].__name__] + [str(a) for a in m[1:]]) for m in SOLVED])
def test_node_setup_is_the_start_of_solve_node(oracle, make):
    """the same consensus-pair count as orc_pipeline_solve_node, the supplied matrices handed through, the envelope of p_z,
    and pairs that pass the reference's conditions in its order"""
    c = R.cached(*make)
    st = S.reference(oracle, c)[0]
    assert len(st["cbp"]) == R.reference(oracle, c)[0]["ncbp"]
    node = c.nodes[0]
    if len(node) > 4:
        assert st["p_x"].tobytes() == np.asarray(node[4], np.float32).tobytes() and st["p_y"].tobytes() == np.asarray(node[5], np.float32).tobytes()
    elif c.w_pct == 0.0:
        for m in S.MATRICES:
            assert S.first_matrix_difference(S.average(c, m), st[m]) is None, m
    assert np.array_equal(st["env"], oracle.nw_envelope(st["p_z"], R.TH_A))
    cbp = st["cbp"].astype(np.int64)
    if len(cbp):
        i, j, k, l = cbp.T
        assert (j > i).all() and (l > k).all()
        assert (st["p_x"][i, j] > S.CUT).all() and (st["p_y"][k, l] > S.CUT).all() and (st["p_z"][i, k] > S.CUT).all() and (st["p_z"][j, l] > S.CUT).all()
        key = ((i * (1 << 16) + j) * (1 << 16) + k) * (1 << 16) + l
        assert (np.diff(key) > 0).all()                           # (i, j, k, l) ascending: dafs.cpp:1022-1044
    if make[0] is S.case_e_hand:
        assert len(cbp) > 0


def test_e_hand_made_matrices_have_their_edges():
    for L in S.E_HAND:
        node = R.cached(S.case_e_hand, L).nodes[0]
        for p in (node[4], node[5]):
            keep = np.triu(p > S.CUT, 1)
            assert not keep[0].any() and not keep[20].any() and not keep[L - 1].any()      # empty rows
            assert any(keep[i, i + 1:].all() for i in range(L - 1))                        # a row kept whole
            assert keep[:, L - 1].any() and keep[L - 2, L - 1]                             # the last column
            assert np.diagonal(keep, 1).sum() >= 2                                         # j = i + 1
            assert (p == S.CUT).any()
        rp, col, val = R.cached(S.case_e_hand, L).mp[(0, 1)]
        n = np.diff(rp.astype(np.int64))
        assert (n == 0).any() and (n == L).any() and (col == L - 1).any() and (val == S.CUT).any()


def test_the_header_declares_and_the_library_exports_node_peek():
    import ctypes
    from dafs_amd import capi
    with open(os.path.join(ROOT, "include", "dafs_hip.h")) as f:
        header = f.read()
    assert "int dafs_hip_node_peek(dafs_hip_ctx* ctx, uint32_t handle, int what, void* dst, uint64_t capacity_bytes, uint64_t* bytes_out);" in header
    names = [w.strip() for w in header.split("DAFS_PEEK_P_X = 0,")[1].split("}")[0].replace("\n", " ").split(",")]
    assert ["p_x"] + [n[len("DAFS_PEEK_"):].lower() for n in names] == list(capi.NODE_PEEK)
    assert isinstance(getattr(capi.lib, "dafs_hip_node_peek"), ctypes._CFuncPtr)
    out = ctypes.c_uint64(77)
    assert capi.lib.dafs_hip_node_peek(None, 0, 0, None, 0, ctypes.byref(out)) == -1 and out.value == 77   # no context: refused before any HIP call
