"""What a node's set-up kernels write (dd.hip: k_node_avg, k_node_lists or k_lists_rows / k_lists_scan / k_node_lists_tail,
k_node_cbp_fill), fetched from the open node with Context.node_peek, against orc_pipeline_node_setup on the same hand-made
stores.  For every case and form of node_setup_cases.py: open, peek, close, compare --

- p_x, p_y, p_z by their bytes against the oracle's matrices;
- the x, y and z lists: per row the ascending columns whose oracle value is above the cut-off (x, y: j > i only), and the
  dense maps that invert them, -1 elsewhere;
- env against the oracle's nw_envelope of p_z; env4 (written by the node's first iteration, not by the set-up) as dd.h
  defines it from env, in the test that iterates;
- cbp: (i, j, k, l) in the oracle's order, its entry and cell ids consistent with the peeked maps, the cz lists the sorted
  distinct cells (i, k) and (j, l) with their map, cbp_cnt the count per x entry.

A failure names the case, the form, the array and the first cell, matrices with both values in hex.  Every variant is
compared with the oracle, never with another variant.

Without a definition on the oracle's side: cbp_cnt as peeked is the running total of the per-entry counts wherever the node
has a consensus pair (k_node_cbp_fill scans it in place), the plain counts (all zero) otherwise -- the test derives both from
the oracle's pairs; the flag arrays (cflag, cz_flag), the first / last columns that the envelope kernels leave in x and z as
scratch, and the zero / -1 fills of the multipliers and counters are not peeked.

Left out: the averaging launch with two rows per workgroup, which needs more than 7936 columns."""
import ctypes

import numpy as np
import pytest

import dd_nodes_ref as R
import node_setup_cases as S

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in R.ALL_SWITCHES:
        monkeypatch.delenv("DAFS_HIP_DD_" + name, raising=False)
    for name in S.SETUP_SWITCHES:
        monkeypatch.delenv(name, raising=False)


def _form(monkeypatch, form):
    if form:
        monkeypatch.setenv(*form.split("="))
    return form or "default switches"


def _compare(oracle, cases, form, copies=1, **kw):
    got = S.open_and_peek(cases, copies, **kw)
    for c, per_copy in zip(cases, got):
        want = S.reference(oracle, c)[0]
        for k, peek in enumerate(per_copy):
            d = S.setup_difference(peek, want)
            assert d is None, "case %r, %s%s, %d x %d columns: %s" % (c.key, form, ", copy %d of %d in one open call" % (k, copies) if copies > 1 else "",
                                                                      want["p_z"].shape[0], want["p_z"].shape[1], d)


@pytest.mark.parametrize("form", [None, "DAFS_HIP_DD_WIDE=1"], ids=["default", "wide"])
@pytest.mark.parametrize("side", [0, 1], ids=["p_x", "p_y"])
@pytest.mark.parametrize("n", S.A_ROWS)
def test_a_sources_per_row(oracle, monkeypatch, n, side, form):
    """1, 2, 63, 64, 65 and 130 gapped rows in one child: avg_row deals the sources to the lanes 64 at a time, gaps inside a
    batch; four averaging rows per workgroup, and one (DAFS_HIP_DD_WIDE)"""
    _compare(oracle, [R.cached(S.case_a, n, side)], _form(monkeypatch, form))


B_VARIANTS = {"cooperative": (None, 1), "per-wavefront": ("DAFS_HIP_AVG_COOP0=1", 1), "five-nodes": (None, 5)}


@pytest.mark.parametrize("variant", list(B_VARIANTS))
@pytest.mark.parametrize("n1,n2", S.B_SHAPES, ids=["%dx%d" % s for s in S.B_SHAPES])
def test_b_cooperative_form(oracle, monkeypatch, n1, n2, variant):
    """n1 * n2 >= 512 sources per row of p_z: a workgroup per row with four staged batches a round; the per-wavefront form at
    four rows per workgroup by the switch; and by nodes_open's rule, five such nodes in one call"""
    form, copies = B_VARIANTS[variant]
    _compare(oracle, [R.cached(S.case_b, n1, n2)], _form(monkeypatch, form), copies)


def test_c_batch_splits(oracle):
    """64 sources whose addends pass the staging area: the batch splits after lane 0, before lane 63, and where the running
    total is exactly 1024 or one more (columns 0 .. 3 of p_x)"""
    _compare(oracle, [R.cached(S.case_c_split)], "default switches")


@pytest.mark.parametrize("form", [None, "DAFS_HIP_AVG_COOP0=1"], ids=["cooperative", "per-wavefront"])
def test_c_rounds_beyond_the_stage(oracle, monkeypatch, form):
    """(23, 23) with dense first sources: round 0 of a row of p_z goes the one-wavefront way, rounds 1 and 2 are staged"""
    _compare(oracle, [R.cached(S.case_c_rounds)], _form(monkeypatch, form))


@pytest.mark.parametrize("form", [None, "DAFS_HIP_DD_LISTS_WIDE=1"], ids=["default", "lists_wide"])
def test_c_one_source_beyond_the_stage(oracle, monkeypatch, form):
    """1100 columns, rows of about 1060 entries: the source that alone exceeds the staging area, for p_x and for p_z; row counts
    scanned beyond 512 rows.  Opened and peeked, never iterated."""
    _compare(oracle, [R.cached(S.case_c_long)], _form(monkeypatch, form))


@pytest.mark.parametrize("form", [None, "DAFS_HIP_DD_WIDE=1"], ids=["default", "wide"])
@pytest.mark.parametrize("n", [1, 2])
def test_d_cuts(oracle, monkeypatch, n, form):
    """sums at the cut-off become 0 and sums above 1 become 1 (p_z), one ulp to either side of both bounds they do not"""
    c = R.cached(S.case_d, n)
    name = _form(monkeypatch, form)
    _compare(oracle, [c], name)
    peek = S.open_and_peek([c])[0][0]
    for m, cells in c.cells.items():
        for what, i, j, v in cells:
            assert peek[m][i, j].tobytes() == np.float32(v).tobytes(), "case %r, %s, %s cell (%d, %d) %s: 0x%08x, expected 0x%08x" % (
                c.key, name, m, i, j, what, peek[m][i:i + 1, j].view(np.uint32)[0], np.float32(v).view(np.uint32))


@pytest.mark.parametrize("form", list(S.E_FORMS))
@pytest.mark.parametrize("L1,L2", S.E_SHAPES, ids=["%dx%d" % s for s in S.E_SHAPES])
def test_e_every_shape_of_the_table(oracle, monkeypatch, L1, L2, form):
    """single-row shapes from 1 to 1025 columns (63 / 64 / 65, 255 / 256 / 257, 511 / 513 rows and beyond): the lists, maps,
    envelope and consensus pairs in every form of the list kernels"""
    _compare(oracle, [R.cached(R.shape_case, L1, L2)], _form(monkeypatch, S.E_FORMS[form]))


@pytest.mark.parametrize("form", list(S.E_FORMS))
@pytest.mark.parametrize("L", S.E_HAND)
def test_e_hand_made_matrices(oracle, monkeypatch, L, form):
    """empty rows, rows kept whole, kept cells in the last column and at j = i + 1, cells at the cut-off"""
    _compare(oracle, [R.cached(S.case_e_hand, L)], _form(monkeypatch, S.E_FORMS[form]))


def test_e_seventeen_nodes_in_one_call(oracle):
    """more than 16 nodes in one open call: one workgroup per node by dd_lists_launch's rule"""
    shapes = [s for s in R.TABLE if max(s) <= 257] + list(S.E_HAND)
    cases = [R.cached(R.shape_case, *s) if isinstance(s, tuple) else R.cached(S.case_e_hand, s) for s in shapes]
    copies = -(-17 // len(cases))
    assert len(cases) * copies >= 17
    _compare(oracle, cases, "%d nodes in one open call" % (len(cases) * copies), copies)


def test_peeking_disturbs_nothing(oracle):
    """open, peek everything, advance to the end: the result is the one solve_nodes gives, and the oracle's; env4 as dd.h
    defines it from env once the first iteration has written it"""
    case = R.cached(R.shape_case, 63, 65)
    want = R.reference(oracle, case)[0]
    ctx, nodes = R.open_context([case])
    prm = R.device_params(case)
    try:
        plain = ctx.solve_nodes(nodes[0], prm)[0]
        (h,), ((L1, L2),) = ctx.nodes_open(nodes[0], prm)
        before = S.peek_all(ctx, h)
        assert ctx.nodes_advance([h], prm, 0).all()
        after = S.peek_all(ctx, h, ("p_x", "p_y", "p_z", "env", "env4", "x_col", "y_col", "pz_k", "cbp"))
        got = ctx.nodes_result(h, L1, L2)
        ctx.nodes_close()
    finally:
        ctx.close()
    assert S.setup_difference(before, S.reference(oracle, case)[0]) is None
    for a in ("p_x", "p_y", "p_z", "env", "x_col", "y_col", "pz_k", "cbp"):
        assert np.array_equal(before[a], after[a]), a
    assert np.array_equal(after["env4"], S.env4_of(before["env"], L1))
    R.assert_node(got, want, case, "opened, peeked, advanced")
    R.assert_node(got, plain, case, "opened, peeked, advanced, against solve_nodes")


def test_a_node_that_a_round_opened(oracle):
    """nodes_round sets a new node up on the second stream while an open one advances: the new node's arrays after its first
    iteration, both nodes' results at the end"""
    first, a = R.cached(R.shape_case, 63, 63), R.cached(S.case_a, 65, 0)
    second = R.Case(a.key + ("iterated",), a.seqs, a.bp, a.mp, a.nodes, first.t_max)   # one iteration cap for the whole call
    ctx, nodes = R.open_context([first, second])
    prm = R.device_params(first)
    try:
        (h0,), (dims0,) = ctx.nodes_open(nodes[0], prm)
        (h1,), (dims1,), fin0, fin1 = ctx.nodes_round(nodes[1], [h0], prm, 1)
        peek = S.peek_all(ctx, h1)
        while not (fin0.all() and fin1.all()):
            _, _, fin0, fin1 = ctx.nodes_round([], [h0, h1], prm, 50)
            fin0, fin1 = fin0[:1], fin0[1:]
        got = [ctx.nodes_result(h0, *dims0), ctx.nodes_result(h1, *dims1)]
        ctx.nodes_close()
    finally:
        ctx.close()
    d = S.setup_difference(peek, S.reference(oracle, second)[0])
    assert d is None, "case %r, opened by nodes_round beside a running node: %s" % (second.key, d)
    R.assert_node(got[0], R.reference(oracle, first)[0], first, "advanced while a round opened another node")
    R.assert_node(got[1], R.reference(oracle, second)[0], second, "opened by nodes_round, peeked after one iteration")


def test_refusals_leave_outputs_and_context_alone(oracle):
    from dafs_amd import capi
    coupled, uncoupled = R.cached(R.shape_case, 63, 63), R.cached(R.shape_case, 1, 65)
    assert R.reference(oracle, uncoupled)[0]["ncbp"] == 0
    ctx, nodes = R.open_context([coupled, uncoupled])
    prm = R.device_params(coupled)
    try:
        (h,), _ = ctx.nodes_open(nodes[0], prm)
        (hu,), _ = ctx.nodes_open(nodes[1], R.device_params(uncoupled, skip_uncoupled_folds=1))
        (hd,), ((L1, L2),) = ctx.nodes_open(nodes[0], prm)
        assert ctx.nodes_advance([hd], prm, 0).all()
        ctx.nodes_result(hd, L1, L2)   # its memory has gone back

        def refused(handle, what, capacity):
            buf = np.full(64 * 64 + 400, 0x5A5A5A5A, np.uint32)
            n = ctypes.c_uint64(77)
            rc = capi._node_peek(ctx._h, handle, what, buf.ctypes.data, capacity, ctypes.byref(n))
            return rc == -1 and n.value == 77 and (buf == 0x5A5A5A5A).all()
        P = capi.NODE_PEEK.index
        assert refused(99, P("p_x"), 1 << 20), "unknown handle"
        assert refused(hd, P("p_x"), 1 << 20), "a node whose memory nodes_result gave back"
        assert refused(h, len(capi.NODE_PEEK), 1 << 20) and refused(h, -1, 1 << 20), "unknown array"
        assert refused(h, P("p_x"), 63 * 63 * 4 - 1) and refused(h, P("x_col"), 0) and refused(h, P("env"), 4), "buffer too small"
        assert refused(hu, P("cbp"), 1 << 20), "cbp of a node opened without its folding arrays"
        with pytest.raises(capi.DafsHipError):
            ctx.node_peek(h, "q_x")
        with pytest.raises(capi.DafsHipError):
            ctx.node_peek(99, "p_x")
        # the context goes on: both nodes are what the oracle says, and the first one solves
        assert S.setup_difference(S.peek_all(ctx, h), S.reference(oracle, coupled)[0]) is None
        want_u = S.reference(oracle, uncoupled)[0]
        assert S.first_matrix_difference(ctx.node_peek(hu, "p_z"), want_u["p_z"]) is None and np.array_equal(ctx.node_peek(hu, "env"), want_u["env"])
        assert ctx.nodes_advance([h], prm, 0).all()
        R.assert_node(ctx.nodes_result(h, L1, L2), R.reference(oracle, coupled)[0], coupled, "after refused peeks")
        ctx.nodes_close()
    finally:
        ctx.close()
