"""The fused node solver (dd.hip, capi_dd.cpp) node by node against the oracle, at every plan: Context.solve_nodes and the
resident-node rounds against orc_pipeline_solve_node on the same supplied stores.  Every output is compared -- x, y, z as
arrays, the score by its bytes, ncbp, iterations, violated -- and a failure names the node, its plan class and the first
output that differs.  Shapes, inputs and the comparison live in dd_nodes_ref.py; test_dd_nodes_cpu.py checks, without a
GPU, that the shapes reach every plan class and that the inputs keep the solver busy and meet ties."""
import numpy as np
import pytest

import dd_nodes_ref as R

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF


@pytest.fixture(autouse=True)
def default_switches(monkeypatch):
    for name in R.ALL_SWITCHES:
        monkeypatch.delenv("DAFS_HIP_DD_" + name, raising=False)


def _check(oracle, case, what="", **kw):
    want = R.reference(oracle, case)
    got = R.solve_on_device(case, **kw)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        R.assert_node(g, w, case, what)
    return got


@pytest.mark.parametrize("L1,L2", R.TABLE, ids=["%dx%d" % s for s in R.TABLE])
def test_every_shape_of_the_table(oracle, L1, L2):
    """single-row children, continuous values: every (lds_flags, fold_fast) class of the planner up to 1025 columns, both
    orientations of the asymmetric ones, and the shapes with a side of one or two columns"""
    _check(oracle, R.cached(R.shape_case, L1, L2))


@pytest.mark.parametrize("switch", R.SWITCHES, ids=[s or "default" for s in R.SWITCHES])
@pytest.mark.parametrize("family", list(R.FAMILIES), ids=[f.replace(" ", "_") for f in R.FAMILIES])
def test_quantised_values_in_every_form(oracle, monkeypatch, family, switch):
    """base-pairing values from {0.25, 0.5, 0.75, 1} and matching values from multiples of 1/8, so that the DPs inside the
    solver meet ties (asserted in test_dd_nodes_cpu.py): one shape per form family, under the default plan and under each
    switch that moves it to another form.  Every variant against the oracle, not against the others."""
    if switch:
        monkeypatch.setenv(*switch.split("="))
    _check(oracle, R.cached(R.shape_case, *R.FAMILIES[family], True), "quantised, %s, %s" % (family, switch or "default switches"))


@pytest.mark.parametrize("L1,L2", R.MULTIROW_SHAPES, ids=["%dx%d" % s for s in R.MULTIROW_SHAPES])
@pytest.mark.parametrize("nseq", [5, 9])
def test_multi_row_children_with_gaps(oracle, nseq, L1, L2):
    """children of 2 to 5 gapped rows on stores relaxed by both consistency transforms: the averaging kernel's weights and
    row maps, and the N1 / N2 factors of the folding scores and the consensus pairs"""
    _check(oracle, R.cached(R.multirow_case, nseq, L1, L2))


@pytest.mark.parametrize("L1,L2", R.SUPPLIED_SHAPES, ids=["%dx%d" % s for s in R.SUPPLIED_SHAPES])
def test_supplied_base_pairing_matrices(oracle, L1, L2):
    """dafs_node_input.p_x / p_y (the --bp-update input) in place of the averages: dense-ish quantised matrices"""
    _check(oracle, R.cached(R.supplied_case, L1, L2))


BATCH_T_MAX = 25


def _batch(oracle):
    shapes = [s for s in R.TABLE if max(s) <= 256]
    cases = [R.cached(R.shape_case, L1, L2, False, BATCH_T_MAX) for L1, L2 in shapes]
    return cases, [R.reference(oracle, c)[0] for c in cases]


def test_one_call_for_many_nodes(oracle):
    """every table shape of at most 256 columns in one solve_nodes call: each node's result is the one it has alone, and the
    oracle's"""
    cases, want = _batch(oracle)
    assert len(cases) >= 10
    ctx, nodes = R.open_context(cases)
    prm = R.device_params(cases[0])
    try:
        together = ctx.solve_nodes([n[0] for n in nodes], prm)
        alone = [ctx.solve_nodes(n, prm)[0] for n in nodes]
    finally:
        ctx.close()
    for c, t, a, w in zip(cases, together, alone, want):
        R.assert_node(a, w, c, "alone in a context of %d sequences" % (2 * len(cases)))
        R.assert_node(t, w, c, "in a call of %d nodes" % len(cases))


@pytest.mark.parametrize("slice_iters", [1, 7])
def test_resident_rounds_for_many_nodes(oracle, slice_iters):
    """the same nodes through nodes_round, half of them opened beside the other half already running, slice_iters iterations
    per round: the oracle's results however the iterations are cut"""
    from dafs_amd import pipeline
    cases, want = _batch(oracle)
    ctx, nodes = R.open_context(cases)
    waves = [[(k, nodes[k][0]) for k in range(0, len(cases), 2)], [(k, nodes[k][0]) for k in range(1, len(cases), 2)]]
    got = {}
    try:
        pipeline._solve_nodes(ctx, R.device_params(cases[0]), lambda: waves.pop(0) if waves else [], lambda k, o, dims: got.__setitem__(k, o),
                              slice_iters=slice_iters)
    finally:
        ctx.close()
    assert sorted(got) == list(range(len(cases)))
    for k, (c, w) in enumerate(zip(cases, want)):
        R.assert_node(got[k], w, c, "resident, %d iterations a round" % slice_iters)


def test_skip_uncoupled_folds(oracle):
    """dafs_dd_params.skip_uncoupled_folds: a node without consensus pairs (here: a side of one column) returns the oracle's
    alignment and no structure; a coupled node is untouched in every output"""
    for L1, L2 in [s for s in R.TABLE if min(s) == 1]:
        case = R.cached(R.shape_case, L1, L2)
        want = R.reference(oracle, case)[0]
        assert want["ncbp"] == 0
        got = R.solve_on_device(case, skip_uncoupled_folds=1)[0]
        R.assert_node(got, want, case, "skip_uncoupled_folds=1", outputs=("z", "ncbp"))
        assert np.all(got["x"] == NONE) and np.all(got["y"] == NONE), case.key
        assert got["iterations"] <= want["iterations"], case.key
    _check(oracle, R.cached(R.shape_case, 63, 63), "skip_uncoupled_folds=1", skip_uncoupled_folds=1)
    _check(oracle, R.cached(R.shape_case, 63, 63, True), "quantised, skip_uncoupled_folds=1", skip_uncoupled_folds=1)


def test_seed_scores_are_the_oracles_node(oracle):
    """pipeline.add (`dafs --seed`; the score and iteration columns of --seed-scores are this node's): every new sequence's node
    -- its leaf against the gapped seed rows, on a phase 1 of ProbCons + CONTRAfold and both transforms over seed and new
    sequences together -- against orc_pipeline_solve_node on the oracle's phase 1 of the same sequences"""
    import os
    from dafs_amd import pipeline, synth
    recs = oracle.fasta(os.path.join(os.path.dirname(__file__), "golden", "RF00005_0.fa"))
    seed = pipeline.run([n for n, _ in recs[:3]], [s for _, s in recs[:3]])
    seed_names, seed_rows = [n for n, _ in recs[:3]], list(seed.rows)
    assert any("-" in r for r in seed_rows)
    new = [recs[3], ("short", synth.random_set(1, 31, seed=5)[0][1])]     # a tRNA, and a short sequence against the long seed
    names, seqs = [n for n, _ in new], [s for _, s in new]
    got = pipeline.add(seed_names, seed_rows, names, seqs, skip_uncoupled_folds=False)
    m = len(seed_rows)
    seed_seqs = [r.replace("-", "") for r in seed_rows]
    seed_mask = np.array([[ch != "-" for ch in r] for r in seed_rows], np.uint8)
    pl = oracle.pipeline(seed_names + names, seed_seqs + seqs, oracle.params())
    pl.phase1()
    coupled = 0
    for j, s in enumerate(seqs):
        want = pl.solve_node(np.array([m + j], np.uint32), np.ones((1, len(s)), np.uint8), np.arange(m, dtype=np.uint32), seed_mask)
        its, viol, ncbp, score = got.dd_log[j]
        mine = dict(z=got.z[j], score=np.float32(score), ncbp=ncbp, iterations=its, violated=viol)
        d = R.first_difference(mine, want, outputs=("z", "score", "ncbp", "iterations", "violated"))
        assert d is None, "new sequence %d (%d residues) against the seed of %d rows x %d columns: %s" % (j, len(s), m, seed_mask.shape[1], d)
        coupled += ncbp > 0
    pl.close()
    assert coupled >= 1
