"""GPU tests of the structural pair score: k_struct_sim and k_struct_w against the numpy restatement
(structure_sim_ref.py) as integers, on hand-made stores and on the stores the device makes; Context.similarity with
score="structure" and "mix" under every range budget; pipeline.cluster and `dafs --cluster-score`.  Every case is seconds."""
import os
import subprocess

import numpy as np
import pytest

import cluster_ref
import structure_sim_ref as ref
from linkage_ref import linkage_ref
from dafs_amd import capi, pipeline, synth
from test_cluster_structure_cpu import csr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NAN = float("nan")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _install(ctx, seqs, mps, bps):
    """hand-made stores through set_mp / set_bp: mps[(x, y)] and bps[x] as CSR triples"""
    n = len(seqs)
    pairs = [(x, y) for x in range(n) for y in range(x + 1, n)]
    ctx.set_sequences(seqs)
    ctx.set_mp([len(mps[p][1]) for p in pairs], np.concatenate([mps[p][0] for p in pairs]),
               np.concatenate([mps[p][1] for p in pairs]), np.concatenate([mps[p][2] for p in pairs]))
    ctx.set_bp(bps)
    return pairs


def _scores_without_lds(ctx):
    """structure_scores() with the kernel's LDS copies switched off, and with room for some of the arrays only"""
    out = []
    for knob, value in (("DAFS_HIP_STRUCT_LDS", "0"), ("DAFS_HIP_STRUCT_LDS_WORDS", "300")):
        os.environ[knob] = value
        try:
            out.append(ctx.structure_scores())
        finally:
            del os.environ[knob]
    return out


def _check_against_restatement(ctx, seqs, mps, bps):
    pairs = _install(ctx, seqs, mps, bps)
    T, terms, W = ctx.structure_scores()
    assert T.dtype == terms.dtype == W.dtype == np.uint64
    for other in _scores_without_lds(ctx):  # where the kernel reads its rows changes nothing
        assert all(a.tobytes() == b.tobytes() for a, b in zip(other, (T, terms, W)))
    want = [ref.pair_terms(mps[p], bps[p[0]], bps[p[1]]) for p in pairs]
    assert [int(t) for t in T] == [w[0] for w in want]
    assert [int(t) for t in terms] == [w[1] for w in want]
    assert [int(w) for w in W] == [ref.weight(b) for b in bps]
    return dict(zip(pairs, want)), [int(w) for w in W]


def test_known_answers_on_hand_made_stores(ctx):
    seqs = ["ACGUAC", "GGGAAA"]
    empty = csr(6, {})
    got, W = _check_against_restatement(ctx, seqs, {(0, 1): csr(6, {0: [(0, 0.5)], 5: [(5, 0.25)]})}, [csr(6, {0: [(5, 0.5)]}), csr(6, {0: [(5, 0.75)]})])
    assert got[(0, 1)] == (51539607552, 1) and W == [549755813888, 824633720832]
    assert np.float32(capi.structure_score(got[(0, 1)][0], W[0], W[1])).tobytes() == np.float32(0.09375).tobytes()
    bx, by = csr(6, {0: [(5, 0.5)], 1: [(4, 0.3)]}), csr(6, {0: [(5, 0.75)], 1: [(4, 0.7)]})
    got, W = _check_against_restatement(ctx, seqs, {(0, 1): csr(6, {0: [(0, 0.5)], 1: [(1, 0.9)], 4: [(4, 0.6)], 5: [(5, 0.25)]})}, [bx, by])
    assert got[(0, 1)] == (176224230624, 2) and W == [879609315328, 1594291847168]
    assert int(np.float32(capi.structure_score(got[(0, 1)][0], W[0], W[1])).view(np.uint32)) == 1045243626
    # rows 0 and 5 with their columns swapped: k = 5 > l = 0
    got, _ = _check_against_restatement(ctx, seqs, {(0, 1): csr(6, {0: [(5, 0.5)], 1: [(1, 0.9)], 4: [(4, 0.6)], 5: [(0, 0.25)]})}, [bx, by])
    assert got[(0, 1)] == (124684623072, 1)
    # a store without an entry, and sequences without a base pair
    got, W = _check_against_restatement(ctx, seqs, {(0, 1): empty}, [bx, empty])
    assert got[(0, 1)] == (0, 0) and W[1] == 0
    assert capi.structure_score(0, W[0], W[1]) == 0.0


def test_edge_shapes_on_hand_made_stores(ctx):
    """x of 12, y of 80 and z of 6 residues: rows wider than a wavefront on both sides of the search, rows of one and two entries
    hit at both ends and missed on both sides, k = l and k > l, empty rows, the clamp at both ends and NaN, and a sequence
    without a base pair"""
    seqs = ["ACGUACGUACGU", "ACGU" * 20, "GGGAAA"]
    bx = csr(12, {0: [(11, 0.5)], 1: [(10, 0.3)], 2: [(9, 1.5)], 3: [(8, -0.25)], 4: [(7, NAN)], 5: [(6, 0.4)]})
    by = csr(80, {0: [(l, 0.01 * (l % 7 + 1)) for l in range(1, 66)],  # 65 entries
                  1: [(40, 0.7)], 2: [(30, 0.2), (50, NAN)], 4: [(5, 0.5)], 5: [(6, 0.5)], 70: [(79, 1.0)]})
    bz = csr(6, {})
    mxy = csr(12, {0: [(k, 0.005 * (k % 5 + 1)) for k in range(70)],          # 70 entries: k = 0, 1 and 2 lead into rows of bp[y]
                   11: [(l, 0.004 * (l % 9 + 1)) for l in range(1, 71)],      # 70 entries
                   1: [(1, 0.9)], 10: [(39, 0.1), (40, 0.6), (41, 0.1)],      # a row of one entry: missed below, hit, missed above
                   2: [(2, 1.5)], 9: [(29, 0.1), (30, 0.2), (50, 0.3), (51, 0.4)],  # a row of two entries: both ends, and past them
                   3: [(5, 0.5)], 8: [(4, 0.5), (5, 0.5), (6, 0.5)],          # k > l, k = l, and a hit under p = -0.25
                   4: [(2, 0.5)], 7: [(30, 0.5)],                             # a hit under p = NaN
                   6: [(3, 1.5)]})                                            # row 5 is empty: the pair (5, 6) of x meets nothing
    mxz = csr(12, {0: [(0, 0.5)], 11: [(5, 0.5)]})
    myz = csr(80, {0: [(0, 0.5)], 65: [(5, 0.5)], 79: [(5, 0.25)]})
    got, W = _check_against_restatement(ctx, seqs, {(0, 1): mxy, (0, 2): mxz, (1, 2): myz}, [bx, by, bz])
    T, terms = got[(0, 1)]
    # the pair (0, 11) of x meets rows 0, 1, 2, 4 and 5 of bp[y]; then (1, 10), (2, 9), (3, 8) and (4, 7)
    assert terms == (65 + 1 + 2 + 1 + 1) + 1 + 2 + 1 + 1 and T > 0
    assert got[(0, 2)] == (0, 0) and got[(1, 2)] == (0, 0) and W[2] == 0
    # the scored pass needs sequences the pair kernels take, not these stores; the formulas on the integers above
    assert capi.structure_score(T, W[0], W[1]) == ref.structure_score(T, W[0], W[1]) > 0.0


# ------------------------------------------------------------------------------------------------- stores the device makes
@pytest.fixture(scope="module")
def scored(ctx):
    """per alignment model, on the test set: the fetched rows of a full-pair-set align_posteriors and of fold_posteriors, the
    restatement's integers and matrices on them, and the sequence matrix of today's similarity()"""
    names, seqs, family = ref.test_set()
    n = len(seqs)
    out = {}
    for model in (capi.ALIGN_PROBCONS, capi.ALIGN_CONTRALIGN):
        ctx.set_sequences(seqs)
        ctx.fold_posteriors(0.01)
        res = ctx.align_posteriors(model, 0.01)
        bps = ctx.bp(0)
        got = ctx.structure_scores()
        for other in _scores_without_lds(ctx):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(other, got))
        mps = {(int(res.pair_x[p]), int(res.pair_y[p])): res.csr(p) for p in range(len(res))}
        T, terms, W, st, _ = ref.matrices(n, mps, bps)
        ctx.set_sequences(seqs)
        seq_sim, ranges = ctx.similarity(model, 0.01)
        out[model] = dict(pairs=list(mps), got=got, T=T, terms=terms, W=W, st=st, bps=bps, seq=seq_sim, ranges=ranges)
    return names, seqs, family, out


def _mix(seq, st, w):
    out = np.eye(len(seq), dtype=np.float32)
    for x in range(len(seq)):
        for y in range(len(seq)):
            if x != y:
                out[x, y] = ref.mix_score(seq[x, y], st[x, y], w)
    return out


@pytest.mark.parametrize("model", [capi.ALIGN_PROBCONS, capi.ALIGN_CONTRALIGN], ids=["probcons", "contralign"])
def test_device_made_stores_equal_the_restatement(scored, model):
    names, seqs, family, out = scored
    d = out[model]
    T, terms, W = d["got"]
    assert len(d["pairs"]) == 105 == len(T)
    assert [int(t) for t in T] == [d["T"][p] for p in d["pairs"]]
    assert [int(t) for t in terms] == [d["terms"][p] for p in d["pairs"]]
    assert [int(w) for w in W] == d["W"]
    # the inputs exercise the kernel: every family pair scores, the 3-nt sequence cannot
    tiny = names.index("r3")
    assert d["W"][tiny] == 0 and np.all(d["st"][tiny, np.arange(len(seqs)) != tiny] == 0.0)
    for x, y in d["pairs"]:
        if family[x] is not None and family[x] == family[y]:
            assert d["T"][(x, y)] > 0, (names[x], names[y])


def _budgets(seqs):
    lens = [len(s) for s in seqs]
    n = len(lens)
    total = sum(cluster_ref.pair_bytes(lens[x], lens[y]) for x in range(n) for y in range(x + 1, n))
    return [(None, 1), (total // 4, None), (1, n * (n - 1) // 2)]


@pytest.mark.parametrize("score,w", [("structure", None), ("mix", 0.5), ("mix", 0.25)], ids=["structure", "mix", "mix-quarter"])
def test_scored_similarity_in_ranges(ctx, scored, score, w):
    names, seqs, family, out = scored
    d = out[capi.ALIGN_PROBCONS]
    want = d["st"] if score == "structure" else _mix(d["seq"], d["st"], w)
    assert want.tobytes() == want.T.copy().tobytes()
    kw = {} if w is None or w == 0.5 else dict(structure_weight=w)  # 0.5 is the default weight
    for budget, n_ranges in _budgets(seqs):
        ctx.set_sequences(seqs)
        ctx.fold_posteriors(0.01)
        sim, got_ranges = ctx.similarity(capi.ALIGN_PROBCONS, 0.01, budget, score=score, **kw)
        assert sim.tobytes() == want.tobytes(), budget
        assert got_ranges == len(capi.similarity_ranges([len(s) for s in seqs], budget))
        assert got_ranges == n_ranges if n_ranges is not None else 4 <= got_ranges <= 6
        seq_sim, st = ctx.pair_scores()
        assert seq_sim.tobytes() == d["seq"].tobytes() and st.tobytes() == d["st"].tobytes()
        assert ctx.sim().tobytes() == want.tobytes()
        # as after today's pass no matching store is left: a transform is refused, a fetch too; the folding is still there
        with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
            ctx.consistency_match(0.25)
        with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
            ctx.mp(0)
        bps = ctx.bp(0)
        assert all(a[k].tobytes() == b[k].tobytes() for a, b in zip(bps, d["bps"]) for k in range(3))
        # and the device copy is the chosen matrix: the linkage tree of the block the pass left
        tree = ctx.linkage_tree("average")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(tree, linkage_ref(want, "average")))


def test_score_sequence_is_the_call_from_before(ctx, scored):
    names, seqs, family, out = scored
    for model in (capi.ALIGN_PROBCONS, capi.ALIGN_CONTRALIGN):
        for budget in (None, 1):
            ctx.set_sequences(seqs)
            want, want_ranges = ctx.similarity(model, 0.01, budget)
            ctx.set_sequences(seqs)
            got, got_ranges = ctx.similarity(model, 0.01, budget, score="sequence")
            assert got.tobytes() == want.tobytes() == out[model]["seq"].tobytes() and got_ranges == want_ranges
            with pytest.raises(capi.DafsHipError, match=r"code -1\b"):  # no structural pass: nothing was kept
                ctx.pair_scores()
    assert out[capi.ALIGN_PROBCONS]["ranges"] == 1


def test_without_a_fold_the_call_is_refused_and_the_context_goes_on(ctx, scored):
    names, seqs, family, out = scored
    ctx.set_sequences(seqs)
    for score in ("structure", "mix"):
        with pytest.raises(capi.DafsHipError, match=r"code -1\b.*no un-relaxed base-pairing store"):
            ctx.similarity(capi.ALIGN_PROBCONS, 0.01, score=score)
    ctx.align_posteriors(capi.ALIGN_PROBCONS, 0.01, fetch=False)
    with pytest.raises(capi.DafsHipError, match=r"code -1\b.*no un-relaxed base-pairing store"):
        ctx.structure_scores()
    ctx.set_sequences(seqs)
    ctx.fold_posteriors(0.01)
    with pytest.raises(capi.DafsHipError, match=r"code -1\b.*no un-relaxed matching store"):
        ctx.structure_scores()
    ctx.set_families([0, 7, 15])
    with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
        ctx.similarity(capi.ALIGN_PROBCONS, 0.01, score="structure")
    ctx.set_sequences(seqs)
    assert ctx.similarity(capi.ALIGN_PROBCONS, 0.01)[0].tobytes() == out[capi.ALIGN_PROBCONS]["seq"].tobytes()
    ctx.fold_posteriors(0.01)
    assert ctx.similarity(capi.ALIGN_PROBCONS, 0.01, score="structure")[0].tobytes() == out[capi.ALIGN_PROBCONS]["st"].tobytes()


# ------------------------------------------------------------------------------------------------------------ the drivers
_RUNS = {}


def _run_of(ctx, names, seqs, members):
    """pipeline.run of a cluster's members, computed once per member set"""
    key = tuple(members)
    if key not in _RUNS:
        _RUNS[key] = pipeline.run([names[i] for i in members], [seqs[i] for i in members], ctx=ctx)
    return _RUNS[key]


def _log(r):
    return {k: (v[0], v[1], v[2], np.float32(v[3]).tobytes()) for k, v in r.dd_log.items()}


@pytest.mark.parametrize("linkage", ["guide", "average"])
@pytest.mark.parametrize("score", ["sequence", "structure", "mix"])
def test_pipeline_cluster_on_each_score(ctx, scored, score, linkage):
    names, seqs, family, out = scored
    d = out[capi.ALIGN_PROBCONS]
    n = len(seqs)
    want = d["seq"] if score == "sequence" else d["st"] if score == "structure" else _mix(d["seq"], d["st"], 0.5)
    res = pipeline.cluster(names, seqs, count=6, ctx=ctx, linkage=linkage, score=score, min_size=3)
    assert res.score == score and res.linkage == linkage and res.ranges == 1
    assert res.sim.tobytes() == want.tobytes() and res.seq_sim.tobytes() == d["seq"].tobytes()
    if score == "sequence":
        assert res.struct_sim is None and set(res.seconds) == {"similarity", "tree", "batch", "total"}
    else:
        assert res.struct_sim.tobytes() == d["st"].tobytes() and set(res.seconds) == {"fold", "similarity", "tree", "batch", "total"}
    tree = capi.build_tree(want) if linkage == "guide" else linkage_ref(want, "average")
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(tree, res.tree))
    labels = cluster_ref.cut(tree, count=6)[0]
    assert np.array_equal(res.labels, labels)
    assert res.clusters == [[i for i in range(n) if labels[i] == c] for c in range(6)]
    assert res.table == cluster_ref.table(names, [len(s) for s in seqs], labels, tree, want)
    assert res.tree_line == pipeline._tree_line(tree[0], tree[1], tree[2], names)
    aligned = 0
    for members, got in zip(res.clusters, res.results):
        if len(members) < 3:
            assert got is None
            continue
        run = _run_of(ctx, names, seqs, members)
        assert got.output == run.output and _log(got) == _log(run) and got.sim.tobytes() == run.sim.tobytes()
        aligned += 1
    assert aligned >= 1


def _cli(*args):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.mark.parametrize("score,linkage,w", [("structure", "average", None), ("mix", "guide", 0.25), ("mix", "single", None)],
                         ids=["structure-average", "mix-guide-quarter", "mix-single"])
def test_cli_equals_python(ctx, scored, tmp_path, score, linkage, w):
    names, seqs, family, out = scored
    res = pipeline.cluster(names, seqs, count=6, ctx=ctx, linkage=linkage, score=score, structure_weight=w, min_size=3)
    fa = tmp_path / "set.fa"
    fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    tsv, tree = tmp_path / "t.tsv", tmp_path / "tree.txt"
    args = ["--cluster-count", 6, "--cluster-min-size", 3, "--cluster-linkage", linkage, "--cluster-score", score]
    if w is not None:
        args += ["--cluster-structure-weight", w]
    text = _cli(*args, "--cluster-table", tsv, "--cluster-tree", tree, fa)
    assert text == "".join("==> cluster %d <==\n" % (c + 1) + r.output for c, r in enumerate(res.results) if r is not None) and text
    assert tsv.read_text() == res.table
    assert tree.read_text() == res.tree_line + "\n"
    # the table carries the chosen score: with another score it is another table
    assert res.table != pipeline.cluster(names, seqs, count=6, ctx=ctx, linkage=linkage, min_size=len(seqs) + 1).table
