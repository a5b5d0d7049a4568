"""GPU tests of the clustering: Context.similarity (the similarity matrix computed in ranges of pairs),
pipeline.cluster and `dafs --cluster`.  The matrix must be, bit for bit, the one a full-pair-set align_posteriors leaves,
whatever the budget; every cluster's result must be, bit for bit, the plain run of its sequences."""
import math
import os
import subprocess

import numpy as np
import pytest

import cluster_ref
from dafs_amd import capi, pipeline, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")


def _mixed():
    """14 sequences: three families of four at about 40, 60 and 90 nt and two unrelated sequences of 9 and 130 nt, the
    families interleaved.  Ranges cut from this set fall into different launch plans (16-, 32- and 64-lane groups), the one
    way the range loop could change a score."""
    a, b, c = synth.family_set(4, 40, seed=71), synth.family_set(4, 60, seed=72), synth.family_set(4, 90, seed=73)
    short, long_ = synth.random_set(1, 9, seed=74, jitter=0.0)[0], synth.random_set(1, 130, seed=75, jitter=0.0)[0]
    recs = [("a%d" % k, a[k][1]) for k in range(4)] + [("b%d" % k, b[k][1]) for k in range(4)] + [("c%d" % k, c[k][1]) for k in range(4)]
    order = [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11]
    recs = [recs[k] for k in order[:5]] + [("r9", short[1])] + [recs[k] for k in order[5:]] + [("r130", long_[1])]
    return [n for n, _ in recs], [s for _, s in recs]


def _small():
    """6 sequences of 20 to 70 nt: a family of three, a family of two and an unrelated one (the CONTRAlign set)"""
    a, b = synth.family_set(3, 45, seed=81), synth.family_set(2, 65, seed=82)
    r = synth.random_set(1, 20, seed=83, jitter=0.0)[0]
    recs = [("a0", a[0][1]), ("b0", b[0][1]), ("a1", a[1][1]), ("r20", r[1]), ("b1", b[1][1]), ("a2", a[2][1])]
    return [n for n, _ in recs], [s for _, s in recs]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _full_sim(ctx, seqs, model):
    ctx.set_sequences(seqs)
    ctx.align_posteriors(model, 0.01, fetch=False)
    return ctx.sim()


@pytest.fixture(scope="module")
def mixed(ctx):
    """the 14 sequences, the similarity matrix of a full-pair-set align_posteriors (ProbCons) and the threshold of the tests:
    the score of join number ceil((N - 1) / 2) of the device's own tree, which keeps at least that many joins"""
    names, seqs = _mixed()
    sim = _full_sim(ctx, seqs, capi.ALIGN_PROBCONS)
    return names, seqs, sim, _middle_join(sim)


def _middle_join(sim):
    n = sim.shape[0]
    score, _, _ = capi.build_tree(sim)
    return float(score[n + math.ceil((n - 1) / 2) - 1])


def _budgets(seqs):
    lens = [len(s) for s in seqs]
    n = len(lens)
    total = sum(cluster_ref.pair_bytes(lens[x], lens[y]) for x in range(n) for y in range(x + 1, n))
    return lens, [(None, 1), (total, 1), (total // 4, None), (1, n * (n - 1) // 2)]


@pytest.mark.parametrize("model,inputs", [(capi.ALIGN_PROBCONS, _mixed), (capi.ALIGN_CONTRALIGN, _small), (capi.ALIGN_CONTRALIGN, _mixed)],
                         ids=["probcons", "contralign", "contralign-mixed"])
def test_similarity_in_ranges_equals_the_full_pair_set(ctx, model, inputs):
    names, seqs = inputs()
    want = _full_sim(ctx, seqs, model)
    lens, budgets = _budgets(seqs)
    for budget, n_ranges in budgets:
        ctx.set_sequences(seqs)
        sim, got_ranges = ctx.similarity(model, 0.01, budget)
        assert sim.tobytes() == want.tobytes(), budget
        assert got_ranges == len(capi.similarity_ranges(lens, budget))
        if n_ranges is not None:
            assert got_ranges == n_ranges
        else:
            assert 4 <= got_ranges <= 6
        # no store of the whole set is left, whatever the number of ranges: a transform is refused, not run on the last range
        with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
            ctx.consistency_match(0.25)
        with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
            ctx.mp(0)
        assert ctx.sim().tobytes() == want.tobytes()
    # the context goes on: a plain run on it
    assert pipeline.run(names[:3], seqs[:3], ctx=ctx).output == pipeline.run(names[:3], seqs[:3]).output


def test_similarity_refusals(ctx):
    names, seqs = _small()
    ctx.set_sequences(seqs)
    ctx.set_families([0, 3, 6])
    with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
        ctx.similarity()
    ctx.set_sequences(seqs[:1])
    with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
        ctx.similarity()
    ctx.set_sequences(seqs)
    with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
        ctx.similarity(model=7)
    assert ctx.similarity()[1] == 1


def _log(r):
    return {k: (v[0], v[1], v[2], np.float32(v[3]).tobytes()) for k, v in r.dd_log.items()}


def _check_clustering(ctx, names, seqs, res, threshold, **kw):
    """the partition is the restatement's on the returned matrix, and every cluster is the plain run of its sequences"""
    n = len(seqs)
    tree = capi.build_tree(res.sim)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(tree, res.tree))
    want, _ = cluster_ref.cut(tree, threshold=threshold)
    assert np.array_equal(res.labels, want)
    assert res.clusters == [[i for i in range(n) if want[i] == c] for c in range(int(want.max()) + 1)]
    assert len(res.clusters) > 1 and max(len(m) for m in res.clusters) >= 3
    assert res.tree_line == pipeline.tree_string(tree[0], tree[1], tree[2], names)
    assert res.table == cluster_ref.table(names, [len(s) for s in seqs], res.labels, tree, res.sim)
    assert len(res.results) == len(res.clusters)
    for members, got in zip(res.clusters, res.results):
        run = pipeline.run([names[i] for i in members], [seqs[i] for i in members], ctx=ctx, **kw)
        assert got.output == run.output
        assert _log(got) == _log(run)
        assert got.sim.tobytes() == run.sim.tobytes()
        if kw.get("reliability"):
            assert got.stockholm == run.stockholm
        if not kw.get("w_pct_f"):  # a cluster's own matrix is the piece of the whole set's (with -f it is the transformed one)
            assert got.sim.tobytes() == np.ascontiguousarray(res.sim[np.ix_(members, members)]).tobytes()


@pytest.mark.parametrize("kw", [dict(), dict(w_pct_f=0.5), dict(reliability=True)], ids=["plain", "fourway", "reliability"])
def test_clusters_equal_runs_of_their_sequences(ctx, mixed, kw):
    names, seqs, sim, threshold = mixed
    res = pipeline.cluster(names, seqs, threshold=threshold, ctx=ctx, **kw)
    assert res.sim.tobytes() == sim.tobytes() and res.ranges == 1  # with -f too: the clustering reads the raw scores
    assert set(res.seconds) == {"similarity", "tree", "batch", "total"}
    _check_clustering(ctx, names, seqs, res, threshold, **kw)


def test_clusters_equal_runs_contralign(ctx):
    names, seqs = _small()
    kw = dict(align_model=capi.ALIGN_CONTRALIGN)
    threshold = _middle_join(_full_sim(ctx, seqs, capi.ALIGN_CONTRALIGN))
    res = pipeline.cluster(names, seqs, threshold=threshold, ctx=ctx, **kw)
    _check_clustering(ctx, names, seqs, res, threshold, **kw)


def test_budget_count_and_min_size_change_no_result(ctx, mixed):
    names, seqs, sim, threshold = mixed
    base = pipeline.cluster(names, seqs, threshold=threshold, ctx=ctx)
    n = len(seqs)
    # one pair per range, and one cluster per sub-batch
    tight = pipeline.cluster(names, seqs, threshold=threshold, ctx=ctx, max_bytes=1)
    assert tight.ranges == n * (n - 1) // 2 and base.ranges == 1
    assert tight.sim.tobytes() == base.sim.tobytes() and np.array_equal(tight.labels, base.labels) and tight.table == base.table
    for a, b in zip(base.results, tight.results):
        assert a.output == b.output and _log(a) == _log(b) and a.sim.tobytes() == b.sim.tobytes()
    # the same partition asked for by its size
    by_count = pipeline.cluster(names, seqs, count=len(base.clusters), ctx=ctx, min_size=n + 1)
    assert np.array_equal(by_count.labels, base.labels) and by_count.clusters == base.clusters
    assert by_count.results == [None] * len(base.clusters) and by_count.table == base.table
    # small clusters are listed, not aligned
    big = pipeline.cluster(names, seqs, threshold=threshold, ctx=ctx, min_size=2)
    assert big.table == base.table and np.array_equal(big.labels, base.labels)
    for members, a, b in zip(base.clusters, base.results, big.results):
        if len(members) < 2:
            assert b is None
        else:
            assert a.output == b.output and _log(a) == _log(b)
    # a set of one sequence: one cluster, no launch of the pair kernels
    one = pipeline.cluster(names[:1], seqs[:1], threshold=0.5, ctx=ctx)
    assert one.ranges == 0 and one.clusters == [[0]] and one.results[0].output == pipeline.run(names[:1], seqs[:1], ctx=ctx).output


def _cli(*args):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_cluster_equals_python_and_files_of_the_clusters(ctx, tmp_path):
    """stdout, --cluster-table, --cluster-tree and the Stockholm blocks are the Python driver's; each stdout block is `dafs` on
    a file of that cluster"""
    names, seqs = _small()
    recs = list(zip(names, seqs))
    threshold = _middle_join(_full_sim(ctx, seqs, capi.ALIGN_PROBCONS))
    res = pipeline.cluster(names, seqs, threshold=threshold, ctx=ctx, reliability=True)
    assert len(res.clusters) > 1 and max(len(m) for m in res.clusters) >= 3
    fa = tmp_path / "six.fa"
    fa.write_text(synth.to_fasta(recs))
    tsv, tree, sto = tmp_path / "t.tsv", tmp_path / "tree.txt", tmp_path / "out.sto"
    out = _cli("--cluster", repr(threshold), "--cluster-table", tsv, "--cluster-tree", tree, "--stockholm", sto, fa)
    assert out == "".join("==> cluster %d <==\n" % (c + 1) + r.output for c, r in enumerate(res.results))
    assert tsv.read_text() == res.table
    assert tree.read_text() == res.tree_line + "\n"
    assert sto.read_text() == "".join(r.stockholm for r in res.results)
    assert sto.read_text().count("# STOCKHOLM 1.0") == len(res.clusters)
    want = ""
    for c, members in enumerate(res.clusters):
        one = tmp_path / ("c%d.fa" % c)
        one.write_text(synth.to_fasta([recs[i] for i in members]))
        want += "==> cluster %d <==\n" % (c + 1) + _cli(one)
    assert out == want
    # by count, small clusters left out: the same blocks without the singletons', the table unchanged
    tsv2 = tmp_path / "t2.tsv"
    out2 = _cli("--cluster-count", len(res.clusters), "--cluster-min-size", 2, "--cluster-table", tsv2, fa)
    assert out2 == "".join("==> cluster %d <==\n" % (c + 1) + r.output for c, r in enumerate(res.results) if len(res.clusters[c]) >= 2)
    assert tsv2.read_text() == res.table


def test_cli_cluster_side_outputs_equal_python(ctx, tmp_path):
    """--stockholm with --row-structures, --covariation and --identity with --identity-matrix under --cluster: one block or table
    per printed cluster, the tables under the cluster's header line, all the Python driver's; a cluster of one sequence among them"""
    names, seqs = _small()
    threshold = _middle_join(_full_sim(ctx, seqs, capi.ALIGN_PROBCONS))
    res = pipeline.cluster(names, seqs, threshold=threshold, ctx=ctx, reliability=True, row_structures=True, identity=True,
                           covariation=dict(shuffles=20, seed=3))
    assert len(res.clusters) > 1 and min(len(m) for m in res.clusters) == 1
    fa = tmp_path / "six.fa"
    fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    sto, cov, idt, mat = tmp_path / "out.sto", tmp_path / "cov.tsv", tmp_path / "id.tsv", tmp_path / "id.mat"
    out = _cli("--cluster", repr(threshold), "--stockholm", sto, "--row-structures", "--covariation", cov, "--cov-shuffles", 20, "--cov-seed", 3,
               "--identity", idt, "--identity-matrix", mat, fa)
    heads = ["==> cluster %d <==\n" % (c + 1) for c in range(len(res.clusters))]
    assert out == "".join(h + r.output for h, r in zip(heads, res.results))
    assert sto.read_text() == "".join(r.stockholm for r in res.results)
    lines = sto.read_text().split("\n")
    assert sum(1 for ln in lines if ln.startswith("#=GR ") and ln.split()[2] == "SS") == len(seqs)
    assert sum(1 for ln in lines if ln.startswith("#=GS ") and ln.split()[2] == "WT") == len(seqs)
    assert cov.read_text() == "".join(h + pipeline.covariation_tsv(r) for h, r in zip(heads, res.results))
    assert idt.read_text() == "".join(h + pipeline.identity_tsv(r.row_names, r.identity) for h, r in zip(heads, res.results))
    assert mat.read_text() == "".join(h + pipeline.identity_matrix_tsv(r.row_names, r.identity) for h, r in zip(heads, res.results))
