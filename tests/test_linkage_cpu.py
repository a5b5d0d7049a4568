"""CPU tests of the linkage rules: the two facts about the contract that make a cut of these trees
meaningful (join scores never rise; a subtree is the tree of its members alone) on the numpy restatement, the host cut and
table on its trees, hand-checkable cases, the library's exports, and every refusal that needs no device -- of capi, of
pipeline.cluster, of the library's entry points and of `dafs --cluster-linkage`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cluster_ref
from linkage_ref import RULES, canon, chain_case, leaves, linkage_ref
from dafs_amd import capi, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
RF00005 = os.path.join(ROOT, "tests", "golden", "RF00005_0.fa")  # ten sequences


def _matrices():
    """symmetric, unit diagonal, N = 1 .. 33, every third rounded to quarters so that joins tie"""
    rng = np.random.default_rng(21)
    out = []
    for n in range(1, 34):
        s = rng.random((n, n)).astype(np.float32)
        if n % 3 == 2:
            s = (np.round(s * 4) / 4).astype(np.float32)
        s = np.maximum(s, s.T)
        np.fill_diagonal(s, 1.0)
        out.append(s)
    return out


_SIMS = _matrices()
_TREES = {rule: [linkage_ref(s, rule) for s in _SIMS] for rule in RULES}


@pytest.mark.parametrize("rule", RULES)
def test_join_scores_never_rise(rule):
    for sim, (score, left, right) in zip(_SIMS, _TREES[rule]):
        n = sim.shape[0]
        assert (score[:n] == 0).all() and (left[:n] == -1).all() and (right[:n] == -1).all()
        assert (np.diff(score[n:]) <= 0).all(), (n, score[n:])
        for i in range(n, 2 * n - 1):  # the children are earlier nodes
            assert 0 <= left[i] < i and 0 <= right[i] < i and left[i] != right[i]


@pytest.mark.parametrize("rule", RULES)
def test_a_subtree_is_the_tree_of_its_members(rule):
    """for every join of every tree: the linkage of the members' sub-matrix is the relabelled subtree, topology and score bits"""
    checked = 0
    for sim, tree in zip(_SIMS, _TREES[rule]):
        n = sim.shape[0]
        for node in range(n, 2 * n - 1):
            m = leaves(tree, node)
            sub = linkage_ref(sim[np.ix_(m, m)], rule)
            assert canon(sub, len(sub[0]) - 1, list(range(len(m)))) == canon(tree, node, {x: i for i, x in enumerate(m)}), (n, node)
            checked += 1
    assert checked == sum(s.shape[0] - 1 for s in _SIMS)


@pytest.mark.parametrize("rule", RULES)
def test_the_host_cut_and_table_accept_the_trees(rule):
    for sim, tree in zip(_SIMS, _TREES[rule]):
        score = tree[0]
        n = sim.shape[0]
        names, lengths = ["s%d" % i for i in range(n)], [10 + i for i in range(n)]
        for k in range(1, n + 1):  # count = K gives exactly K clusters
            labels, got = capi.cluster_cut(tree, count=k)
            assert got == k and len(set(labels.tolist())) == k
            assert (labels == cluster_ref.cut(tree, count=k)[0]).all()
            if k in (1, (n + 1) // 2, n):
                assert capi.cluster_table(names, lengths, labels, tree, sim).count("\n") == n
        joins = sorted(set(float(x) for x in score[n:]))
        for th in joins + [(a + b) / 2 for a, b in zip(joins, joins[1:])] + [0.0, 1.5]:
            labels, k = capi.cluster_cut(tree, threshold=th)
            # scores never rise: "kept" is "joined before the first score below the threshold"
            below = [t for t in range(n - 1) if score[n + t] < np.float32(th)]
            first = below[0] if below else n - 1
            assert cluster_ref.kept_joins(tree, threshold=th) == [True] * n + [t < first for t in range(n - 1)]
            assert k == n - first
            assert (labels == cluster_ref.cut(tree, threshold=th)[0]).all()
            assert capi.cluster_table(names, lengths, labels, tree, sim).count("\n") == n


def _f32(x):
    return np.float32(x)


def _mean(weights, values):
    """the contract's average: exact products, one rounding each for the sum, the quotient and the narrowing"""
    s = np.float64(0)
    for w, v in zip(weights, values):
        s = s + np.float64(w) * np.float64(_f32(v))
    return _f32(s / np.float64(sum(weights)))


def test_three_rules_three_trees_by_hand():
    """0 and 1 join first at 0.9.  Then single sees S(01,2) = 0.85, S(01,3) = 0.8, S(2,3) = 0.5: 2 joins, then 3.  Complete sees
    0.05, 0.3, 0.5: 2 and 3 join, then the two pairs at min(0.05, 0.3).  Average sees 0.45, 0.55, 0.5: 3 joins, then 2 at
    (2 * 0.45 + 0.5) / 3."""
    sim = np.eye(4, dtype=np.float32)
    for (x, y), v in {(0, 1): .9, (0, 2): .85, (1, 2): .05, (0, 3): .3, (1, 3): .8, (2, 3): .5}.items():
        sim[x, y] = sim[y, x] = v
    leaf = [-1, -1, -1, -1]
    want = {
        "single": ([0, 0, 0, 0, _f32(.9), _f32(.85), _f32(.8)], leaf + [0, 4, 5], leaf + [1, 2, 3]),
        "complete": ([0, 0, 0, 0, _f32(.9), _f32(.5), _f32(.05)], leaf + [0, 2, 4], leaf + [1, 3, 5]),
        "average": ([0, 0, 0, 0, _f32(.9), _mean([1, 1], [.3, .8]), _mean([2, 1], [_mean([1, 1], [.85, .05]), .5])], leaf + [0, 4, 5],
                    leaf + [1, 3, 2]),
    }
    for rule in RULES:
        score, left, right = linkage_ref(sim, rule)
        assert score.tobytes() == np.array(want[rule][0], np.float32).tobytes(), rule
        assert left.tolist() == want[rule][1] and right.tolist() == want[rule][2], rule
    assert len({(tuple(t[1]), tuple(t[2])) for t in want.values()}) == 3  # three topologies


@pytest.mark.parametrize("rule", RULES)
def test_the_all_equal_matrix_is_a_left_comb(rule):
    n = 7
    sim = np.full((n, n), 0.5, np.float32)
    score, left, right = linkage_ref(sim, rule)
    assert score.tolist() == [0.0] * n + [0.5] * (n - 1)
    assert left.tolist() == [-1] * n + [0] + list(range(n, 2 * n - 2))  # slot 0 holds the growing cluster
    assert right.tolist() == [-1] * n + list(range(1, n))               # and takes the next slot


@pytest.mark.parametrize("rule", RULES)
def test_the_closed_form_of_the_chain_matrix(rule):
    """the GPU tests use chain_case at sizes the restatement is too slow for: here the closed form is the restatement's tree"""
    for n in (1, 2, 3, 37, 130):
        sim, want = chain_case(n)
        assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(linkage_ref(sim, rule), want)), n


def test_zero_and_minus_zero_are_equal_and_slot_a_wins():
    sim = np.array([[1, -0.0, 0.0], [0, 1, 0.0], [0, 0, 1]], np.float32)
    for rule in RULES:
        score, left, right = linkage_ref(sim, rule)
        assert (left[3], right[3]) == (0, 1) and np.signbit(score[3])  # the first of the equal entries, with its sign
        assert (left[4], right[4]) == (3, 2)
    nan_below = sim.copy()
    nan_below[np.tril_indices(3, -1)] = np.nan
    for rule in RULES:
        assert all(x.tobytes() == y.tobytes() for x, y in zip(linkage_ref(sim, rule), linkage_ref(nan_below, rule)))


def test_the_library_exports_the_entry_points():
    for name in ("dafs_hip_linkage_tree", "dafs_hipk_linkage", "dafs_hipk_linkage_workspace"):
        assert getattr(capi.lib, name) is not None
    assert capi.LINKAGES == ("guide", "single", "complete", "average")
    assert capi.linkage_workspace(0) == 0 and capi.linkage_workspace(65537) == 0
    for n in (1, 2, 1100, 32768):
        assert capi.linkage_workspace(n) >= n * n * 4 + 16 * n and capi.linkage_workspace(n) % 256 == 0


def test_capi_refuses_before_it_needs_a_context():
    good = np.eye(3, dtype=np.float32)
    with pytest.raises(ValueError, match="unknown rule"):
        capi.linkage_check("ward", good)
    with pytest.raises(ValueError, match="build_tree"):
        capi.linkage_check("guide", good)
    with pytest.raises(ValueError, match="n x n"):
        capi.linkage_check("single", np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="n x n"):
        capi.linkage_check("single", np.zeros(4, np.float32))
    for bad in (np.nan, np.inf, -np.inf):
        m = good.copy()
        m[0, 2] = bad
        with pytest.raises(ValueError, match="not finite"):
            capi.linkage_check("average", m)
        code, kept = capi.linkage_check("average", m.T)  # below the diagonal nothing is read
        assert code == 3 and kept.shape == (3, 3)
    assert [capi.linkage_check(r)[0] for r in RULES] == [1, 2, 3]
    # Context.linkage_tree runs the same checks first: no handle is touched
    ctx = object.__new__(capi.Context)
    ctx._h, ctx._lens = None, None
    with pytest.raises(ValueError, match="unknown rule"):
        ctx.linkage_tree("centroid")
    with pytest.raises(ValueError, match="build_tree"):
        ctx.linkage_tree("guide", good)


def test_the_library_refuses_without_a_device():
    f, i = np.zeros(8, np.float32), np.zeros(8, np.int32)
    args = (f.ctypes.data, f.ctypes.data, i.ctypes.data, i.ctypes.data)
    assert capi._linkage_tree(None, 1, 2, *args) == -1 and b"missing argument" in capi._last_error()
    one = C.c_void_p(256)  # never dereferenced: every refusal below comes first
    for rule, n, ptrs, why in ((0, 4, (one,) * 5, b"unknown linkage"), (4, 4, (one,) * 5, b"unknown linkage"),
                               (1, 1, (one,) * 5, b"2 to 65536"), (1, 65537, (one,) * 5, b"2 to 65536"),
                               (2, 4, (None,) + (one,) * 4, b"missing argument"), (3, 4, (one, C.c_void_p(8)) + (one,) * 3, b"256-byte aligned")):
        assert capi.linkage_launch(rule, n, *ptrs, None) == -1
        assert why in capi._last_error(), (rule, n, capi._last_error())


def test_pipeline_cluster_refuses_a_bad_rule_before_it_opens_a_context(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a context was opened")
    monkeypatch.setattr(capi, "Context", no_context)
    names, seqs = ["a", "b", "c"], ["ACGUACGU", "ACGGACGU", "UUUUCCCC"]
    for bad in ("ward", "centroid", "", None, 1):
        with pytest.raises(ValueError, match="unknown linkage"):
            pipeline.cluster(names, seqs, threshold=0.5, linkage=bad)
    for rule in capi.LINKAGES:  # the checks passed: the next step is the context
        with pytest.raises(AssertionError, match="a context was opened"):
            pipeline.cluster(names, seqs, count=2, linkage=rule)


@pytest.mark.parametrize("args,message", [
    (["--cluster", "0.5", "--cluster-linkage", "ward", RF00005], "--cluster-linkage: unknown rule 'ward'"),
    (["--cluster-count", "2", "--cluster-linkage", "Average", RF00005], "--cluster-linkage: unknown rule 'Average'"),
    (["--cluster-count", "2", "--cluster-linkage=", RF00005], "--cluster-linkage: unknown rule ''"),
    (["--cluster-linkage", "average", RF00005], "--cluster-linkage needs --cluster or --cluster-count"),
    (["--cluster-linkage", "guide", RF00005], "--cluster-linkage needs --cluster or --cluster-count"),
    (["--cluster-count", "2", "--cluster-linkage", "single", "--devices", "0,1", RF00005], "--devices cannot be combined with --cluster"),
])
def test_cli_refuses_while_parsing(args, message, tmp_path):
    assert os.path.exists(DAFS), "the dafs executable is built by build()"
    r = subprocess.run([DAFS] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert r.stderr.count("\n") == 1 and "HIP" not in r.stderr
    assert r.stdout == ""
    assert os.listdir(str(tmp_path)) == []


def test_cli_help_names_the_option():
    r = subprocess.run([DAFS, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "--cluster-linkage RULE" in text and text.index("--cluster-tree OUT") < text.index("--cluster-linkage RULE") < text.index("Aligning options")
