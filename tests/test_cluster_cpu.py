"""CPU tests of the clustering: the cut of the guide tree (dafs_host_cluster_cut) against a plain-Python
restatement, the two facts about DAFS::build_tree that make the cut meaningful (join scores never rise; a subtree is the tree
of its members alone), the ranges of the similarity pass, the cluster table's bytes, and the refusals of pipeline.cluster and
of `dafs --cluster` -- all before any HIP call."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import cluster_ref
import text_ref
from dafs_amd import capi, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
G = os.path.join(ROOT, "tests", "golden")
RF00005 = os.path.join(G, "RF00005_0.fa")  # ten sequences


def _blocks(n, groups, inside, outside):
    s = np.full((n, n), outside, np.float32)
    for g in groups:
        for i in g:
            for j in g:
                s[i, j] = inside
    np.fill_diagonal(s, 1.0)
    return s


def _matrices():
    """symmetric, unit diagonal, values in [0, 1]: hand-made ones, and seeded random ones of N = 1, 2, 3, 8, 33, every third
    rounded to quarters so that joins tie"""
    out = [np.ones((1, 1), np.float32), np.array([[1, 0.4], [0.4, 1]], np.float32),
           np.array([[1, .9, .1, .1], [.9, 1, .1, .1], [.1, .1, 1, .8], [.1, .1, .8, 1]], np.float32),
           np.array([[1, .1, .9, .1], [.1, 1, .1, .8], [.9, .1, 1, .1], [.1, .8, .1, 1]], np.float32),  # interleaved clusters
           _blocks(8, [[0, 3, 5], [1, 2], [4, 6, 7]], 0.75, 0.25), _blocks(3, [[0, 1, 2]], 0.5, 0.5)]
    rng = np.random.default_rng(20)
    for n in (2, 3, 8, 33):
        for rep in range(3):
            s = rng.random((n, n)).astype(np.float32)
            if rep == 2:
                s = (np.round(s * 4) / 4).astype(np.float32)
            s = np.maximum(s, s.T)
            np.fill_diagonal(s, 1.0)
            out.append(s)
    return out


def _cuts(tree):
    """the cuts tried on a tree: every join score as the threshold (>= keeps that join), the midpoints between them, 0 (one
    cluster) and above 1 (all singletons); 1, a middle and n clusters by count"""
    score = tree[0]
    n = (len(score) + 1) // 2
    joins = sorted(set(float(x) for x in score[n:]))
    ths = joins + [(a + b) / 2 for a, b in zip(joins, joins[1:])] + [0.0, 1.5]
    counts = sorted({1, (n + 1) // 2, n})
    return [dict(threshold=t) for t in ths] + [dict(count=k) for k in counts]


_CASES = [(sim, capi.build_tree(sim)) for sim in _matrices()]


def test_build_tree_is_the_restatement():
    for sim, tree in _CASES:
        want = text_ref.build_tree(sim)
        assert tree[0].tobytes() == want[0].tobytes() and np.array_equal(tree[1], want[1]) and np.array_equal(tree[2], want[2])


def test_cut_equals_the_restatement():
    for sim, tree in _CASES:
        n = sim.shape[0]
        for kw in _cuts(tree):
            labels, k = capi.cluster_cut(tree, **kw)
            want, roots = cluster_ref.cut(tree, **kw)
            assert labels.dtype == np.uint32 and np.array_equal(labels, want), (n, kw)
            assert k == len(roots) == int(labels.max()) + 1
            # numbered by the smallest member: the first appearances of the labels are 0, 1, 2, ...
            first = [int(np.flatnonzero(labels == c)[0]) for c in range(k)]
            assert first == sorted(first)
            if "count" in kw:
                assert k == kw["count"]
        assert capi.cluster_cut(tree, threshold=0.0)[1] == 1
        assert capi.cluster_cut(tree, threshold=1.5)[1] == n
        assert capi.cluster_cut(tree, count=1)[1] == 1 and capi.cluster_cut(tree, count=n)[1] == n


def test_cut_of_hand_made_trees():
    two_pairs, interleaved = _CASES[2][1], _CASES[3][1]
    assert [float(x) for x in two_pairs[0][4:6]] == [np.float32(0.9), np.float32(0.8)]
    assert list(capi.cluster_cut(two_pairs, threshold=float(np.float32(0.8)))[0]) == [0, 0, 1, 1]  # >= keeps the join at T
    assert list(capi.cluster_cut(two_pairs, threshold=0.85)[0]) == [0, 0, 1, 2]
    assert list(capi.cluster_cut(two_pairs, threshold=0.95)[0]) == [0, 1, 2, 3]
    assert list(capi.cluster_cut(two_pairs, threshold=0.0)[0]) == [0, 0, 0, 0]
    assert list(capi.cluster_cut(two_pairs, count=2)[0]) == [0, 0, 1, 1]
    assert list(capi.cluster_cut(two_pairs, count=3)[0]) == [0, 0, 1, 2]
    assert list(capi.cluster_cut(interleaved, threshold=0.5)[0]) == [0, 1, 0, 1]  # members keep the input order
    assert list(capi.cluster_cut(_CASES[4][1], threshold=0.5)[0]) == [0, 1, 1, 0, 2, 0, 2, 2]
    # a join above the threshold over a join below it is not kept: "every join below it is kept"
    score = np.array([0, 0, 0, 0.2, 0.9], np.float32)
    left, right = np.array([-1, -1, -1, 0, 3]), np.array([-1, -1, -1, 1, 2])
    assert list(capi.cluster_cut((score, left, right), threshold=0.5)[0]) == [0, 1, 2]


def _raw_cut(n, score, left, right, mode, threshold, count, labels=True, k=True):
    score = None if score is None else np.ascontiguousarray(score, np.float32)
    left = None if left is None else np.ascontiguousarray(left, np.int32)
    right = None if right is None else np.ascontiguousarray(right, np.int32)
    out = np.zeros(max(n, 1), np.uint32)
    cnt = C.c_uint32()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return capi._cluster_cut(n, ptr(score), ptr(left), ptr(right), mode, threshold, count, out.ctypes.data if labels else None,
                             C.byref(cnt) if k else None)


def test_cut_refusals():
    score, left, right = capi.build_tree(_matrices()[4])
    n = 8
    assert _raw_cut(n, score, left, right, capi.CLUSTER_THRESHOLD, 0.5, 0) == 0
    for bad in (dict(score=None), dict(left=None), dict(right=None)):
        args = dict(score=score, left=left, right=right)
        args.update(bad)
        assert _raw_cut(n, args["score"], args["left"], args["right"], capi.CLUSTER_THRESHOLD, 0.5, 0) == -1
    assert _raw_cut(n, score, left, right, capi.CLUSTER_THRESHOLD, 0.5, 0, labels=False) == -1
    assert _raw_cut(n, score, left, right, capi.CLUSTER_THRESHOLD, 0.5, 0, k=False) == -1
    assert _raw_cut(0, score, left, right, capi.CLUSTER_THRESHOLD, 0.5, 0) == -1
    assert _raw_cut(n, score, left, right, 2, 0.5, 1) == -1  # unknown mode
    assert _raw_cut(n, score, left, right, capi.CLUSTER_THRESHOLD, math.nan, 0) == -1
    assert b"not a number" in capi._last_error()
    for k in (0, n + 1):
        assert _raw_cut(n, score, left, right, capi.CLUSTER_COUNT, 0.0, k) == -1
        with pytest.raises(ValueError, match="number of clusters"):
            capi.cluster_cut((score, left, right), count=k)
    with pytest.raises(ValueError, match="not a number"):
        capi.cluster_cut((score, left, right), threshold=math.nan)
    for kw in (dict(), dict(threshold=0.5, count=2)):
        with pytest.raises(ValueError, match="exactly one"):
            capi.cluster_cut((score, left, right), **kw)
    with pytest.raises(ValueError, match="2 n - 1"):
        capi.cluster_cut((score[:-1], left[:-1], right[:-1]), count=1)
    # malformed trees
    def broken(edit):
        l, r = left.copy(), right.copy()
        edit(l, r)
        with pytest.raises(ValueError, match="malformed tree"):
            capi.cluster_cut((score, l, r), count=1)
    broken(lambda l, r: l.__setitem__(0, 3))            # a leaf with a child
    broken(lambda l, r: l.__setitem__(n, n))            # a join of itself
    broken(lambda l, r: l.__setitem__(n, 2 * n - 2))    # a child that comes later
    broken(lambda l, r: l.__setitem__(n, -1))           # a join without a child
    broken(lambda l, r: l.__setitem__(2 * n - 2, int(l[n])))  # a node that is a child twice (and one that never is)
    broken(lambda l, r: r.__setitem__(n, int(l[n])))    # both children the same node
    one = (np.zeros(1, np.float32), -np.ones(1, np.int64), -np.ones(1, np.int64))
    assert list(capi.cluster_cut(one, threshold=0.9)[0]) == [0] and capi.cluster_cut(one, count=1)[1] == 1


def test_join_scores_never_rise():
    """for similarities in [0, 1] a merged distance (d1 + d2) * s / 2 is at most s: "kept" is "joined before the first score
    below T"."""
    for sim, (score, _, _) in _CASES:
        n = sim.shape[0]
        assert np.all(np.diff(score[n:]) <= 0), n


def test_a_cluster_subtree_is_the_tree_of_its_members():
    """for every cluster of every cut: build_tree on the cluster's sub-matrix is the relabelled subtree, same topology, the
    scores to the bit -- so a cluster's printed tree line is the matching piece of the whole set's"""
    checked = 0
    for sim, tree in _CASES:
        n = sim.shape[0]
        seen = set()
        for kw in _cuts(tree):
            labels, roots = cluster_ref.cut(tree, **kw)
            for c, node in enumerate(roots):
                if node < n or node in seen:
                    continue
                seen.add(node)
                m = [int(i) for i in np.flatnonzero(labels == c)]
                sub = capi.build_tree(np.ascontiguousarray(sim[np.ix_(m, m)]))
                a = cluster_ref.subtree_canon(tree, node, {x: i for i, x in enumerate(m)})
                b = cluster_ref.subtree_canon(sub, 2 * len(m) - 2, {i: i for i in range(len(m))})
                assert a == b, (n, kw, c)
                checked += 1
    assert checked > 100


def _check_ranges(lens, budget):
    got = capi.similarity_ranges(lens, budget)
    n = len(lens)
    pairs = [(x, y) for x in range(n) for y in range(x + 1, n)]
    assert got == cluster_ref.ranges(lens, budget)
    # every pair once, in order
    assert [b for b, _ in got] == [0] + [e for _, e in got[:-1]] and (got[-1][1] if got else 0) == len(pairs)
    for b, e in got:
        assert e > b
        size = sum(cluster_ref.pair_bytes(lens[x], lens[y]) for x, y in pairs[b:e])
        assert size <= budget or e - b == 1
        if e < len(pairs):  # greedy: the next pair would not have fitted
            assert size + cluster_ref.pair_bytes(*[lens[i] for i in pairs[e]]) > budget
    return got


def test_similarity_ranges():
    lens = [40, 38, 41, 9, 60, 62, 59, 130, 90, 91, 88, 61, 39, 92]
    n = len(lens)
    np_all = n * (n - 1) // 2
    total = sum(cluster_ref.pair_bytes(lens[x], lens[y]) for x in range(n) for y in range(x + 1, n))
    assert _check_ranges(lens, total) == [(0, np_all)]
    assert len(_check_ranges(lens, total - 1)) == 2
    assert 4 <= len(_check_ranges(lens, total // 4)) <= 6
    many = _check_ranges(lens, 3 * cluster_ref.pair_bytes(60, 60))
    assert len(many) > 20
    assert _check_ranges(lens, 1) == [(p, p + 1) for p in range(np_all)]  # every pair over the budget: one per range
    assert capi.similarity_ranges(lens) == [(0, np_all)]  # the library's budget
    assert capi.similarity_ranges(lens, int(capi._batch_bytes())) == [(0, np_all)]
    assert capi.similarity_ranges([50]) == [] and capi.similarity_ranges([]) == []
    assert _check_ranges([7, 300], 10) == [(0, 1)]
    with pytest.raises(ValueError):
        capi.similarity_ranges(lens, 0)
    count = C.c_uint64()
    assert capi._similarity_ranges(3, None, 1, None, 0, C.byref(count)) == -1
    three = np.array([5, 6, 7], np.uint32)
    assert capi._similarity_ranges(3, three.ctypes.data, 1, None, 0, None) == -1
    assert capi._similarity_ranges(3, three.ctypes.data, 1, None, 2, C.byref(count)) == -1
    end = np.zeros(2, np.uint64)  # fewer places than ranges: the count is whole, the places are filled
    assert capi._similarity_ranges(3, three.ctypes.data, 1, end.ctypes.data, 2, C.byref(count)) == 0
    assert count.value == 3 and list(end) == [1, 2]


def test_cluster_table_equals_the_restatement():
    for sim, tree in _CASES:
        n = sim.shape[0]
        headers = ["seq %d of the set" % i if i % 3 else "dup" for i in range(n)]
        if n > 4:
            headers[4] = ""
        lengths = [10 + 3 * i for i in range(n)]
        for kw in _cuts(tree):
            labels, _ = capi.cluster_cut(tree, **kw)
            got = capi.cluster_table(headers, lengths, labels, tree, sim)
            assert got == cluster_ref.table(headers, lengths, labels, tree, sim), (n, kw)
            assert got.count("\n") == n
    # singletons, one sequence, and ties in the nearest sequence, written out
    one = capi.cluster_table(["only one"], [7], [0], _CASES[0][1], _CASES[0][0])
    assert one == "1\tonly\t7\t1\t1\tnan\t0\tnan\t0\tnan\n"
    sim, tree = _CASES[4]
    labels, k = capi.cluster_cut(tree, threshold=0.5)
    lines = capi.cluster_table(["s%d" % i for i in range(8)], [20] * 8, labels, tree, sim).splitlines()
    assert k == 3
    # sequence 1: sequences 4 and 6 tie inside its cluster, 2, 3, 5, 7 and 8 outside; its cluster's top join is
    # (0.75 + 0.75) * 0.75 / 2, sequence 1 against the join of 4 and 6
    assert lines[0] == "1\ts0\t20\t1\t3\t0.5625\t4\t0.75\t2\t0.25"
    assert lines[1] == "2\ts1\t20\t2\t2\t0.75\t3\t0.75\t1\t0.25"
    singles = capi.cluster_table(["a", "b"], [5, 6], [0, 1], _CASES[1][1], _CASES[1][0]).splitlines()
    assert singles == ["1\ta\t5\t1\t1\tnan\t0\tnan\t2\t%s" % text_ref._fmt9(np.float32(0.4)),
                       "2\tb\t6\t2\t1\tnan\t0\tnan\t1\t%s" % text_ref._fmt9(np.float32(0.4))]
    with pytest.raises(ValueError, match="not those of a cut"):
        capi.cluster_table(["s%d" % i for i in range(8)], [20] * 8, [0, 1, 0, 1, 0, 1, 0, 1], tree, sim)
    with pytest.raises(ValueError, match="one header"):
        capi.cluster_table(["a"], [5, 6], [0, 1], _CASES[1][1], _CASES[1][0])


def test_pipeline_cluster_refuses_before_it_opens_a_context(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a context was opened")
    monkeypatch.setattr(capi, "Context", no_context)
    names, seqs = ["a", "b", "c"], ["ACGUACGU", "ACGGACGU", "UUUUCCCC"]
    bad = [dict(), dict(threshold=0.5, count=2), dict(threshold=math.nan), dict(threshold=math.inf), dict(count=0), dict(count=4),
           dict(count=1.5), dict(threshold=0.5, min_size=0), dict(threshold=0.5, max_bytes=0), dict(threshold=0.5, mp=None),
           dict(threshold=0.5, bp=None), dict(threshold=0.5, shard=None), dict(threshold=0.5, compare=(["a"], ["A"])),
           dict(threshold=0.5, level_sync=True, bp_update=True), dict(threshold=0.5, covariation=dict(no_such_key=1))]
    for kw in bad:
        with pytest.raises(ValueError):
            pipeline.cluster(names, seqs, **kw)
    with pytest.raises(TypeError):
        pipeline.cluster(names, seqs, threshold=0.5, no_such_option=1)
    for nm, sq in (([], []), (["a"], ["ACGU", "ACGU"]), (["a", "b"], ["ACGU", ""])):
        with pytest.raises(ValueError):
            pipeline.cluster(nm, sq, threshold=0.5)
    with pytest.raises(AssertionError, match="a context was opened"):  # the checks passed: the next step is the context
        pipeline.cluster(names, seqs, threshold=0.5)


@pytest.mark.parametrize("args,message", [
    (["--cluster", "0.5"], "exactly one input FILE"),
    (["--cluster", "0.5", RF00005, RF00005], "exactly one input FILE"),
    (["--cluster", "0.5", "--cluster-count", "2", RF00005], "give one of them"),
    (["--cluster-table", "t.tsv", RF00005], "need --cluster or --cluster-count"),
    (["--cluster-tree", "t.txt", RF00005], "need --cluster or --cluster-count"),
    (["--cluster-min-size", "2", RF00005], "need --cluster or --cluster-count"),
    (["--cluster", "nan", RF00005], "finite threshold"),
    (["--cluster", "inf", RF00005], "finite threshold"),
    (["--cluster", "0.5x", RF00005], "finite threshold"),
    (["--cluster-count", "0", RF00005], "positive integer"),
    (["--cluster-count", "-3", RF00005], "positive integer"),
    (["--cluster", "0.5", "--cluster-min-size", "0", RF00005], "positive integer"),
    (["--cluster", "0.5", "--cluster-table", "", RF00005], "needs a file name"),
    (["--cluster", "0.5", "--seed", RF00005, RF00005], "--seed cannot be combined with --cluster"),
    (["--cluster", "0.5", "--seed", RF00005, "--seed-each", RF00005], "cannot be combined with --cluster"),
    (["--cluster", "0.5", "--seed-scores", "x", RF00005], "--seed-scores cannot be combined with --cluster"),
    (["--cluster", "0.5", "--pairwise", RF00005], "--pairwise cannot be combined with --cluster"),
    (["--cluster", "0.5", "--pairwise-scores", "x", RF00005], "--pairwise-scores cannot be combined with --cluster"),
    (["--cluster", "0.5", "--describe", RF00005, "--identity", "x"], "--describe cannot be combined with --cluster"),
    (["--cluster-count", "2", "--devices", "0,1", RF00005], "--devices cannot be combined with --cluster"),
    (["--cluster", "0.5", "--compare", "x", "--compare-ref", RF00005, RF00005], "cannot be combined with --cluster"),
    (["--cluster", "0.5", "--compare-matrix", "x", RF00005], "--compare-matrix cannot be combined with --cluster"),
    (["--cluster", "0.5", "--align-aux", "x", RF00005], "--align-aux cannot be combined with --cluster"),
    (["--cluster", "0.5", "--fold-aux", "x", RF00005], "--fold-aux cannot be combined with --cluster"),
    (["--cluster", "0.5", "--save-align-aux", "x", RF00005], "--save-align-aux cannot be combined with --cluster"),
    (["--cluster-count", "3", "--save-fold-aux", "x", RF00005], "--save-fold-aux cannot be combined with --cluster"),
    (["--cluster-count", "11", RF00005], "11 clusters asked of 10 sequences"),
])
def test_cli_refusals_come_before_the_device(args, message, tmp_path):
    """each refusal is the option check's own message: no context was asked for (on a machine without a device that would be
    the error), nothing is printed and no file is written"""
    assert os.path.exists(DAFS), "the dafs executable is built by build()"
    r = subprocess.run([DAFS] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode != 0
    assert message in r.stderr, r.stderr
    assert r.stderr.count("\n") == 1 and "HIP" not in r.stderr and "device" not in r.stderr.replace("--devices", "")
    assert r.stdout == ""
    assert os.listdir(str(tmp_path)) == []


def test_tree_line_without_recursion_is_tree_string():
    for sim, tree in _CASES:
        names = ["n%d" % i for i in range(sim.shape[0])]
        assert pipeline._tree_line(tree[0], tree[1], tree[2], names) == pipeline.tree_string(tree[0], tree[1], tree[2], names)
    n = 1500  # a chain deeper than the interpreter's recursion limit
    sim = np.full((n, n), 0.001, np.float32)
    for i in range(n - 1):
        sim[i, i + 1] = sim[i + 1, i] = 0.9
    np.fill_diagonal(sim, 1.0)
    score, left, right = capi.build_tree(sim)
    line = pipeline._tree_line(score, left, right, ["x"] * n)
    assert line.count("x") == n and line.count("[") == line.count("]") == n - 1
