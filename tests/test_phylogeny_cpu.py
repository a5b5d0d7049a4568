"""CPU tests of neighbour joining: what makes the contract neighbour joining (an additive tree comes back
exactly, splits and lengths) and its tie rule on the numpy restatement, dafs_host_nj_distances against a Python restatement,
dafs_host_newick, the library's exports, `dafs --help`, and every refusal that needs no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nj_ref
from nj_ref import nj_ref as restate
from dafs_amd import capi, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
HEADER = os.path.join(ROOT, "include", "dafs_hip.h")
RF00005 = os.path.join(ROOT, "tests", "golden", "RF00005_0.fa")  # ten sequences


@pytest.mark.parametrize("n", list(range(4, 41, 3)))
def test_an_additive_tree_comes_back_exactly(n):
    """branch lengths that are multiples of 2^-10: every sum and every half of the joins is exact, so the unrooted tree comes
    back to the bit, splits and lengths; the two branches below the root add up to the edge the last join split"""
    rng = np.random.default_rng(22000 + n)
    for _ in range(3):
        left, right, length = nj_ref.random_tree(rng, n)
        assert (length[:-1] > 0).all() and (length * 1024 == np.round(length * 1024)).all()
        dist = nj_ref.tree_distances(left, right, length)
        got = restate(dist)
        want_edges, got_edges = nj_ref.unrooted_edges(left, right, length), nj_ref.unrooted_edges(*got)
        assert set(got_edges) == set(want_edges) and len(want_edges) == 2 * n - 3  # the splits
        assert got_edges == want_edges                                             # every length, exactly
        root = 2 * n - 2
        a, b = int(got[0][root]), int(got[1][root])
        below = nj_ref.leaf_sets(got[0], got[1])
        side = below[a] if 0 not in below[a] else below[b]
        assert got[2][a] + got[2][b] == want_edges[side] and got[2][root] == 0.0
        perm = rng.permutation(n)  # the same tree under other leaf numbers
        again = restate(dist[np.ix_(perm, perm)])
        relabelled = {frozenset(int(np.flatnonzero(perm == x)[0]) for x in s): v for s, v in want_edges.items()}
        everything = frozenset(range(n))
        relabelled = {(s if 0 not in s else everything - s): v for s, v in relabelled.items()}
        assert nj_ref.unrooted_edges(*again) == relabelled


def test_the_layout_and_the_small_trees():
    left, right, length = restate(np.zeros((1, 1)))
    assert left.tolist() == [-1] and right.tolist() == [-1] and length.tolist() == [0.0]
    left, right, length = restate(np.array([[0, 0.75], [np.nan, 0]]))  # below the diagonal nothing is read
    assert left.tolist() == [-1, -1, 0] and right.tolist() == [-1, -1, 1] and length.tolist() == [0.375, 0.375, 0.0]
    # three leaves: m - 2 = 1, then the last edge.  d01 = 3, d02 = 5, d12 = 6: the branches are 1, 2 and 4
    left, right, length = restate(np.array([[0, 3.0, 5.0], [0, 0, 6.0], [0, 0, 0]]))
    assert left.tolist() == [-1, -1, -1, 0, 3] and right.tolist() == [-1, -1, -1, 1, 2]
    assert length.tolist() == [1.0, 2.0, 2.0, 2.0, 0.0]  # leaf 2's branch of 4 is split in the middle by the root


def test_the_tie_rule():
    for n in (2, 3, 4, 9):
        left, right, length = restate(np.full((n, n), 0.5))
        assert (left[n], right[n]) == (0, 1)  # all Q equal: the smallest a, then the smallest b
    d = np.full((4, 4), 1.0)  # Q(0,1) = Q(2,3) = -4, every other -2.5: the smaller row wins
    d[0, 1] = d[2, 3] = 0.25
    left, right, _ = restate(d)
    assert (left[4], right[4]) == (0, 1)
    d = np.full((5, 5), 1.0)  # Q(0,1) = Q(0,2) = Q(3,4) = -5: within the row the smaller column wins
    d[0, 1] = d[0, 2] = 0.25
    left, right, _ = restate(d)
    assert (left[5], right[5]) == (0, 1)


def test_negative_lengths_are_kept_and_refusals_raise():
    rng = np.random.default_rng(5)
    assert any((restate(rng.random((12, 12)))[2] < 0).any() for _ in range(10))
    for bad in (np.nan, np.inf, -np.inf):
        d = rng.random((5, 5))
        d[1, 3] = bad
        with pytest.raises(ValueError, match="non-finite entry"):
            restate(d)
        restate(d.T)  # the entry is below the diagonal now
    with pytest.raises(ValueError, match="written"):
        restate(np.full((4, 4), 1e308))
    restate(np.full((4, 4), 1e300))


def test_nj_distances_equal_the_python_restatement():
    rng = np.random.default_rng(6)
    n = 40
    aligned = rng.integers(0, 200, (n, n)).astype(np.uint32)
    aligned = np.maximum(aligned, aligned.T)
    ident = (aligned * rng.random((n, n))).astype(np.uint32)
    ident = np.minimum(ident, ident.T)
    # the edges: nothing aligned, nothing different, and both sides of 4 mism = 3 comp
    aligned[0, 1] = aligned[1, 0] = 0; ident[0, 1] = ident[1, 0] = 0
    aligned[2, 3] = aligned[3, 2] = 120; ident[2, 3] = ident[3, 2] = 120
    for (r, s), (comp, mism) in {(4, 5): (100, 75), (6, 7): (100, 74), (8, 9): (100, 76), (10, 11): (4, 3), (12, 13): (3, 2),
                                 (14, 15): (4000000000, 2999999999), (16, 17): (4000000000, 3000000000), (18, 19): (1, 1)}.items():
        aligned[r, s] = aligned[s, r] = comp
        ident[r, s] = ident[s, r] = comp - mism
    for model in ("jc", "p"):
        got = capi.nj_distances(ident, aligned, model)
        want = nj_ref.distances_ref(ident, aligned, model)
        assert got.dtype == np.float64 and got.tobytes() == want.tobytes(), model
        assert (np.diag(got) == 0).all()
    jc, p = capi.nj_distances(ident, aligned, "jc"), capi.nj_distances(ident, aligned, "p")
    assert jc[0, 1] == 3.0 and p[0, 1] == 1.0 and jc[2, 3] == 0.0 and p[2, 3] == 0.0
    assert jc[4, 5] == 3.0 and jc[8, 9] == 3.0 and jc[10, 11] == 3.0 and jc[12, 13] < 3.0  # the 3/4 boundary
    assert jc[6, 7] == 3.0 and -0.75 * np.log(1.0 - 296.0 / 300.0) > 3.0  # just below the boundary the logarithm is capped
    assert jc[14, 15] == 3.0 and jc[16, 17] == 3.0 and jc[18, 19] == 3.0 and p[18, 19] == 1.0  # the cap; 4 mism in 64 bits
    assert jc.max() == 3.0 and (jc * 1048576 == np.round(jc * 1048576)).all()  # quantised to 2^-20
    with pytest.raises(ValueError):
        capi.nj_distances(ident, aligned, "k80")
    with pytest.raises(ValueError):
        capi.nj_distances(ident, aligned[:-1], "jc")
    more = ident.copy()
    more[0, 1] = 7  # more identical columns than aligned ones
    with pytest.raises(ValueError, match="identical"):
        capi.nj_distances(more, aligned, "p")


def test_newick_text():
    left, right = [-1, -1, -1, 0, 3], [-1, -1, -1, 1, 2]
    length = [0.5, 1 / 3, 2, 1e-12, 0]
    assert capi.newick(["a", "b", "c"], left, right, length) == "((a:0.5,b:0.333333333):1e-12,c:2);\n"
    assert capi.newick(["a", "b", "c"], left, right) == "((a,b),c);\n"  # the topology alone
    assert capi.newick(["a", "b", "c"], left, right, [-0.25, 1e300, 123456789.125, 0.1, 9]) == "((a:-0.25,b:1e+300):0.1,c:123456789);\n"
    assert capi.newick(["only"], [-1], [-1], [0.0]) == "only;\n"
    assert capi.newick(["it's"], [-1], [-1]) == "'it''s';\n"
    quoted = ["a b", "x(y", "x)y", "x[y", "x]y", "q'r", "m:n", "s;t", "u,v", "tab\there", ""]
    n = len(quoted)
    comb_left = [-1] * n + [0] + list(range(n, 2 * n - 2))
    comb_right = [-1] * n + list(range(1, n))
    text = capi.newick(quoted, comb_left, comb_right)
    for name in quoted:
        assert "'" + name.replace("'", "''") + "'" in text
    assert capi.newick(["plain_name.1|x/y", "B-2"], [-1, -1, 0], [-1, -1, 1], [1, 2, 0]) == "(plain_name.1|x/y:1,B-2:2);\n"


def test_newick_of_a_chain_of_20000_joins_uses_no_call_stack():
    n = 20001
    names = ["s%d" % k for k in range(n)]
    left = np.concatenate([np.full(n, -1), [0], np.arange(n, 2 * n - 2)])
    right = np.concatenate([np.full(n, -1), np.arange(1, n)])
    text = capi.newick(names, left, right, np.full(2 * n - 1, 0.5))
    assert text.startswith("(" * 20000 + "s0:0.5,s1:0.5):0.5,s2:0.5)") and text.endswith(",s20000:0.5);\n") and text.count("(") == 20000
    # the right comb is as deep on the other side
    left = np.concatenate([np.full(n, -1), np.arange(1, n)])
    right = np.concatenate([np.full(n, -1), [0], np.arange(n, 2 * n - 2)])
    assert capi.newick(names, left, right).endswith("(s1,s0)" + ")" * 19999 + ";\n")


@pytest.mark.parametrize("left,right,why", [
    ([0, -1, -1, 0, 3], [-1, -1, -1, 1, 2], "a leaf with a child"),
    ([-1, -1, -1, 0, 3], [-1, -1, -1, 0, 2], "with itself"),
    ([-1, -1, -1, 0, 4], [-1, -1, -1, 1, 2], "not an earlier node"),
    ([-1, -1, -1, 0, 3], [-1, -1, -1, 1, -1], "not an earlier node"),
    ([-1, -1, -1, 0, 0], [-1, -1, -1, 1, 2], "a child twice"),
    ([-1, -1, -1, 0, 3], [-1, -1, -1, 7, 2], "not an earlier node"),
])
def test_newick_refuses_a_malformed_tree(left, right, why):
    with pytest.raises(ValueError, match=why):
        capi.newick(["a", "b", "c"], left, right)
    # the same trees are refused by the cut
    with pytest.raises(ValueError):
        capi.cluster_cut((np.zeros(5, np.float32), np.array(left), np.array(right)), count=1)


def test_newick_refuses_bad_arguments():
    with pytest.raises(ValueError):
        capi.newick(["a", "b"], [-1, -1, 0, 1, 2], [-1, -1, 1, 0, 3])
    with pytest.raises(ValueError):
        capi.newick(["a", "b"], [-1, -1, 0], [-1, -1, 1], [1.0])
    with pytest.raises(ValueError):
        capi.newick([], [], [])
    out = C.c_void_p()
    assert capi._newick(0, None, None, None, None, C.byref(out)) == -1
    assert capi._newick(2, None, None, None, None, C.byref(out)) == -1


def test_the_library_exports_and_declares_the_entry_points():
    header = open(HEADER).read()
    for name in ("dafs_hip_nj_tree", "dafs_hipk_nj_workspace", "dafs_hipk_nj", "dafs_host_nj_distances", "dafs_host_newick",
                 "dafs_host_phylogeny_refusal"):
        assert getattr(capi.lib, name) is not None
        assert re.search(r"\b%s\(" % name, header), name
    assert re.search(r"DAFS_NJ_P = 0, DAFS_NJ_JC = 1", header)
    assert capi.NJ_MODELS == ("p", "jc") and capi.NJ_MAX_ROWS == 16384 and capi.COV_TREES == ("average", "nj")
    assert capi.nj_workspace(0) == 0 and capi.nj_workspace(16385) == 0
    for n in (1, 2, 1100, 16384):
        assert capi.nj_workspace(n) >= n * n * 8 + 24 * n and capi.nj_workspace(n) % 256 == 0
    assert all(capi.phylogeny_refusal(k) for k in range(7)) and capi.phylogeny_refusal(7) == ""


def test_the_library_refuses_without_a_device():
    d, i = np.zeros(16, np.float64), np.zeros(8, np.int32)
    assert capi._nj_tree(None, 2, d.ctypes.data, i.ctypes.data, i.ctypes.data, d.ctypes.data) == -1 and b"missing argument" in capi._last_error()
    one = C.c_void_p(256)  # never dereferenced: every refusal below comes first
    for n, ptrs, why in ((1, (one,) * 5, b"2 to 16384"), (16385, (one,) * 5, b"2 to 16384"), (4, (None,) + (one,) * 4, b"missing argument"),
                         (4, (one, C.c_void_p(8)) + (one,) * 3, b"256-byte aligned")):
        assert capi.nj_launch(n, *ptrs, None) == -1
        assert why in capi._last_error(), (n, capi._last_error())
    assert capi._nj_distances(0, i.ctypes.data, i.ctypes.data, 1, d.ctypes.data) == -1
    assert capi._nj_distances(2, i.ctypes.data, i.ctypes.data, 2, d.ctypes.data) == -1 and b"unknown model" in capi._last_error()


def test_python_refuses_before_it_opens_a_context(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a context was opened")
    real_context = capi.Context
    monkeypatch.setattr(capi, "Context", no_context)
    names, seqs = ["a", "b", "c"], ["ACGUACGU", "ACGGACGU", "UUUUCCCC"]
    unknown = capi.phylogeny_refusal(capi.PHY_UNKNOWN_MODEL)
    for call in (lambda: pipeline.run(names, seqs, phylogeny="k80"), lambda: pipeline.run_batch([(names, seqs)], phylogeny="k80"),
                 lambda: pipeline.add(names[:2], seqs[:2], names[2:], seqs[2:], phylogeny="JC"),
                 lambda: pipeline.describe(names, seqs, phylogeny="k80"), lambda: pipeline.cluster(names, seqs, count=2, phylogeny="k80")):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == unknown
    with pytest.raises(ValueError) as e:
        pipeline.pairwise(names, seqs, phylogeny="jc")
    assert str(e.value) == capi.phylogeny_refusal(capi.PHY_NO_PAIRWISE)
    with pytest.raises(ValueError) as e:
        pipeline.add_each(names[:2], seqs[:2], names[2:], seqs[2:], phylogeny="jc")
    assert str(e.value) == capi.phylogeny_refusal(capi.PHY_NO_SEED_EACH)
    with pytest.raises(ValueError) as e:
        pipeline.cov_options(dict(tree="nj"))
    assert str(e.value) == capi.phylogeny_refusal(capi.PHY_COV_TREE_NEEDS_NULL)
    with pytest.raises(ValueError) as e:
        pipeline.cov_options(dict(null="tree", tree="upgma"))
    assert str(e.value) == capi.phylogeny_refusal(capi.PHY_UNKNOWN_COV_TREE)
    assert pipeline.cov_options(dict(null="tree", tree="nj"))["tree"] == "nj" and "tree" not in pipeline.cov_options(dict(null="tree"))
    with pytest.raises(AssertionError, match="a context was opened"):  # the checks passed: the next step is the context
        pipeline.run(names, seqs, phylogeny="p")
    ctx = object.__new__(real_context)  # Context.nj_tree and alignment_tree check first: no handle is touched
    ctx._h = None
    with pytest.raises(ValueError, match="n x n"):
        ctx.nj_tree(np.zeros((2, 3)))
    with pytest.raises(ValueError) as e:
        ctx.alignment_tree(["ACGU", "ACGA"], model="k80")
    assert str(e.value) == unknown


@pytest.mark.parametrize("args,which", [
    (["--phylogeny", "t.nwk", "--pairwise", RF00005], capi.PHY_NO_PAIRWISE),
    (["--seed", "s.sto", "--seed-each", "--phylogeny", "t.nwk", RF00005], capi.PHY_NO_SEED_EACH),
    (["--phylogeny-model", "jc", RF00005], capi.PHY_MODEL_NEEDS_TREE),
    (["--phylogeny", "t.nwk", "--phylogeny-model", "k80", RF00005], capi.PHY_UNKNOWN_MODEL),
    (["--phylogeny", "t.nwk", "--phylogeny-model", "JC", RF00005], capi.PHY_UNKNOWN_MODEL),
    (["--covariation", "c.tsv", "--cov-tree", "nj", RF00005], capi.PHY_COV_TREE_NEEDS_NULL),
    (["--covariation", "c.tsv", "--cov-null", "shuffle", "--cov-tree", "nj", RF00005], capi.PHY_COV_TREE_NEEDS_NULL),
    (["--covariation", "c.tsv", "--cov-null", "tree", "--cov-tree", "upgma", RF00005], capi.PHY_UNKNOWN_COV_TREE),
])
def test_cli_refuses_while_parsing(args, which, tmp_path):
    assert os.path.exists(DAFS), "the dafs executable is built by build()"
    r = subprocess.run([DAFS] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 1
    assert capi.phylogeny_refusal(which) in r.stderr, r.stderr
    assert r.stderr.count("\n") == 1 and "HIP" not in r.stderr
    assert r.stdout == ""
    assert os.listdir(str(tmp_path)) == []


def test_cli_help_names_the_options():
    r = subprocess.run([DAFS, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "--phylogeny OUT" in text and "--phylogeny-model M" in text and "--cov-tree NAME" in text
    assert text.index("--cov-null NAME") < text.index("--cov-tree NAME") < text.index("--phylogeny OUT") < text.index("Aligning options")
