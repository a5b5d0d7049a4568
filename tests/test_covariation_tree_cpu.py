"""CPU tests of the tree-aware null of the covariation statistics: the restatement (tests/covariation_tree_ref.py) against the
known answers of DESIGN.md section 13, the properties the contract claims (the permutation, Fitch's score, what a null
alignment keeps), what the null is for (related rows, independent columns), the options and the command line's refusals."""
import os
import subprocess

import numpy as np
import pytest

import covariation_ref as cr
import covariation_tree_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = cr.NONE
EIGHT = "AUA AUC CGA CGC GCA G-C UAA NAC".split()


def _text(code):
    return " ".join("".join("ACGU-"[v] for v in row) for row in code)


def test_permutation_known_answers():
    assert [tr.pi(cr.mix(1), 10, c) for c in range(10)] == [8, 3, 0, 6, 1, 4, 7, 5, 9, 2]
    assert [tr.pi(cr.mix(2), 17, c) for c in range(17)] == [16, 1, 14, 0, 9, 13, 10, 8, 5, 7, 12, 4, 2, 15, 3, 11, 6]
    assert [tr.pi(cr.mix(3), 2, c) for c in range(2)] == [1, 0]
    for key in (0, 1, cr.mix(9), 2 ** 64 - 1):
        assert tr.pi(key, 1, 0) == 0
    assert [tr.halfbits(n) for n in (1, 2, 4, 5, 16, 17, 64, 65, 256, 257, 1024, 1025)] == [1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6]


@pytest.mark.parametrize("key", [0, 1, cr.mix(5), 2 ** 64 - 1, 0x0123456789ABCDEF])
def test_permutation_is_one_and_both_forms_agree(key):
    for length in list(range(1, 71)) + [256, 257, 1025]:
        vec = tr.pi_all(key, length)
        assert sorted(vec.tolist()) == list(range(length)), length
        if length <= 70 or length == 257:
            assert [tr.pi(key, length, c) for c in range(length)] == vec.tolist(), length
        # the walk's bound: no column needs more than 4^h - length + 1 applications of F
        h = tr.halfbits(length)
        for c in (0, length // 2, length - 1):
            x, steps = tr.feistel(key, h, c), 1
            while x >= length:
                x, steps = tr.feistel(key, h, x), steps + 1
            assert steps <= 4 ** h - length + 1


def test_eight_rows_known_answers():
    code = cr.encode(EIGHT)
    assert float(tr.similarity(code)[0, 1]) == 0.6666666865348816
    left, right = tr.default_tree(code)
    assert left.tolist() == [-1] * 8 + [5, 0, 2, 4, 9, 12, 13] and right.tolist() == [-1] * 8 + [7, 1, 3, 6, 8, 10, 11]
    _, state, chg = tr.fitch(code, left, right)
    assert state[-1].tolist() == [2, 0, 0] and (chg != 0).sum(0).tolist() == [3, 3, 3]
    assert chg.tolist() == [[0, 0, 5], [0, 0, 0], [0, 0, 5], [0, 0, 0], [0, 2, 0], [0, 0, 0], [12, 0, 0], [0, 0, 0], [0, 0, 0], [9, 4, 0],
                            [10, 3, 0], [0, 0, 0], [0, 0, 0], [0, 0, 2], [0, 0, 0]]
    assert _text(tr.null_alignment(code, "tree", None, 12345, 0)) == "CAU AAU AAG GAG GAC C-A UAA -AA"
    assert _text(tr.null_alignment(code, "tree", None, 12345, 1)) == "CUA AUA CAC CGC GCA C-A UAA -AA"
    assert np.array_equal(tr.null_alignment(code, "shuffle", None, 12345, 0), cr.shuffled(code, 12345, 0))


def _random_case(n, length, seed):
    rs = np.random.RandomState(seed)
    code = rs.randint(0, 4, (n, length)).astype(np.uint8)
    code[rs.rand(n, length) < 0.12] = 4
    code[:, length // 2] = 4  # a column without a base: every set is 15, the root's state 0, no change
    return code, tr.random_tree(n, rs)


@pytest.mark.parametrize("n", list(range(2, 34)))
def test_what_fitch_and_a_null_alignment_keep(n):
    length = 23 + n
    code, (left, right) = _random_case(n, length, 100 + n)
    parent = tr.check_tree(n, left, right)
    sets, state, chg = tr.fitch(code, left, right)
    # the changes of a column are its parsimony score, and the scalar form says the same
    assert ((chg != 0).sum(0) == tr.parsimony(code, left, right)).all()
    for c in (0, length // 2, length - 1):
        s1, st1, ch1 = tr.fitch_column(code[:, c], left, right, parent)
        assert (s1, st1, ch1) == (sets[:, c].tolist(), state[:, c].tolist(), chg[:, c].tolist())
    assert not chg[:, length // 2].any() and not chg[-1].any()
    # a leaf without a base takes its parent's state
    gap = np.nonzero(code == 4)
    assert (state[gap[0], gap[1]] == state[parent[gap[0]], gap[1]]).all()
    for k in range(3):
        ns = tr.evolve(code, left, right, 7, k, nodes=True)
        null = tr.evolve(code, left, right, 7, k)
        assert np.array_equal(null == 4, code == 4)
        assert np.array_equal(null[code != 4], ns[:n][code != 4]) and ns.max() <= 3
        for v in range(2 * n - 2):  # every branch changes in as many columns as in the real alignment
            assert int((ns[v] != ns[parent[v]]).sum()) == int((chg[v] != 0).sum()), (k, v)
        assert np.array_equal(ns[-1], state[-1])
    assert not np.array_equal(tr.evolve(code, left, right, 7, 0), tr.evolve(code, left, right, 7, 1))


def test_trees_of_the_tests_are_trees():
    for n in (2, 3, 8, 33):
        for left, right in (tr.comb_tree(n), tr.balanced_tree(n), tr.random_tree(n, np.random.RandomState(n))):
            parent = tr.check_tree(n, left, right)
            assert (parent[:-1] > np.arange(2 * n - 2)).all() and parent[-1] == -1
    left, right = tr.comb_tree(4)
    for bad_left, bad_right in ((left[:-1], right[:-1]), (np.where(left == 4, 5, left), right), (np.where(left == 4, 1, left), right)):
        with pytest.raises(AssertionError):
            tr.check_tree(4, bad_left, bad_right)
    with pytest.raises(AssertionError, match="without a base"):
        tr.default_tree(np.array([[0, 1], [4, 4], [2, 2]], np.uint8))


def test_row_order_and_child_order():
    """What a permutation of the rows (with the tree relabelled to match) moves.  Fitch's records move with the rows and the
    joins' null states stay where they are; the null row of a leaf does NOT simply move: key_v of a leaf's branch is made
    from its row index, so the branch draws other columns (as many of them).  Which child of a join is called left and which
    right changes nothing at all."""
    code, (left, right) = _random_case(9, 40, 5)
    n = 9
    perm = np.random.RandomState(2).permutation(n)
    l2, r2 = tr.relabel_tree(left, right, perm)
    parent, parent2 = tr.check_tree(n, left, right), tr.check_tree(n, l2, r2)
    _, state, chg = tr.fitch(code, left, right)
    _, state2, chg2 = tr.fitch(code[perm], l2, r2)
    assert np.array_equal(chg2[:n], chg[perm]) and np.array_equal(chg2[n:], chg[n:]) and np.array_equal(state2[n:], state[n:])
    for k in range(2):
        ns, ns2 = tr.evolve(code, left, right, 3, k, nodes=True), tr.evolve(code[perm], l2, r2, 3, k, nodes=True)
        assert np.array_equal(ns2[n:], ns[n:])
        for i in range(n):
            assert int((ns2[i] != ns2[parent2[i]]).sum()) == int((ns[perm[i]] != ns[parent[perm[i]]]).sum())
        assert np.array_equal(tr.evolve(code[perm], l2, r2, 3, k) == 4, (code == 4)[perm])
        swap = np.arange(2 * n - 1) % 2 == 0
        assert np.array_equal(tr.evolve(code, np.where(swap, right, left), np.where(swap, left, right), 3, k), tr.evolve(code, left, right, 3, k))


@pytest.fixture(scope="module")
def phylo_flags():
    """per (seed, planted): the columns with best_e <= 0.05 under each null, and pair_e of the planted pairs"""
    out = {}
    for seed in (3, 5, 7, 11):
        for planted in (0, 6):
            code, ss = tr.phylo(seed, planted)
            per = {}
            for null in tr.NULLS:
                r = tr.restate(code, ss, 100, 1, null=null, matrix=False)
                per[null] = (set(np.nonzero(r["best_e"] <= 0.05)[0].tolist()), r["pair_e"][ss != NONE])
            out[seed, planted] = per
    return out


@pytest.mark.parametrize("seed", [3, 5, 7, 11])
def test_related_rows_with_independent_columns(phylo_flags, seed):
    """The reason the tree null exists: 48 rows in four deep clades, no column coupled to another.  The shuffle null flags a
    large part of the columns, the tree null next to none; with six planted pairs both find all twelve columns and the tree
    null next to nothing else.  (Measured with this restatement: 39, 66, 44, 42 columns against 0; 12 of 12 and 0 others.)"""
    free, six = phylo_flags[seed, 0], phylo_flags[seed, 6]
    planted = set(range(5, 11)) | set(range(55, 61))
    print("seed", seed, "unplanted: shuffle", len(free["shuffle"][0]), "tree", len(free["tree"][0]),
          "| planted: shuffle others", len(six["shuffle"][0] - planted), "tree others", len(six["tree"][0] - planted))
    assert len(free["shuffle"][0]) >= 20
    assert len(free["tree"][0]) <= 2
    assert planted <= six["shuffle"][0] and planted <= six["tree"][0]
    assert len(six["tree"][0] - planted) <= 2
    assert (six["tree"][1] <= 0.05).all()


def test_planted_star_alignment_under_the_tree_null():
    code, ss = cr.planted_alignment()
    cr.check_planted(tr.restate(code, ss, 20, 12345, null="tree", matrix=False), ss)


def test_covariation_options_take_a_null():
    from dafs_amd import capi, pipeline
    assert capi.COV_NULLS == ("shuffle", "tree")
    assert pipeline.cov_options(dict(null="tree")) == dict(shuffles=100, seed=1, e_max=0.05, null="tree")
    assert pipeline.cov_options(dict(null="shuffle", shuffles=3))["null"] == "shuffle"
    assert "null" not in pipeline.cov_options(True)
    with pytest.raises(ValueError, match="null"):
        pipeline.cov_options(dict(null="star"))


def _cli(*args):
    return subprocess.run([DAFS] + list(args), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args, msg", [
    (["--cov-null", "tree"], "--cov-null needs --covariation"), (["--cov-null", "shuffle"], "--cov-null needs --covariation"),
    (["--covariation", "OUT", "--cov-null", "star"], "unknown null 'star'"), (["--covariation", "OUT", "--cov-null", ""], "unknown null"),
    (["--pairwise", "--covariation", "OUT", "--cov-null", "tree"], "--pairwise")])
def test_cli_refusals_happen_while_parsing(tmp_path, args, msg):
    out = str(tmp_path / "cov.tsv")
    r = _cli(*[out if a == "OUT" else a for a in args], os.path.join(G, "RF00005_0.fa"))
    assert r.returncode != 0 and msg in r.stderr and r.stdout == ""
    assert not os.path.exists(out)


def test_cli_help_names_the_option():
    r = _cli("--help")
    assert r.returncode == 0 and "--cov-null NAME" in r.stdout


def test_symbols_are_exported_and_declared():
    from dafs_amd import capi
    header = open(os.path.join(ROOT, "include", "dafs_hip.h")).read()
    for name in ("dafs_hip_alignment_covariation_null", "dafs_hip_covariation_null_alignment"):
        assert hasattr(capi.lib, name) and name + "(" in header
    assert "DAFS_COV_NULL_SHUFFLE = 0, DAFS_COV_NULL_TREE = 1" in header
