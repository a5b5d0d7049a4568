"""CPU tests of the bootstrap support: the known draws, dafs_host_tree_support against the restatement
(bootstrap_ref.py), dafs_host_newick_support and dafs_host_support_table byte for byte, the refusal texts, and, on the
restatement alone, what the support is for: the splits of a tree that the rows really evolved along are supported, the
splits of a tree of unrelated rows are not."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bootstrap_ref as br
import nj_ref
from dafs_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_known_draws():
    assert br.mix(1) == 0x5692161D100B05E5
    assert br.draws(12345, 0, 8) == [2, 6, 6, 4, 0, 4, 2, 0]
    assert br.draws(12345, 1, 8) == [2, 4, 6, 6, 0, 3, 5, 7]
    assert br.draws(0, 0, 10) == [2, 9, 6, 4, 2, 1, 5, 5, 5, 3]
    for seed, k in ((0, 0), (12345, 7), ((1 << 64) - 1, 65535)):
        assert br.draws(seed, k, 1) == [0]
    # a replicate is the used columns in the drawn order
    cell = np.arange(3 * 10, dtype=np.uint8).reshape(3, 10) % 6
    use = np.array([1, 0, 1, 1, 0, 1, 1, 1, 0, 1], np.uint8)
    cols = [0, 2, 3, 5, 6, 7, 9]
    assert br.used_columns(10, use) == cols
    got = br.replicate_cells(cell, use, 12345, 0)
    assert got.shape == (3, 7) and (got == cell[:, [cols[j] for j in br.draws(12345, 0, 7)]]).all()


def rerooted(left, right, above, rng):
    """the same unrooted tree with its root on the edge above node `above`, children swapped at random, in build_tree's
    layout (children precede their join)"""
    n = (len(left) + 1) // 2
    root = 2 * n - 2
    nb = {v: [] for v in range(root)}  # the unrooted tree: the root is taken out of its edge
    for v in range(n, root):
        for c in (int(left[v]), int(right[v])):
            nb[v].append(c)
            nb[c].append(v)
    a, b = int(left[root]), int(right[root])
    nb[a].append(b)
    nb[b].append(a)
    parent = [-1] * (2 * n - 1)
    for v in range(n, 2 * n - 1):
        parent[int(left[v])] = parent[int(right[v])] = v
    other = parent[above] if parent[above] != root else (b if above == a else a)  # the neighbour across the edge above `above`
    new_left, new_right = [-1] * n, [-1] * n

    def build(v, come_from):  # returns the new index of the subtree at v seen from come_from
        if v < n:
            return v
        kids = [build(x, v) for x in nb[v] if x != come_from]
        assert len(kids) == 2
        if rng.random() < 0.5:
            kids.reverse()
        new_left.append(kids[0])
        new_right.append(kids[1])
        return len(new_left) - 1

    kids = [build(above, other), build(other, above)]
    if rng.random() < 0.5:
        kids.reverse()
    new_left.append(kids[0])
    new_right.append(kids[1])
    return np.array(new_left, np.int64), np.array(new_right, np.int64)


@pytest.mark.parametrize("n", list(range(4, 41, 4)))
def test_tree_support_equals_the_restatement(n):
    rng = np.random.default_rng(23000 + n)
    left, right, _ = nj_ref.random_tree(rng, n)
    # B copies of itself, re-rooted and with children swapped: every non-trivial split is in every copy
    B = 5
    copies = [rerooted(left, right, int(rng.integers(0, 2 * n - 2)), rng) for _ in range(B)]
    for cl, cr in copies:
        assert set(br.sides(cl, cr)) == set(br.sides(left, right))  # the helper keeps the unrooted tree
    got = capi.tree_support(left, right, [c[0] for c in copies], [c[1] for c in copies])
    want = br.support_ref(left, right, [c[0] for c in copies], [c[1] for c in copies])
    assert got.dtype == np.int64 and (got == want).all()
    assert set(got.tolist()) <= {-1, B} and (got == B).sum() >= n - 3  # n - 3 splits; the root's is on both its children
    assert got[2 * n - 2] == -1 and (got[:n] == -1).all()
    a, b = int(left[-1]), int(right[-1])
    assert got[a] == got[b]
    # random other trees: exactly the restatement's counts
    others = [nj_ref.random_tree(rng, n) for _ in range(6)] + [(left, right, None)]
    got = capi.tree_support(left, right, [o[0] for o in others], [o[1] for o in others])
    want = br.support_ref(left, right, [o[0] for o in others], [o[1] for o in others])
    assert (got == want).all() and got.max() >= 1


def test_tree_support_of_small_trees_and_refusals():
    for n in (1, 2, 3):
        left, right, _ = nj_ref.random_tree(np.random.default_rng(n), n) if n > 1 else (np.array([-1]), np.array([-1]), None)
        got = capi.tree_support(left, right, [left] * 4, [right] * 4)
        assert got.tolist() == [-1] * (2 * n - 1)
    left, right, _ = nj_ref.random_tree(np.random.default_rng(5), 5)
    assert capi.tree_support(left, right, np.zeros((0, 9), np.int32), np.zeros((0, 9), np.int32)).max() == 0  # no replicate: nothing counted
    bad = left.copy()
    bad[6] = 6
    with pytest.raises(ValueError, match="malformed tree"):
        capi.tree_support(bad, right, [left], [right])
    with pytest.raises(ValueError, match="replicate 1: malformed tree"):
        capi.tree_support(left, right, [left, bad], [right, right])


def test_a_caterpillar_of_20000_leaves():
    """((((0,1),2),3),...): a chain as deep as the tree has leaves; the walk keeps its own stack"""
    n = 20000
    left = np.full(2 * n - 1, -1, np.int64)
    right = np.full(2 * n - 1, -1, np.int64)
    left[n] = 0
    right[n] = 1
    for t in range(1, n - 1):
        left[n + t] = n + t - 1
        right[n + t] = t + 1
    # the same chain with the children of every join swapped, and a chain over the reversed leaves (the same unrooted tree)
    rev_left, rev_right = left.copy(), right.copy()
    rev_left[n], rev_right[n] = n - 1, n - 2
    rev_right[n + 1:] = np.arange(n - 3, -1, -1)
    got = capi.tree_support(left, right, [right, rev_left], [left, rev_right])
    assert got[n] == 2 and got[2 * n - 2] == -1 and got[2 * n - 3] == -1  # the last join splits off one leaf
    assert (got[n:2 * n - 3] == 2).all() and (got[:n] == -1).all()
    text = capi.newick(["s%d" % k for k in range(n)], left, right, None, support=got, replicates=2)
    assert text.startswith("(" * (n - 1) + "s0,s1)100,s2)100,") and text.endswith(")100,s%d),s%d);\n" % (n - 2, n - 1))


FIVE = (np.array([-1, -1, -1, -1, -1, 0, 2, 5, 7]), np.array([-1, -1, -1, -1, -1, 1, 3, 6, 4]))  # (((A,B),(C,D)),E)
NAMES = ["A", "B", "C", "D", "E"]
LENGTHS = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.05, 0.06, 0.07, 0.0])


def test_newick_support():
    left, right = FIVE
    none = np.full(9, -1)
    assert capi.newick(NAMES, left, right, LENGTHS, support=none, replicates=10) == capi.newick(NAMES, left, right, LENGTHS)
    assert capi.newick(NAMES, left, right, None, support=none, replicates=10) == capi.newick(NAMES, left, right)
    # node 7 = ((A,B),(C,D)) is a root child and a join: it shows the root split {E | rest}; here that split is trivial
    support = np.array([-1, -1, -1, -1, -1, 87, 40, -1, -1])
    assert capi.newick(NAMES, left, right, LENGTHS, support=support, replicates=100) == "(((A:0.1,B:0.2)87:0.05,(C:0.3,D:0.4)40:0.06):0.07,E:0.5);\n"
    assert capi.newick(NAMES, left, right, None, support=support, replicates=100) == "(((A,B)87,(C,D)40),E);\n"
    # the rounding: 1/3 -> 33, 2/3 -> 67; 1 of 200 is 0.5 % and rounds up
    assert capi.newick(NAMES, left, right, None, support=np.array([-1] * 5 + [1, 2, -1, -1]), replicates=3) == "(((A,B)33,(C,D)67),E);\n"
    assert capi.newick(NAMES, left, right, None, support=np.array([-1] * 5 + [1, 0, -1, -1]), replicates=200) == "(((A,B)1,(C,D)0),E);\n"
    assert capi.newick(NAMES, left, right, None, support=np.array([-1] * 5 + [3, 3, -1, -1]), replicates=3) == "(((A,B)100,(C,D)100),E);\n"
    # the root-child rule: ((A,B),((C,D),E)): both root children are joins and carry one split; the left one shows it
    left2, right2 = np.array([-1] * 5 + [0, 2, 6, 5]), np.array([-1] * 5 + [1, 3, 4, 7])
    support2 = np.array([-1] * 5 + [9, 5, 9, -1])
    assert capi.newick(NAMES, left2, right2, None, support=support2, replicates=10) == "((A,B)90,((C,D)50,E));\n"
    # the left root child a leaf: the right one shows what it has
    left3, right3 = np.array([-1] * 5 + [0, 2, 6, 4]), np.array([-1] * 5 + [1, 3, 5, 7])  # (E,((C,D),(A,B)))
    support3 = np.array([-1] * 5 + [9, 5, 7, -1])
    assert capi.newick(NAMES, left3, right3, None, support=support3, replicates=10) == "(E,((C,D)50,(A,B)90)70);\n"
    # both root children leaves: nothing to label
    assert capi.newick(["A", "B"], [-1, -1, 0], [-1, -1, 1], None, support=[-1, -1, -1], replicates=4) == "(A,B);\n"
    # the restatement writes the same text
    for lft, rgt, sup, B in ((left, right, support, 100), (left2, right2, support2, 10), (left3, right3, support3, 10)):
        assert br.newick_ref(NAMES, lft, rgt, LENGTHS, sup, B) == capi.newick(NAMES, lft, rgt, LENGTHS, support=sup, replicates=B)
    with pytest.raises(ValueError, match="replicates"):
        capi.newick(NAMES, left, right, None, support=support, replicates=0)
    with pytest.raises(ValueError, match="above the number of replicates"):
        capi.newick(NAMES, left, right, None, support=support, replicates=50)


def test_support_table():
    rng = np.random.default_rng(7)
    for n in (4, 5, 9, 17):
        left, right, _ = nj_ref.random_tree(rng, n)
        others = [nj_ref.random_tree(rng, n) for _ in range(3)] + [(left, right)]
        support = br.support_ref(left, right, [o[0] for o in others], [o[1] for o in others])
        names = ["row%d" % k for k in range(n)]
        got = capi.support_table(names, left, right, support, 4, seed=2 ** 63 + 5, model="p")
        assert got == br.table_ref(names, left, right, support, 4, 2 ** 63 + 5, "p")
        lines = got.splitlines()
        assert lines[0] == "# rows %d replicates 4 seed %d model p" % (n, 2 ** 63 + 5) and len(lines) == 1 + n - 3
        assert all("row0" not in ln.split("\t")[5].split(",") for ln in lines[1:])
    left, right = FIVE
    assert capi.support_table(NAMES, left, right, [-1] * 5 + [87, 40, -1, -1], 100) == (
        "# rows 5 replicates 100 seed 12345 model jc\n6\t87\t100\t87\t3\tC,D,E\n7\t40\t100\t40\t2\tC,D\n")


def test_the_refusal_texts_and_their_numbers():
    """the refusals of the phylogeny options keep their numbers and their count; the bootstrap's have a function of their own"""
    old = {0: "--pairwise", 1: "--seed-each", 2: "16384 rows", 3: "--phylogeny-model needs", 4: "is jc or p", 5: "--cov-null tree", 6: "average or nj"}
    for which, part in old.items():
        assert part in capi.phylogeny_refusal(which)
    assert (capi.PHY_NO_PAIRWISE, capi.PHY_UNKNOWN_COV_TREE) == (0, 6) and capi.phylogeny_refusal(7) == ""
    assert (capi.BOOT_NEEDS_TREE, capi.BOOT_COUNT, capi.BOOT_NEEDS_REPLICATES, capi.BOOT_NO_COLUMN) == (0, 1, 2, 3)
    assert capi.bootstrap_refusal(capi.BOOT_NEEDS_TREE).startswith("--phylogeny-bootstrap, --phylogeny-seed and --phylogeny-support")
    assert "need --phylogeny" in capi.bootstrap_refusal(capi.BOOT_NEEDS_TREE)
    assert "1 to 65536" in capi.bootstrap_refusal(capi.BOOT_COUNT)
    assert "--phylogeny-bootstrap" in capi.bootstrap_refusal(capi.BOOT_NEEDS_REPLICATES)
    assert "one used column" in capi.bootstrap_refusal(capi.BOOT_NO_COLUMN)
    assert capi.bootstrap_refusal(4) == "" and capi.bootstrap_refusal(-1) == ""
    header = open(os.path.join(ROOT, "include", "dafs_hip.h")).read()
    for name in ("dafs_hip_nj_trees", "dafs_hipk_nj_batch", "dafs_hipk_nj_batch_workspace", "dafs_hip_alignment_bootstrap",
                 "dafs_hip_bootstrap_alignment", "dafs_host_tree_support", "dafs_host_newick_support", "dafs_host_support_table",
                 "dafs_host_bootstrap_refusal"):
        assert name + "(" in header and hasattr(C.CDLL(os.path.join(ROOT, "dafs_amd", "libdafs_hip.so")), name)
    assert capi.nj_batch_workspace(1, 3) == 0 and capi.nj_batch_workspace(5, 0) == 0 and capi.nj_batch_workspace(5, 3) % 256 == 0


# ---- what it is for, on the restatement alone ----
def balanced_alignment(rng, columns=300, p_internal=0.15, p_leaf=0.05):
    """16 rows evolved down a balanced binary tree of depth 4: every cell is redrawn (uniformly from ACGU) with probability
    p_internal on a branch to an internal node and p_leaf on a branch to a leaf"""
    level = [rng.integers(0, 4, columns)]
    for depth in range(1, 5):
        p = p_leaf if depth == 4 else p_internal
        nxt = []
        for seq in level:
            for _ in range(2):
                redraw = rng.random(columns) < p
                nxt.append(np.where(redraw, rng.integers(0, 4, columns), seq))
        level = nxt
    return np.array(level, np.uint8)


def supported(cell, B=50, seed=12345, at_least=45):
    ident, aligned = br.counts(cell)
    tree = nj_ref.nj_ref(nj_ref.distances_ref(ident, aligned, "jc"))
    support, _, _ = br.bootstrap_ref(cell, None, "jc", B, seed, tree)
    shown = support >= 0
    silent = br.silent_root_child(tree[0], tree[1])
    if silent is not None:  # the root split stands on both root children: it counts once
        shown[silent] = False
    values = support[shown]
    assert len(values) == 13
    return int((values >= at_least).sum()), values


@pytest.mark.parametrize("seed", [0, 1])
def test_support_tells_an_evolved_set_from_a_random_one(seed):
    rng = np.random.default_rng(seed)
    high, values = supported(balanced_alignment(rng))
    print("evolved set, seed %d: %d of 13 splits reach 45 of 50; the values %s" % (seed, high, sorted(values.tolist())))
    assert high >= 11
    high, values = supported(rng.integers(0, 4, (16, 300)).astype(np.uint8))
    print("random set, seed %d: %d of 13 splits reach 45 of 50; the values %s" % (seed, high, sorted(values.tolist())))
    assert high <= 2


# ---- memory safety of the host entry points ----
def _runs_clean_under_sanitizers(tmp_path, main, with_sources):
    """tests/<main>.cpp and the named files of dafs_amd/csrc as a program of its own built with -fsanitize=address,undefined:
    exit status 0, nothing on stderr"""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    flags = ["-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no usable address / undefined-behaviour sanitizer runtime: " + r.stderr.strip()[-200:])
    srcs = [os.path.join(ROOT, "tests", main + ".cpp")] + [os.path.join(ROOT, "dafs_amd", "csrc", s) for s in with_sources]
    exe = str(tmp_path / main)
    r = subprocess.run([cxx] + flags + ["-Wall"] + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.stdout, r.stderr)


def test_host_support_under_sanitizers(tmp_path):
    """tests/host_support_main.cpp calls dafs_host_tree_support, dafs_host_newick_support and dafs_host_support_table, the
    refusals included"""
    _runs_clean_under_sanitizers(tmp_path, "host_support_main", ["host_text.cpp", "host_tree.cpp"])


def test_host_call_helpers_under_sanitizers(tmp_path):
    """tests/host_call_main.cpp checks what dafs_amd/csrc/call_host.h gives the per-call entry points, compiled without a ROCm
    include path: the offset carver, the knob readers, the structure check, and the distance of a pair of rows against
    dafs_host_nj_distances to the bit"""
    _runs_clean_under_sanitizers(tmp_path, "host_call_main", ["host_tree.cpp"])


def test_python_refuses_before_it_opens_a_context(monkeypatch):
    from dafs_amd import pipeline

    def no_context(*a, **k):
        raise AssertionError("a context was opened")
    monkeypatch.setattr(capi, "Context", no_context)
    names, seqs = ["a", "b", "c"], ["ACGUACGU", "ACGGACGU", "UUUUCCCC"]
    needs_tree, count = capi.bootstrap_refusal(capi.BOOT_NEEDS_TREE), capi.bootstrap_refusal(capi.BOOT_COUNT)
    for call in (lambda **kw: pipeline.run(names, seqs, **kw), lambda **kw: pipeline.run_batch([(names, seqs)], **kw),
                 lambda **kw: pipeline.add(names[:2], seqs[:2], names[2:], seqs[2:], **kw), lambda **kw: pipeline.describe(names, seqs, **kw),
                 lambda **kw: pipeline.cluster(names, seqs, count=2, **kw)):
        with pytest.raises(ValueError) as e:
            call(phylogeny_bootstrap=10)
        assert str(e.value) == needs_tree
        with pytest.raises(ValueError) as e:
            call(phylogeny="jc", phylogeny_bootstrap=65537)
        assert str(e.value) == count
    for call in (lambda **kw: pipeline.pairwise(names, seqs, **kw), lambda **kw: pipeline.add_each(names[:2], seqs[:2], names[2:], seqs[2:], **kw)):
        with pytest.raises(ValueError):
            call(phylogeny_bootstrap=10)
    opt = pipeline.phylogeny_option("p", 5, 2 ** 64 + 3)
    assert opt == "p" and (opt.bootstrap, opt.seed) == (5, 3) and pipeline.phylogeny_option(opt) is opt and pipeline.phylogeny_model(opt) is opt
    assert pipeline.phylogeny_option(False) is None and pipeline.phylogeny_option(True) == "jc" and pipeline.phylogeny_option(True).bootstrap == 0


def test_the_command_line_knows_the_options():
    dafs = os.path.join(ROOT, "dafs_amd", "dafs")
    text = subprocess.run([dafs, "--help"], capture_output=True, text=True).stdout
    for option in ("--phylogeny-bootstrap B", "--phylogeny-seed S", "--phylogeny-support OUT"):
        assert option in text
    r = subprocess.run([dafs, "--phylogeny-bootstrap", "5", os.path.join(ROOT, "tests", "golden", "RF00005_0.fa")], capture_output=True, text=True)
    assert r.returncode != 0 and r.stdout == "" and capi.bootstrap_refusal(capi.BOOT_NEEDS_TREE) in r.stderr
