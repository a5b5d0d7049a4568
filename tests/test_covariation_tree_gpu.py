"""GPU tests of the tree-aware null of the covariation statistics (dafs_hip_alignment_covariation_null,
dafs_hip_covariation_null_alignment, Context.alignment_covariation(null="tree"), Context.covariation_null_alignment,
pipeline's covariation=dict(null=...), dafs --cov-null) against the restatement in tests/covariation_tree_ref.py, bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import covariation_ref as cr
import covariation_tree_ref as tr
from dafs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = cr.NONE
FLOATS = ("best_score", "best_e", "pair_score", "pair_e")
INTS = ("col_sum", "best", "pair_rows", "pair_canonical", "pair_types")
OUTS = ("col_sum", "best", "best_score", "best_e", "pair_score", "pair_e", "pair_rows", "pair_canonical", "pair_types")
# the wavefront's edges (63, 64, 65, 130) and the edges of the permutation's 4^h (4 | 5, 16 | 17, 64 | 65, 256 | 257)
LENGTHS = (2, 3, 4, 5, 16, 17, 63, 64, 65, 130, 257)


@pytest.fixture(scope="module")
def ctx():
    from dafs_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def _same(got, want, keys=FLOATS + INTS + ("total", "g")):
    """every output equal to the bit; a NaN equals a NaN"""
    for k in keys:
        if k == "g" and ("g" not in got or "g" not in want):
            continue
        if k == "total":
            assert int(got[k]) == int(want[k])
        elif k in FLOATS:
            a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
            assert np.array_equal(np.isnan(a), np.isnan(b)), k
            assert a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes(), (k, a, b)
        else:
            assert np.asarray(got[k]).astype(np.int64).tobytes() == np.asarray(want[k]).astype(np.int64).tobytes(), k


def _case(n, length, seed):
    """12 % non-bases, one column without any base (its root set is 15), a base in every row"""
    rs = np.random.RandomState(seed)
    code = rs.randint(0, 4, (n, length)).astype(np.uint8)
    code[rs.rand(n, length) < 0.12] = 4
    code[:, length // 2] = 4
    keep = 0 if length // 2 != 0 else 1
    bare = ~(code < 4).any(1)
    code[bare, keep] = rs.randint(0, 4, int(bare.sum()))
    return code


def _ss(length, seed):
    ss = np.full(length, NONE, np.uint32)
    cols = list(np.random.RandomState(seed).permutation(length))
    for _ in range(length // 4):
        a, b = sorted((int(cols.pop()), int(cols.pop())))
        ss[a] = b
    return ss


@pytest.mark.parametrize("form", ["lds", "global"])
@pytest.mark.parametrize("n", [2, 3, 8, 33])
def test_null_alignments_equal_the_restatement(ctx, n, form, monkeypatch):
    """form: where k_cov_evolve keeps the joins' states (DAFS_COV_TREE_LDS=0: in global memory at every n)"""
    if form == "global":
        monkeypatch.setenv("DAFS_COV_TREE_LDS", "0")
    else:
        monkeypatch.delenv("DAFS_COV_TREE_LDS", raising=False)
    for length in LENGTHS:
        code = _case(n, length, 1000 * n + length)
        trees = dict(default=None, comb=tr.comb_tree(n), balanced=tr.balanced_tree(n))
        for name, tree in trees.items():
            left, right = tr.default_tree(code) if tree is None else tree
            fit = tr.fitch(code, left, right)
            for k in range(3):
                got = ctx.covariation_null_alignment(code, k, null="tree", tree=tree, seed=77)
                assert got.dtype == np.uint8 and got.tobytes() == tr.evolve(code, left, right, 77, k, fit).tobytes(), (length, name, k)
        for k in range(3):
            assert ctx.covariation_null_alignment(code, k, null="shuffle", seed=77).tobytes() == cr.shuffled(code, 77, k).tobytes(), (length, k)
    text = ["".join("ACGU-"[v] for v in row) for row in code]  # text rows give the same codes
    assert ctx.covariation_null_alignment(text, 1, null="tree", seed=77).tobytes() == tr.null_alignment(code, "tree", None, 77, 1).tobytes()


@pytest.mark.parametrize("n", [1025, 1026])
def test_last_tree_in_lds_and_first_beyond(ctx, n, monkeypatch):
    """the joins' states of 1 025 rows fill the 64 KiB of LDS a workgroup gets unasked; 1 026 rows go through global memory"""
    monkeypatch.delenv("DAFS_COV_TREE_LDS", raising=False)
    code = _case(n, 70, n)
    left, right = tr.random_tree(n, np.random.RandomState(n))
    got = ctx.covariation_null_alignment(code, 1, null="tree", tree=(left, right), seed=8)
    assert got.tobytes() == tr.evolve(code, left, right, 8, 1).tobytes()


def test_known_answer_and_edges(ctx):
    code = cr.encode("AUA AUC CGA CGC GCA G-C UAA NAC".split())
    assert " ".join("".join("ACGU-"[v] for v in r) for r in ctx.covariation_null_alignment(code, 0, null="tree", seed=12345)) == \
        "CAU AAU AAG GAG GAC C-A UAA -AA"
    one = np.array([[0, 4, 2, 3]], np.uint8)  # one row comes back as it is, under both nulls
    for null in tr.NULLS:
        assert ctx.covariation_null_alignment(one, 0, null=null).tobytes() == one.tobytes()
    col = np.array([[0], [1], [1], [4]], np.uint8)  # one column
    assert ctx.covariation_null_alignment(col, 2, null="tree", tree=tr.comb_tree(4), seed=3).tobytes() == \
        tr.evolve(col, *tr.comb_tree(4), 3, 2).tobytes()


CASES = {"8x17": lambda: (_case(8, 17, 1), _ss(17, 1)), "33x65": lambda: (_case(33, 65, 2), _ss(65, 2)), "48x100": lambda: tr.phylo(3, 6)}


@pytest.mark.parametrize("which", sorted(CASES))
def test_statistics_equal_the_restatement(ctx, which, monkeypatch):
    monkeypatch.delenv("DAFS_COV_CHUNK_WORDS", raising=False)
    code, ss = CASES[which]()
    ctx.stage_timing(True)
    ctx.stage_report()
    try:
        got = {}
        for use in (ss, None):
            got[use is None] = ctx.alignment_covariation(code, use, shuffles=5, seed=9, matrix=True, null="tree")
            _same(got[use is None], tr.restate(code, use, 5, seed=9, null="tree"))
            st = ctx.stage_report()  # the recorder knows the three kernels: one once per call, two once per null alignment
            assert st["k_cov_fitch"][2] == 1 and st["k_cov_draw"][2] == 5 and st["k_cov_evolve"][2] == 5 and "k_cov_shuffle" not in st
        tree = tr.balanced_tree(len(code))
        _same(ctx.alignment_covariation(code, ss, shuffles=5, seed=9, null="tree", tree=tree), tr.restate(code, ss, 5, seed=9, null="tree", tree=tree))
        monkeypatch.setenv("DAFS_COV_CHUNK_WORDS", "1")  # the LDS stage of the pair kernel: no bit moves
        _same(ctx.alignment_covariation(code, ss, shuffles=5, seed=9, matrix=True, null="tree"), got[False])
    finally:
        ctx.stage_timing(False)


def _old_entry(ctx, code, ss, shuffles, seed):
    """dafs_hip_alignment_covariation itself, as it was before the null could be chosen"""
    from dafs_amd import capi
    L = code.shape[1]
    out = dict(col_sum=np.zeros(L, np.int64), best=np.zeros(L, np.uint32), best_score=np.zeros(L, np.float64), best_e=np.zeros(L, np.float64),
               pair_score=np.zeros(L, np.float64), pair_e=np.zeros(L, np.float64), pair_rows=np.zeros(L, np.uint32),
               pair_canonical=np.zeros(L, np.uint32), pair_types=np.zeros(L, np.uint32))
    total, g = ctypes.c_int64(), np.zeros((L, L), np.int64)
    capi.check(capi._alignment_covariation(ctx._h, code.shape[0], L, code.ctypes.data, ss.ctypes.data, shuffles, seed,
                                           *[out[k].ctypes.data for k in OUTS], ctypes.byref(total), g.ctypes.data))
    out["total"], out["g"] = total.value, g
    return out


def test_shuffle_null_is_the_old_entry_point(ctx):
    code, ss = cr.planted_alignment()
    old = _old_entry(ctx, code, ss, 20, 12345)
    _same(ctx.alignment_covariation(code, ss, shuffles=20, seed=12345, matrix=True, null="shuffle"), old)
    _same(ctx.alignment_covariation(code, ss, shuffles=20, seed=12345, matrix=True), old)
    cr.check_planted(old, ss)
    cr.check_planted(ctx.alignment_covariation(code, ss, shuffles=20, seed=12345, null="tree"), ss)


def test_nothing_to_do_launches_nothing(ctx):
    """n < 2, len < 2 and no null alignments behave as under the shuffle null; none of the tree null's kernels runs"""
    ctx.stage_timing(True)
    ctx.stage_report()
    try:
        for code, shuffles in ((_case(1, 9, 1), 3), (np.array([[0], [1], [1], [4], [2], [0]], np.uint8), 2), (_case(8, 17, 3), 0)):
            ss = _ss(code.shape[1], 1)
            _same(ctx.alignment_covariation(code, ss, shuffles=shuffles, seed=4, matrix=True, null="tree"), cr.restate(code, ss, shuffles, seed=4))
        st = ctx.stage_report()
        assert "k_cov_fitch" not in st and "k_cov_draw" not in st and "k_cov_evolve" not in st and "k_linkage_joins" not in st
    finally:
        ctx.stage_timing(False)


def test_row_order_and_child_order(ctx):
    """Rows permuted and the tree relabelled to match: the device follows the restatement, and the gaps move with their rows.
    (The null rows of the leaves do not simply move: a leaf's branch key is made from its row index; see the CPU test.)
    Which child of a join is left and which right changes no byte."""
    n, length = 33, 65
    code = _case(n, length, 6)
    left, right = tr.random_tree(n, np.random.RandomState(3))
    perm = np.random.RandomState(4).permutation(n)
    l2, r2 = tr.relabel_tree(left, right, perm)
    for k in range(2):
        base = ctx.covariation_null_alignment(code, k, null="tree", tree=(left, right), seed=5)
        moved = ctx.covariation_null_alignment(code[perm], k, null="tree", tree=(l2, r2), seed=5)
        assert moved.tobytes() == tr.evolve(code[perm], l2, r2, 5, k).tobytes()
        assert np.array_equal(moved == 4, (base == 4)[perm])
        assert ctx.covariation_null_alignment(code, k, null="tree", tree=(right, left), seed=5).tobytes() == base.tobytes()


def test_refusals_leave_the_context_usable(ctx):
    from dafs_amd import capi
    code, ss = _case(8, 17, 1), _ss(17, 1)
    left, right = tr.comb_tree(8)
    good = ctx.alignment_covariation(code, ss, shuffles=2, matrix=True, null="tree")
    good_null = ctx.covariation_null_alignment(code, 0, null="tree")
    twice = left.copy()
    twice[9] = 1  # leaf 1 is a child of joins 8 and 9
    later = left.copy()
    later[9] = 12  # a child that is a later node
    leafy = left.copy()
    leafy[3] = 0  # a leaf with a child
    bare = code.copy()
    bare[5] = 4
    bad = [(dict(null="shuffle", tree=(left, right)), "takes no tree"), (dict(null="tree", tree=(left, None)), "both of its arrays"),
           (dict(null="tree", tree=(None, right)), "both of its arrays"), (dict(null="tree", tree=(twice, right)), "a child twice"),
           (dict(null="tree", tree=(later, right)), "not an earlier node"), (dict(null="tree", tree=(leafy, right)), "a leaf with a child"),
           (dict(null="tree", tree=(right, right)), "malformed tree")]
    for kw, msg in bad:
        with pytest.raises(capi.DafsHipError, match=msg):
            ctx.alignment_covariation(code, ss, shuffles=2, **kw)
        with pytest.raises(capi.DafsHipError, match=msg):
            ctx.covariation_null_alignment(code, 0, **kw)
    for call in (lambda: ctx.alignment_covariation(bare, ss, shuffles=2, null="tree"), lambda: ctx.covariation_null_alignment(bare, 0, null="tree")):
        with pytest.raises(capi.DafsHipError, match="a base in every row"):
            call()
    # with a tree of the caller's such a row is no obstacle
    assert ctx.covariation_null_alignment(bare, 0, null="tree", tree=(left, right)).tobytes() == tr.evolve(bare, left, right, 1, 0).tobytes()
    # a null the library does not know (Python refuses the name before it gets there)
    out = np.zeros((8, 17), np.uint8)
    assert capi._covariation_null_alignment(ctx._h, 8, 17, code.ctypes.data, 2, None, None, 1, 0, out.ctypes.data) == -1
    assert b"unknown null" in capi._last_error()
    assert capi._alignment_covariation_null(ctx._h, 8, 17, code.ctypes.data, None, 2, 1, -1, None, None, *[None] * 11) == -1
    assert b"unknown null" in capi._last_error()
    for call in (lambda: ctx.alignment_covariation(code, ss, null="star"), lambda: ctx.covariation_null_alignment(code, 0, null="star"),
                 lambda: ctx.alignment_covariation(code, ss, null="tree", tree=(left[:-1], right[:-1]))):
        with pytest.raises(ValueError):
            call()
    _same(ctx.alignment_covariation(code, ss, shuffles=2, matrix=True, null="tree"), good)
    assert ctx.covariation_null_alignment(code, 0, null="tree").tobytes() == good_null.tobytes()


def _cli(*args):
    return subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)


def test_cli_describe_and_run_equal_python(ctx, tmp_path):
    from dafs_amd import pipeline, stockholm
    code, ss = tr.phylo(3, 6)
    structure = ["."] * len(ss)
    for c in np.nonzero(ss != NONE)[0]:
        structure[c], structure[int(ss[c])] = "(", ")"
    sto = tmp_path / "x.sto"
    sto.write_text("# STOCKHOLM 1.0\n" + "".join("row%d %s\n" % (r, "".join("ACGU-"[v] for v in row)) for r, row in enumerate(code)) +
                   "#=GC SS_cons " + "".join(structure) + "\n//\n")
    tsv = tmp_path / "cov.tsv"
    r = _cli("--describe", sto, "--covariation", tsv, "--cov-shuffles", "20", "--cov-null", "tree")
    assert r.returncode == 0 and r.stdout == "", r.stderr
    got = stockholm.read_seed_structure(str(sto))
    assert got[2].tobytes() == ss.tobytes()
    d = pipeline.describe(*got, ctx=ctx, identity=False, covariation=dict(shuffles=20, null="tree"))
    _same(d.covariation, tr.restate(code, ss, 20, seed=1, null="tree", matrix=False))
    assert tsv.read_text() == pipeline.covariation_tsv(d) and tsv.read_text().count("\tss\t") == 6
    other = pipeline.describe(*got, ctx=ctx, identity=False, covariation=dict(shuffles=20))
    assert d.covariation["best_e"].tobytes() != other.covariation["best_e"].tobytes()  # the null was the one asked for
    # a run: the table and the cov_SS_cons line come from the chosen null; stdout does not change
    recs = synth.family_set(5, 70, seed=75)
    fam, out_sto = tmp_path / "fam.fa", tmp_path / "fam.sto"
    fam.write_text(synth.to_fasta(recs))
    plain = _cli(fam)
    r = _cli("--covariation", tsv, "--cov-shuffles", "10", "--cov-seed", "3", "--cov-null", "tree", "--stockholm", out_sto, fam)
    assert r.returncode == 0 and r.stdout == plain.stdout, r.stderr
    res = pipeline.run([x[0] for x in recs], [x[1] for x in recs], ctx=ctx, reliability=True, covariation=dict(shuffles=10, seed=3, null="tree"))
    assert res.output == r.stdout and tsv.read_text() == pipeline.covariation_tsv(res) and out_sto.read_text() == res.stockholm
    _same(res.covariation, tr.restate(cr.encode(res.rows), res.ss, 10, seed=3, null="tree", matrix=False))
    # without --covariation the option is refused while parsing
    r = _cli("--cov-null", "tree", fam)
    assert r.returncode != 0 and "--cov-null needs --covariation" in r.stderr and r.stdout == ""
