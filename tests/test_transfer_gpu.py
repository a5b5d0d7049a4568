"""GPU tests of the transfer bootstrap.  Every comparison is equality of integer arrays with the numpy
restatement (transfer_ref.py, brute force over boolean side matrices), never a tolerance: dafs_hip_tree_transfer per replicate
and in the sum at the sizes where a rank indexes the edge of a word, in chunks of one tree, with the main tree among the
replicates and with a caterpillar as the main tree; dafs_hip_alignment_bootstrap_transfer beside the call without the sums, in
both forms of the joins; the L0 launch on torch tensors and a torch stream; the degenerate sizes, the refusals, and both
drivers byte for byte.

The restatement's side matrices are the slow side, so the replicate trees and their indices are computed once per size and
shared: B = 1 is a prefix of B = 7."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import bootstrap_ref as br
import nj_ref
import transfer_ref as tr
from nj_ref import nj_ref as restate
from dafs_amd import capi
from test_bootstrap_gpu import alignment

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [4, 5, 63, 64, 65, 128, 129]  # 64 and 128: rank(u, n) names the word behind the last one


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def trees(n, kind="random"):
    """(main, rep_left [7, 2n-1], rep_right): random trees; "member": the main tree is replicate 3; "caterpillar": the main tree
    is the chain over the leaves in a shuffled order, which has a side of every size"""
    rng = np.random.default_rng(2800 + n)
    reps = [nj_ref.random_tree(rng, n)[:2] for _ in range(7)]
    main = nj_ref.random_tree(rng, n)[:2]
    if kind == "member":
        reps[3] = main
    if kind == "caterpillar":
        main = tr.caterpillar(n, rng.permutation(n))
        reps[5] = tr.caterpillar(n, rng.permutation(n))
    return main, np.array([r[0] for r in reps]), np.array([r[1] for r in reps])


@functools.lru_cache(maxsize=None)
def reference(n, kind="random"):
    """phi [7, 2n-1] of the restatement; computed once and shared"""
    main, rep_left, rep_right = trees(n, kind)
    phi = tr.transfer_each_ref(main[0], main[1], rep_left, rep_right)
    phi.setflags(write=False)
    return phi


def check_tree_transfer(ctx, n, B, kind="random"):
    main, rep_left, rep_right = trees(n, kind)
    phi = reference(n, kind)[:B]
    want = np.where(tr.depths(*main) >= 0, phi.sum(0), -1)
    got, each = ctx.tree_transfer(main, rep_left[:B], rep_right[:B], each=True)
    assert got.dtype == each.dtype == np.int64 and got.shape == (2 * n - 1,) and each.shape == (B, 2 * n - 1)
    assert (each == phi).all(), (n, B, kind)
    assert (got == want).all(), (n, B, kind)
    assert (ctx.tree_transfer(main, rep_left[:B], rep_right[:B]) == want).all()
    return got, each


@pytest.mark.parametrize("n", SIZES)
def test_tree_transfer_equals_the_restatement(ctx, n):
    for B in (1, 7):
        got, each = check_tree_transfer(ctx, n, B)
        depth = tr.depths(*trees(n)[0])
        assert ((got >= 0) == (depth >= 0)).all() and n - 3 <= (got >= 0).sum() <= n - 2 and (each[:, depth >= 0] <= depth[depth >= 0] - 1).all()
    if n >= 63:  # random trees of this size share next to nothing: the indices are not all 0 and not all at their bound
        shown = depth >= 0
        assert (each[:, shown] > 0).any() and (each[:, shown] < depth[shown] - 1).any()


@pytest.mark.parametrize("n", SIZES)
def test_chunks_of_one_tree(ctx, monkeypatch, n):
    plain = check_tree_transfer(ctx, n, 7)
    monkeypatch.setenv("DAFS_NJ_BOOT_BYTES", "1")
    ctx.stage_timing(True)
    ctx.stage_report()
    try:
        got = check_tree_transfer(ctx, n, 7)
        stages = ctx.stage_report()
    finally:
        ctx.stage_timing(False)
    assert (got[0] == plain[0]).all() and (got[1] == plain[1]).all()
    assert stages["k_transfer_sides"][2] == stages["k_transfer"][2] == 2 * 7  # two calls of seven chunks


@pytest.mark.parametrize("n", [5, 64, 129])
def test_the_main_tree_among_the_replicates(ctx, n):
    got, each = check_tree_transfer(ctx, n, 7, "member")
    shown = tr.depths(*trees(n, "member")[0]) >= 0
    assert (each[3, shown] == 0).all() and (each[3, ~shown] == -1).all()


@pytest.mark.parametrize("n", [5, 64, 65, 129])
def test_a_caterpillar_as_the_main_tree(ctx, n):
    main = trees(n, "caterpillar")[0]
    depth = tr.depths(*main)
    assert sorted(depth[depth >= 0].tolist()) == sorted(min(k, n - k) for k in range(2, n - 1))  # a side of every size
    check_tree_transfer(ctx, n, 7, "caterpillar")
    # against itself and against the chain over the reversed order (the same unrooted tree): nothing has to move
    order = [int(main[0][n]), int(main[1][n])] + [int(main[1][n + t]) for t in range(1, n - 1)]
    same = tr.caterpillar(n, order[::-1])
    got = ctx.tree_transfer(main, [main[0], same[0]], [main[1], same[1]])
    assert (got == np.where(depth >= 0, 0, -1)).all()


# ---- dafs_hip_alignment_bootstrap_transfer ----
@pytest.fixture
def form(request, monkeypatch):
    if request.param == "looped":
        monkeypatch.setenv("DAFS_NJ_BATCH_MAX_N", "0")
    return request.param


@functools.lru_cache(maxsize=None)
def main_tree(n, length):
    return restate(nj_ref.distances_ref(*br.counts(alignment(n, length)), "jc"))


@pytest.mark.parametrize("form", ["batched", "looped"], indirect=True)
@pytest.mark.parametrize("n,length", [(12, 40), (70, 30)])
def test_alignment_bootstrap_with_transfer(ctx, monkeypatch, n, length, form):
    cell, tree, B = alignment(n, length), main_tree(n, length), 5
    support, rep_left, rep_right = ctx.alignment_bootstrap(cell, B=B, tree=tree, trees=True)
    got = ctx.alignment_bootstrap(cell, B=B, tree=tree, trees=True, transfer=True)
    assert len(got) == 4 and all(g.dtype == np.int64 for g in got)
    assert (got[0] == support).all() and (got[1] == rep_left).all() and (got[2] == rep_right).all()
    transfer, phi = tr.transfer_ref(tree[0], tree[1], rep_left, rep_right)
    assert (got[3] == transfer).all(), (n, length, form)
    shown = support >= 0
    assert ((phi == 0).sum(0)[shown] == support[shown]).all() and (support == br.support_ref(tree[0], tree[1], rep_left, rep_right)).all()
    depth = tr.depths(tree[0], tree[1])
    assert (B - support[shown] <= transfer[shown]).all() and (transfer[shown] <= (B - support[shown]) * (depth[shown] - 1)).all()
    # without the trees, and in chunks of one replicate
    pair = ctx.alignment_bootstrap(cell, B=B, tree=tree, transfer=True)
    assert len(pair) == 2 and (pair[0] == support).all() and (pair[1] == transfer).all()
    assert (ctx.alignment_bootstrap(cell, B=B, tree=tree) == support).all()  # the default return value
    monkeypatch.setenv("DAFS_NJ_BOOT_BYTES", "1")
    ctx.stage_timing(True)
    ctx.stage_report()
    try:
        pair = ctx.alignment_bootstrap(cell, B=B, tree=tree, transfer=True)
        stages = ctx.stage_report()
    finally:
        ctx.stage_timing(False)
    assert (pair[0] == support).all() and (pair[1] == transfer).all()
    assert stages["k_transfer_sides"][2] == stages["k_transfer"][2] == stages["k_boot_pack"][2] == B


def test_degenerate_sizes_launch_nothing(ctx):
    ctx.stage_timing(True)
    ctx.stage_report()
    try:
        for n in (1, 2, 3):
            left, right = (np.array([-1]), np.array([-1])) if n == 1 else tr.caterpillar(n)
            got, each = ctx.tree_transfer((left, right), [left] * 4, [right] * 4, each=True)
            assert got.tolist() == [-1] * (2 * n - 1) and each.tolist() == [[-1] * (2 * n - 1)] * 4
            cell = alignment(5, 64)[:n]
            support, transfer = ctx.alignment_bootstrap(cell, B=4, tree=(left, right), transfer=True)
            assert support.tolist() == transfer.tolist() == [-1] * (2 * n - 1)
        assert ctx.stage_report() == {}
    finally:
        ctx.stage_timing(False)


def _raw(ctx, n, main, B, reps, null=None, each=True):
    T = 2 * n - 1 if n else 1
    arrays = [np.ascontiguousarray(a, np.int32) for a in (main[0], main[1], reps[0], reps[1])]
    transfer = np.full(T, -7, np.int64)
    phi = np.full((max(B, 1), T), -7, np.int32)
    ptr = [a.ctypes.data for a in arrays] + [transfer.ctypes.data, phi.ctypes.data if each else None]
    if null is not None and null != "ctx":
        ptr[null] = None
    rc = capi._tree_transfer(ctx._h if null != "ctx" else None, n, ptr[0], ptr[1], B, ptr[2], ptr[3], ptr[4], ptr[5])
    return rc, capi._last_error().decode(), bool((transfer == -7).all() and (phi == -7).all())


def test_refusals_leave_the_context_usable(ctx):
    n = 5
    main, rep_left, rep_right = trees(n)
    reps = (rep_left, rep_right)
    bad_main = (np.array(main[0]), main[1])
    bad_main[0][6] = 6
    bad_reps = (np.array(rep_left), rep_right)
    bad_reps[0][4, 7] = 8
    twice = (np.array(rep_left), np.array(rep_right))
    twice[0][2, n:], twice[1][2, n:] = [0, 1, 0, 6], [1, 2, 5, 7]  # leaf 1 is a child twice
    cases = [(n, main, 7, reps, k, "tree_transfer: a missing argument") for k in (0, 1, 2, 3, 4, "ctx")] + [
        (0, main, 7, reps, None, "tree_transfer: it takes 1 to 16384 leaves"),
        (16385, main, 7, reps, None, "tree_transfer: it takes 1 to 16384 leaves"),
        (n, main, 0, reps, None, "tree_transfer: it takes 1 to 65536 replicate trees"),
        (n, main, 65537, reps, None, "tree_transfer: it takes 1 to 65536 replicate trees"),
        (n, bad_main, 7, reps, None, "tree_transfer: the main tree: malformed tree (a child that is not an earlier node)"),
        (n, main, 7, bad_reps, None, "tree_transfer: replicate 4: malformed tree (a child that is not an earlier node)"),
        (n, main, 7, twice, None, "tree_transfer: replicate 2: malformed tree (a node that is a child twice)"),
    ]
    for size, m, B, r, null, text in cases:
        rc, msg, untouched = _raw(ctx, size, m, B, r, null)
        assert rc == -1 and msg == text and untouched, text
        check_tree_transfer(ctx, n, 7)  # a valid call follows
    assert _raw(ctx, n, main, 7, reps, each=False)[0] == 0  # transfer_each may be NULL
    with pytest.raises(ValueError, match="replicate 4: malformed tree"):
        ctx.tree_transfer(main, *bad_reps)
    with pytest.raises(ValueError, match=r"\[B, 2n - 1\]"):
        ctx.tree_transfer(main, rep_left[:, :-1], rep_right[:, :-1])
    # dafs_hip_alignment_bootstrap_transfer: its own null pointer, and a refusal of the shared body
    cell = np.ascontiguousarray(alignment(5, 64))
    left, right = (np.ascontiguousarray(a, np.int32) for a in main)
    support, transfer = np.full(9, -7, np.int32), np.full(9, -7, np.int64)
    args = [ctx._h, 5, 64, cell.ctypes.data, None, 1, 4, 12345, left.ctypes.data, right.ctypes.data, support.ctypes.data, None, None]
    assert capi._alignment_bootstrap_transfer(*args, None) == -1 and capi._last_error() == b"alignment_bootstrap_transfer: a missing argument"
    args[6] = 0
    assert capi._alignment_bootstrap_transfer(*args, transfer.ctypes.data) == -1
    assert capi._last_error().decode() == capi.bootstrap_refusal(capi.BOOT_COUNT) and (support == -7).all() and (transfer == -7).all()
    args[6] = 4
    assert capi._alignment_bootstrap_transfer(*args, transfer.ctypes.data) == 0 and (transfer[5:8] >= 0).any()
    with pytest.raises(ValueError, match="malformed tree"):
        ctx.alignment_bootstrap(cell, B=3, tree=bad_main, transfer=True)
    check_tree_transfer(ctx, n, 7)


_L0_CHILD = """
import sys
import numpy as np
import torch  # before the library: both then share torch's HIP runtime, as in bench.py
torch.cuda.init()
sys.path.insert(0, %r)
from dafs_amd import capi
from test_transfer_gpu import trees
dev = torch.device("cuda", 0)
saved = {}
count = 3
for n in (5, 64, 65):
    main, rep_left, rep_right = trees(n)
    left, right = (np.ascontiguousarray(a, np.int32) for a in main)
    pos, lo, ln = np.zeros(n, np.uint32), np.zeros(2 * n - 1, np.uint32), np.zeros(2 * n - 1, np.uint32)
    capi.check(capi._transfer_runs(n, left.ctypes.data, right.ctypes.data, pos.ctypes.data, lo.ctypes.data, ln.ctypes.data))
    nodes = np.flatnonzero(ln)
    split = np.stack([lo[nodes], ln[nodes]], 1).astype(np.uint32)
    d_pos, d_split = torch.from_numpy(pos.view(np.int32)).to(dev), torch.from_numpy(split.view(np.int32)).to(dev)
    d_left = torch.from_numpy(rep_left[:count].astype(np.int32)).to(dev)
    d_right = torch.from_numpy(rep_right[:count].astype(np.int32)).to(dev)
    keep = d_left.clone(), d_right.clone()
    ws = torch.full((capi.tree_transfer_workspace(n, count),), 255, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() %% 256 == 0
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    d_sum = torch.full((len(nodes),), 1000, dtype=torch.int64, device=dev)  # the call adds to what it finds
    d_each = torch.full((count, len(nodes)), -7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        capi.check(capi.tree_transfer_launch(n, count, len(nodes), d_pos.data_ptr(), d_split.data_ptr(), d_left.data_ptr(), d_right.data_ptr(),
                                             ws.data_ptr(), d_sum.data_ptr(), d_each.data_ptr(), stream.cuda_stream))
    stream.synchronize()
    assert ws[:8 * count].cpu().numpy().view(np.uint32).tolist() == [0] * (2 * count)  # the heads: nothing refused
    assert torch.equal(d_left, keep[0]) and torch.equal(d_right, keep[1])
    each = np.full((count, 2 * n - 1), -1, np.int64)
    each[:, nodes] = d_each.cpu().numpy()
    total = np.full(2 * n - 1, -1, np.int64)
    total[nodes] = d_sum.cpu().numpy() - 1000
    saved[str(n)] = np.concatenate([each.ravel(), total])
    # without the indices one by one, on the null stream
    d_sum.fill_(0)
    torch.cuda.synchronize(dev)
    capi.check(capi.tree_transfer_launch(n, count, len(nodes), d_pos.data_ptr(), d_split.data_ptr(), d_left.data_ptr(), d_right.data_ptr(),
                                         ws.data_ptr(), d_sum.data_ptr(), None, None))
    torch.cuda.synchronize(dev)
    assert (d_sum.cpu().numpy() == total[nodes]).all()
    a = (n, count, len(nodes), d_pos.data_ptr(), d_split.data_ptr(), d_left.data_ptr(), d_right.data_ptr(), ws.data_ptr(), d_sum.data_ptr(), None, None)
    for at, bad in ((0, 3), (0, 16385), (1, 0), (1, 32769), (2, 0), (2, 2 * n - 1), (3, None), (5, None), (7, None), (7, ws.data_ptr() + 8), (8, None)):
        assert capi.tree_transfer_launch(*(a[:at] + (bad,) + a[at + 1:])) == -1, (at, bad)
np.savez(sys.argv[1], **saved)
"""


def test_l0_on_torch_tensors_and_a_stream(tmp_path):
    """dafs_hipk_tree_transfer on torch's memory and a non-default torch stream equals the restatement, adds to the sums it
    finds, reports nothing in its heads and leaves the trees alone.  A child process, so that torch starts the HIP runtime
    before the library is loaded."""
    path = str(tmp_path / "l0.npz")
    r = subprocess.run([sys.executable, "-c", _L0_CHILD % os.path.join(ROOT, "tests"), path], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.load(path)
    for n in (5, 64, 65):
        phi = reference(n)[:3]
        want = np.where(tr.depths(*trees(n)[0]) >= 0, phi.sum(0), -1)
        assert np.array_equal(got[str(n)], np.concatenate([phi.ravel(), want])), n


# ---- the drivers ----
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
RF00005 = os.path.join(ROOT, "tests", "golden", "RF00005_0.fa")  # ten sequences


def _fasta(path):
    names, seqs = [], []
    for line in open(path):
        if line.startswith(">"):
            names.append(line[1:].strip())
            seqs.append("")
        elif line.strip():
            seqs[-1] += line.strip()
    return names, seqs


def _cli(*args, ok=True):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr
    return r.stdout if ok else r.stderr


def test_both_drivers_write_the_restatements_bytes(ctx, tmp_path):
    from dafs_amd import pipeline, stockholm
    names, seqs = _fasta(RF00005)
    B = 5
    nwk, tab, sto = tmp_path / "t.nwk", tmp_path / "s.tsv", tmp_path / "a.sto"
    plain = _cli("--stockholm", sto, RF00005)
    assert _cli("--phylogeny", nwk, "--phylogeny-bootstrap", B, "--phylogeny-transfer", "--phylogeny-support", tab, RF00005) == plain
    res = pipeline.run(names, seqs, ctx=ctx, phylogeny="jc", phylogeny_bootstrap=B, phylogeny_transfer=True)
    # the restatement alone, from the printed rows
    cell = capi.encode_cells(res.rows)
    tree = restate(nj_ref.distances_ref(*br.counts(cell), "jc"))
    support, rep_left, rep_right = br.bootstrap_ref(cell, None, "jc", B, 12345, tree)
    transfer, _ = tr.transfer_ref(tree[0], tree[1], rep_left, rep_right)
    assert not any(ch in nm for nm in res.row_names for ch in "()[]':;, \t")
    newick = tr.newick_ref(res.row_names, tree[0], tree[1], tree[2], transfer, B)
    table = tr.table_ref(res.row_names, tree[0], tree[1], support, transfer, B, 12345, "jc")
    phy = res.phylogeny
    assert res.output == plain and (phy.support == support).all() and (phy.transfer == transfer).all()
    assert (phy.depth == tr.depths(tree[0], tree[1])).all() and phy.replicates == B
    assert nwk.read_text() == phy.newick == newick
    assert tab.read_text() == phy.support_table == table and table.count("\n") == 1 + 7 and table.startswith(
        "# rows 10 replicates 5 seed 12345 model jc measure transfer\n")
    # without the option: the bytes of section 23, from both drivers
    old_newick = br.newick_ref(res.row_names, tree[0], tree[1], tree[2], support, B)
    old_table = br.table_ref(res.row_names, tree[0], tree[1], support, B, 12345, "jc")
    assert _cli("--phylogeny", nwk, "--phylogeny-bootstrap", B, "--phylogeny-support", tab, RF00005) == plain
    old = pipeline.run(names, seqs, ctx=ctx, phylogeny="jc", phylogeny_bootstrap=B).phylogeny
    assert nwk.read_text() == old.newick == old_newick and tab.read_text() == old.support_table == old_table
    assert not hasattr(old, "transfer") and not hasattr(old, "depth") and old_newick != newick
    # --describe of the Stockholm output: the same rows, the same bytes
    nwk2, tab2 = tmp_path / "t2.nwk", tmp_path / "s2.tsv"
    assert _cli("--describe", sto, "--phylogeny", nwk2, "--phylogeny-bootstrap", B, "--phylogeny-support", tab2, "--phylogeny-transfer") == ""
    assert nwk2.read_text() == newick and tab2.read_text() == table
    d = pipeline.describe(*stockholm.read_seed_structure(str(sto)), ctx=ctx, identity=False, phylogeny="jc", phylogeny_bootstrap=B,
                          phylogeny_transfer=True)
    assert d.phylogeny.newick == newick and d.phylogeny.support_table == table
    # the refusal, from both
    refusal = capi.transfer_refusal(capi.TRANSFER_NEEDS_REPLICATES)
    assert refusal in _cli("--phylogeny", nwk, "--phylogeny-transfer", RF00005, ok=False)
    with pytest.raises(ValueError) as e:
        pipeline.run(names, seqs, ctx=ctx, phylogeny="jc", phylogeny_transfer=True)
    assert str(e.value) == refusal


def test_cluster_writes_the_transfer_labels_per_printed_cluster(ctx, tmp_path):
    from dafs_amd import pipeline, synth
    a, b = synth.family_set(5, 45, seed=81), synth.family_set(5, 65, seed=82)
    recs = [("%s%d" % (fam, k), rec[1]) for k in range(5) for fam, rec in (("a", a[k]), ("b", b[k]))]
    names, seqs = [r[0] for r in recs], [r[1] for r in recs]
    fa, nwk, tab = tmp_path / "mixed.fa", tmp_path / "c.nwk", tmp_path / "c.tsv"
    fa.write_text(synth.to_fasta(recs))
    plain = _cli("--cluster-count", 2, fa)
    assert _cli("--cluster-count", 2, "--phylogeny", nwk, "--phylogeny-bootstrap", 6, "--phylogeny-transfer", "--phylogeny-support", tab, fa) == plain
    res = pipeline.cluster(names, seqs, count=2, ctx=ctx, phylogeny="jc", phylogeny_bootstrap=6, phylogeny_transfer=True)
    assert len(res.results) == 2 and all(r is not None and len(r.rows) == 5 for r in res.results)
    assert nwk.read_text() == "".join("==> cluster %d <==\n" % (c + 1) + r.phylogeny.newick for c, r in enumerate(res.results))
    assert tab.read_text() == "".join("==> cluster %d <==\n" % (c + 1) + r.phylogeny.support_table for c, r in enumerate(res.results))
    for r in res.results:
        phy = r.phylogeny
        assert phy.support_table.count("\n") == 3 and phy.support_table.splitlines()[0].endswith(" measure transfer")
        assert phy.newick == tr.newick_ref(r.row_names, phy.left, phy.right, phy.length, phy.transfer, 6)
