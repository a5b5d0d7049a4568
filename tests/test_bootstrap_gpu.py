"""GPU tests of the bootstrap support.  Every comparison is equality of arrays with the numpy restatement
(bootstrap_ref.py on nj_ref.py), never a tolerance: dafs_hip_nj_trees per matrix in both of its forms, the L0 launch on torch
tensors and a torch stream, the replicate cells, the support and the replicate trees of dafs_hip_alignment_bootstrap under
every tests-only switch, the degenerate sizes, the refusals, and the three drivers byte for byte.

The restatement is the slow side (Python loops over n x n entries per replicate), so its replicates are computed once per
alignment and shared: replicate k does not depend on B, and B = 1 and 7 are prefixes of B = 64.  The sizes 4 and 5 run the
whole product of lengths, replicate counts and models; 65 and 130 rows (two tiles of s, more rows than a tile of r, an odd
row in the last tile) run every length and both models at B = 7 and one B = 64 each."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import bootstrap_ref as br
import nj_ref
from nj_ref import nj_ref as restate
from dafs_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("plane", "equal", "minus_zero", "additive")
FORMS = ("batched", "looped")


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture
def form(request, monkeypatch):
    if request.param == "looped":
        monkeypatch.setenv("DAFS_NJ_BATCH_MAX_N", "0")
    return request.param


def matrix(n, k):
    """matrix k of the n-row set: the kinds in turn"""
    kind = KINDS[k % 4]
    rng = np.random.default_rng(100000 * n + k)
    if kind == "plane":
        pts = rng.random((n, 2))
        return np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
    if kind == "equal":  # ties everywhere: the first join is (0, 1)
        return np.full((n, n), 0.375)
    if kind == "minus_zero":
        d = np.round(rng.random((n, n)) * 4) / 4
        d[d == 0.0] = -0.0
        d[0, n - 1] = -0.0
        return d
    return nj_ref.tree_distances(*nj_ref.random_tree(rng, n))  # every length comes back exactly


@functools.lru_cache(maxsize=None)
def trees_reference(n, count):
    """the restatement's trees of the first `count` matrices, as nj_trees returns them; computed once and shared"""
    trees = [restate(matrix(n, k)) for k in range(count)]
    return tuple(np.array([t[i] for t in trees]) for i in range(3))


def _same(got, want):
    return all(np.asarray(g).dtype == np.asarray(w).dtype and np.asarray(g).shape == np.asarray(w).shape and
               np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("n", [2, 3, 4, 5, 63, 64, 65, 130])
def test_nj_trees_equal_the_restatement(ctx, n, form):
    for count in (1, 7):
        dists = np.array([matrix(n, k) for k in range(count)])
        got = ctx.nj_trees(dists)
        assert _same(got, tuple(a[:count] for a in trees_reference(n, 7))), (n, count)
    if n >= 4:
        assert got[0][1, n] == 0 and got[1][1, n] == 1  # the all-equal matrix
        left, right, length = (a[3] for a in got)      # the additive one: the tree it was read off
        want = nj_ref.unrooted_edges(*nj_ref.random_tree(np.random.default_rng(100000 * n + 3), n))
        assert nj_ref.unrooted_edges(left, right, length) == want
    if n >= 63:
        assert any(np.signbit(matrix(n, 2)[np.triu_indices(n, 1)]) & (matrix(n, 2)[np.triu_indices(n, 1)] == 0))


@pytest.mark.parametrize("form", FORMS, indirect=True)
@pytest.mark.parametrize("n", [5, 65])
def test_more_matrices_than_compute_units(ctx, n, form):
    count = 300
    got = ctx.nj_trees(np.array([matrix(n, k) for k in range(count)]))
    assert _same(got, trees_reference(n, count)), n
    one = ctx.nj_tree(matrix(n, 0))
    assert _same(tuple(a[0] for a in got), one)  # a batch of trees is the single call's tree, matrix by matrix


def test_one_leaf(ctx):
    left, right, length = ctx.nj_trees(np.zeros((3, 1, 1)))
    assert left.tolist() == [[-1]] * 3 and right.tolist() == [[-1]] * 3 and length.tolist() == [[0.0]] * 3


def _raw_trees(ctx, n, dists):
    count = len(dists)
    T = max(2 * n - 1, 1)
    left = np.full((count, T), -7, np.int32); right = np.full((count, T), -7, np.int32); length = np.full((count, T), -7.0)
    rc = capi._nj_trees(ctx._h, n, count, dists.ctypes.data, left.ctypes.data, right.ctypes.data, length.ctypes.data)
    return rc, capi._last_error(), bool((left == -7).all() and (right == -7).all() and (length == -7.0).all())


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_nj_trees_refusals(ctx, form):
    n = 65
    dists = np.array([matrix(n, k) for k in range(7)])
    for bad in (np.inf, np.nan):
        broken = dists.copy()
        broken[3, 4, 40] = bad
        with pytest.raises(ValueError, match=r"matrix 3: the entry \(4, 40\) above the diagonal is not finite"):
            ctx.nj_trees(broken)
        rc, msg, untouched = _raw_trees(ctx, n, broken)
        assert rc == -1 and b"matrix 3" in msg and untouched
    # entries near the largest double: the row sums overflow, the joins run to their end and the call refuses, as nj_tree does
    huge = np.array([matrix(4, 0), np.full((4, 4), 1e308), matrix(4, 2)])
    with pytest.raises(ValueError):
        restate(huge[1])
    with pytest.raises(ValueError, match="matrix 1: the joins overflowed"):
        ctx.nj_trees(huge)
    with pytest.raises(ValueError, match="overflowed"):
        ctx.nj_tree(huge[1])
    rc, msg, untouched = _raw_trees(ctx, 4, huge)
    assert rc == -1 and b"overflowed" in msg and untouched
    assert _raw_trees(ctx, 4, huge[:0])[0] == -1 and _raw_trees(ctx, 0, huge)[0] == -1 and _raw_trees(ctx, capi.NJ_MAX_ROWS + 1, huge)[0] == -1
    assert _same(ctx.nj_trees(dists), trees_reference(n, 7))  # the context is usable afterwards


_L0_CHILD = """
import sys
import numpy as np
import torch  # before the library: both then share torch's HIP runtime, as in bench.py
torch.cuda.init()
sys.path.insert(0, %r)
from dafs_amd import capi
from test_bootstrap_gpu import matrix
dev = torch.device("cuda", 0)
saved = {}
count = 3
for n in (5, 65):
    dists = np.array([matrix(n, k) for k in range(count)])
    d_dist = torch.from_numpy(dists).to(dev)
    keep = d_dist.clone()
    ws = torch.zeros(capi.nj_batch_workspace(n, count), dtype=torch.uint8, device=dev)
    assert ws.data_ptr() %% 256 == 0
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    out = [torch.full((count, 2 * n - 1), -7, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.float64)]
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        capi.check(capi.nj_batch_launch(n, count, d_dist.data_ptr(), ws.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                        stream.cuda_stream))
    stream.synchronize()
    assert ws[:16 * count].cpu().numpy().view(np.uint32).reshape(count, 4).tolist() == [[0, 0, n - 1, 0]] * count
    assert torch.equal(d_dist, keep)
    saved[str(n)] = np.concatenate([out[0].cpu().numpy().astype(np.int64).ravel(), out[1].cpu().numpy().astype(np.int64).ravel(),
                                    out[2].cpu().numpy().view(np.int64).ravel()])
# a non-finite entry above the diagonal of the second matrix: its head counts it and none of its joins ran; the others are whole
n = 5
dists = np.array([matrix(n, k) for k in range(count)])
dists[1, 0, 3] = np.nan
d_dist = torch.from_numpy(dists).to(dev)
ws = torch.zeros(capi.nj_batch_workspace(n, count), dtype=torch.uint8, device=dev)
out = [torch.full((count, 2 * n - 1), -7, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.float64)]
torch.cuda.synchronize(dev)
capi.check(capi.nj_batch_launch(n, count, d_dist.data_ptr(), ws.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None))
torch.cuda.synchronize(dev)
assert ws[:16 * count].cpu().numpy().view(np.uint32).reshape(count, 4).tolist() == [[0, 0, n - 1, 0], [1, 0, 0, 0], [0, 0, n - 1, 0]]
assert (out[0][1, n:].cpu().numpy() == -7).all()
assert capi.nj_batch_launch(1, count, d_dist.data_ptr(), ws.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None) == -1
assert capi.nj_batch_launch(n, count, d_dist.data_ptr(), ws.data_ptr() + 8, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None) == -1
np.savez(sys.argv[1], **saved)
"""


@pytest.mark.parametrize("form", FORMS, indirect=True)
def test_l0_on_torch_tensors_and_a_stream(tmp_path, form):
    """dafs_hipk_nj_batch on torch's memory and a non-default torch stream equals the restatement and leaves its input alone.
    A child process, so that torch starts the HIP runtime before the library is loaded; it inherits the form's switch."""
    path = str(tmp_path / "l0.npz")
    r = subprocess.run([sys.executable, "-c", _L0_CHILD % os.path.join(ROOT, "tests"), path], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.load(path)
    for n in (5, 65):
        left, right, length = trees_reference(n, 7)
        assert np.array_equal(got[str(n)], np.concatenate([left[:3].ravel(), right[:3].ravel(), length[:3].view(np.int64).ravel()])), n


# ---- replicate alignments ----
@functools.lru_cache(maxsize=None)
def alignment(n, length, lonely=False):
    """rows that differ from one ancestor in a fifth of their cells, with letters outside ACGU (code 4) and gaps; every row
    keeps a residue.  lonely: row 2 holds one residue, in a column that replicate 0 of seed 12345 does not draw and replicate 1
    does (by the restatement's draws), so that a replicate leaves the row without any"""
    rng = np.random.default_rng(1000 * n + length)
    ancestor = rng.integers(0, 4, length)
    cell = np.where(rng.random((n, length)) < 0.2, rng.integers(0, 4, (n, length)), ancestor[None, :]).astype(np.uint8)
    cell[rng.random((n, length)) < 0.03] = 4
    if length > 1:
        cell[rng.random((n, length)) < 0.10] = 5
        cell[:, 0][cell[:, 0] == 5] = 1
    if lonely:
        first, second = set(br.draws(12345, 0, length)), set(br.draws(12345, 1, length))
        cell[2] = 5
        cell[2, min(second - first)] = 2
    cell.setflags(write=False)
    return cell


def masks(length):
    rng = np.random.default_rng(length)
    one = np.zeros(length, np.uint8)
    one[length // 2] = 1
    some = (rng.random(length) < 0.6).astype(np.uint8)
    some[0] = 1
    return (None, some, one)


@pytest.mark.parametrize("length", [1, 63, 64, 65, 200])
def test_bootstrap_alignment_equals_the_restatement(ctx, length):
    cell = alignment(5, length)
    assert (cell == 4).any() or length == 1
    for use in masks(length):
        for seed, k in ((12345, 0), (12345, 6), (2 ** 64 - 1, 65535)):
            got = ctx.bootstrap_alignment(cell, k, use=use, seed=seed)
            want = br.replicate_cells(cell, use, seed, k)
            assert got.dtype == np.uint8 and got.shape == want.shape and (got == want).all(), (length, seed, k)
    wide = alignment(130, length)  # three tiles of rows s, a last tile of rows r with two rows
    assert (ctx.bootstrap_alignment(wide, 3) == br.replicate_cells(wide, None, 12345, 3)).all()


@functools.lru_cache(maxsize=None)
def main_tree(n, length, model, lonely=False):
    cell = alignment(n, length, lonely)
    return restate(nj_ref.distances_ref(*br.counts(cell), model))


@functools.lru_cache(maxsize=None)
def replicates(n, length, model, B, lonely=False):
    """the restatement's first B replicate trees (left [B, 2n-1], right), computed once and shared"""
    cell = alignment(n, length, lonely)
    trees = [br.replicate_tree(cell, None, model, 12345, k) for k in range(B)]
    return np.array([t[0] for t in trees]), np.array([t[1] for t in trees])


def want_bootstrap(n, length, model, B, most, lonely=False):
    rep_left, rep_right = (a[:B] for a in replicates(n, length, model, most, lonely))
    tree = main_tree(n, length, model, lonely)
    return br.support_ref(tree[0], tree[1], rep_left, rep_right), rep_left, rep_right


def check_bootstrap(ctx, n, length, model, B, most, lonely=False):
    tree = main_tree(n, length, model, lonely)
    got = ctx.alignment_bootstrap(alignment(n, length, lonely), model=model, B=B, seed=12345, tree=tree, trees=True)
    assert _same(got, want_bootstrap(n, length, model, B, most, lonely)), (n, length, model, B)
    return got


@pytest.mark.parametrize("model", ["jc", "p"])
@pytest.mark.parametrize("length", [1, 64, 65, 200])
@pytest.mark.parametrize("n", [4, 5])
def test_alignment_bootstrap_small(ctx, n, length, model):
    for B in (1, 7, 64):
        support = check_bootstrap(ctx, n, length, model, B, 64)[0]
        assert support[2 * n - 2] == -1 and (support[:n] == -1).all() and (support >= 0).sum() >= n - 3 and support.max() <= B


LARGE = [(n, length, 7, model) for n in (65, 130) for length in (1, 64, 65, 200) for model in ("jc", "p")] + [(65, 200, 64, "jc"), (130, 64, 64, "p")]


@pytest.mark.parametrize("n,length,B,model", LARGE)
def test_alignment_bootstrap_large(ctx, n, length, B, model):
    check_bootstrap(ctx, n, length, model, B, B)


def test_a_replicate_may_leave_a_row_without_residues(ctx):
    cell = alignment(5, 65, lonely=True)
    empty = [k for k in range(7) if (br.replicate_cells(cell, None, 12345, k)[2] == 5).all()]
    assert empty and len(empty) < 7  # some replicates lose row 2's one residue, some keep it
    for model in ("jc", "p"):
        check_bootstrap(ctx, 5, 65, model, 7, 7, lonely=True)


def test_the_default_tree_and_a_mask(ctx):
    cell = alignment(5, 200)
    use = masks(200)[1]
    tree = restate(nj_ref.distances_ref(*br.counts(cell[:, use != 0]), "jc"))
    reps = [br.replicate_tree(cell, use, "jc", 99, k) for k in range(5)]
    want = br.support_ref(tree[0], tree[1], [r[0] for r in reps], [r[1] for r in reps])
    got = ctx.alignment_bootstrap(cell, use=use, B=5, seed=99)  # the main tree: alignment_tree of the same rows and mask
    assert got.dtype == np.int64 and (got == want).all()


SWITCHES = {
    "chunks of two replicates": {"DAFS_NJ_BOOT_BYTES": "180000"},
    "every entry through the fix-up list": {"DAFS_NJ_BOOT_GUARD": "0.5"},
    "a fix-up list that overflows": {"DAFS_NJ_BOOT_GUARD": "0.5", "DAFS_NJ_BOOT_FIXUPS": "100"},
    "a fix-up list of a few entries": {"DAFS_NJ_BOOT_GUARD": None},  # chosen below from the restatement's own values
    "a few entries for a list of one": {"DAFS_NJ_BOOT_GUARD": None, "DAFS_NJ_BOOT_FIXUPS": "1"},
    "the looped joins": {"DAFS_NJ_BATCH_MAX_N": "0"},
    "the looped joins in chunks": {"DAFS_NJ_BATCH_MAX_N": "0", "DAFS_NJ_BOOT_BYTES": "100000"},
}


@functools.lru_cache(maxsize=None)
def distances_to_a_step(n, length, B):
    """per Jukes-Cantor entry below the cap of the first B replicates, how far -0.75 * log(x) * 2^20 + 0.5 is from an integer
    (Python floats and math.log), ascending"""
    import math
    cell = alignment(n, length)
    out = []
    for k in range(B):
        ident, aligned = br.counts(br.replicate_cells(cell, None, 12345, k))
        for r in range(n):
            for s in range(r + 1, n):
                comp, mism = int(aligned[r, s]), int(aligned[r, s] - ident[r, s])
                if comp == 0 or 4 * mism >= 3 * comp:
                    continue
                y = -0.75 * math.log(1.0 - (4.0 * float(mism)) / (3.0 * float(comp))) * 1048576.0 + 0.5
                out.append(min(y - math.floor(y), math.floor(y) + 1.0 - y))
    return sorted(out)


@pytest.mark.parametrize("switch", list(SWITCHES))
def test_the_switches_change_no_result(ctx, monkeypatch, switch):
    """n = 65, 200 columns, jc, B = 7: a replicate takes 78 248 bytes batched and 44 200 looped, so 180 000 and 100 000 bytes
    hold two; the stage recorder counts the chunks"""
    plain = check_bootstrap(ctx, 65, 200, "jc", 7, 7)
    near = distances_to_a_step(65, 200, 7)
    distinct = sorted(set(near))
    few = (distinct[4] + distinct[5]) / 2  # five values of the list lie below it, each clear of it by far more than an ulp of log
    assert len(near) > 7 * 2080 * 0.9 and distinct[5] - distinct[4] > 1e-6
    for name, value in SWITCHES[switch].items():
        monkeypatch.setenv(name, repr(few) if value is None else value)
    ctx.stage_timing(True)
    ctx.stage_report()
    try:
        got = check_bootstrap(ctx, 65, 200, "jc", 7, 7)
        stages = ctx.stage_report()
    finally:
        ctx.stage_timing(False)
    assert _same(got, plain)
    chunks = 4 if "DAFS_NJ_BOOT_BYTES" in SWITCHES[switch] else 1
    assert stages["k_boot_pack"][2] == chunks and stages["k_boot_dist"][2] == chunks
    if "DAFS_NJ_BATCH_MAX_N" in SWITCHES[switch]:
        assert "k_nj_batch" not in stages and stages["k_nj_update"][2] == 7 * 64
    else:
        assert stages["k_nj_batch"][2] == chunks and "k_nj_update" not in stages
    fixed = capi.bootstrap_fixups()
    if "0.5" in SWITCHES[switch].values():
        assert fixed == len(near)  # every jc entry below the cap
    elif None in SWITCHES[switch].values():
        assert fixed == sum(1 for d in near if d < few) >= 5
    if "DAFS_NJ_BOOT_FIXUPS" in SWITCHES[switch]:  # more entries than the capacity asked for: the case is one for the overflow path
        assert fixed > int(SWITCHES[switch]["DAFS_NJ_BOOT_FIXUPS"])


def test_degenerate_sizes_launch_nothing(ctx):
    ctx.stage_timing(True)
    ctx.stage_report()
    try:
        for n in (1, 2, 3):
            cell = alignment(5, 64)[:n]
            tree = restate(nj_ref.distances_ref(*br.counts(cell), "jc"))
            support, rep_left, rep_right = ctx.alignment_bootstrap(cell, B=4, tree=tree, trees=True)
            assert support.tolist() == [-1] * (2 * n - 1) and (rep_left == -1).all() and (rep_right == -1).all() and rep_left.shape == (4, 2 * n - 1)
            assert _same((support, rep_left, rep_right), br.bootstrap_ref(cell, None, "jc", 4, 12345, tree))
        assert ctx.stage_report() == {}
    finally:
        ctx.stage_timing(False)


def _raw_bootstrap(ctx, cell, use, model, B, left, right):
    n, L = cell.shape
    support = np.full(2 * n - 1, -7, np.int32)
    left = np.ascontiguousarray(left, np.int32); right = np.ascontiguousarray(right, np.int32)
    rc = capi._alignment_bootstrap(ctx._h, n, L, cell.ctypes.data, None if use is None else use.ctypes.data, model, B, 12345, left.ctypes.data,
                                   right.ctypes.data, support.ctypes.data, None, None)
    return rc, capi._last_error().decode(), bool((support == -7).all())


def test_refusals_leave_the_context_usable(ctx):
    cell = np.ascontiguousarray(alignment(5, 64))
    left, right, _ = main_tree(5, 64, "jc")
    nothing = np.zeros(64, np.uint8)
    bad_left = np.array(left)
    bad_left[6] = 6
    bad_cell = cell.copy()
    bad_cell[3, 3] = 6
    cases = (
        (cell, None, 1, 0, left, capi.bootstrap_refusal(capi.BOOT_COUNT)),
        (cell, None, 1, 65537, left, capi.bootstrap_refusal(capi.BOOT_COUNT)),
        (cell, nothing, 1, 4, left, capi.bootstrap_refusal(capi.BOOT_NO_COLUMN)),
        (cell, None, 2, 4, left, capi.phylogeny_refusal(capi.PHY_UNKNOWN_MODEL)),
        (cell, None, 1, 4, bad_left, "alignment_bootstrap: the main tree: malformed tree (a child that is not an earlier node)"),
        (bad_cell, None, 1, 4, left, "alignment_bootstrap: a cell code above 5"),
    )
    for c, use, model, B, lft, text in cases:
        rc, msg, untouched = _raw_bootstrap(ctx, c, use, model, B, lft, right)
        assert rc == -1 and msg == text and untouched, text
        check_bootstrap(ctx, 5, 64, "jc", 7, 64)  # a valid call follows
    with pytest.raises(ValueError, match="1 to 65536"):
        ctx.alignment_bootstrap(cell, B=0)
    with pytest.raises(ValueError, match="one used column"):
        ctx.alignment_bootstrap(cell, use=nothing, B=3, tree=(left, right))
    with pytest.raises(ValueError, match="malformed tree"):
        ctx.alignment_bootstrap(cell, B=3, tree=(bad_left, right))
    with pytest.raises(ValueError, match="one used column"):
        ctx.bootstrap_alignment(cell, 0, use=nothing)
    with pytest.raises(ValueError, match="jc or p"):
        ctx.alignment_bootstrap(cell, model="k80")


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


def _restated(res, B, seed, model="jc"):
    """(newick, table, support) of a result's printed rows by the restatement alone"""
    cell = capi.encode_cells(res.rows)
    tree = restate(nj_ref.distances_ref(*br.counts(cell), model))
    support = br.bootstrap_ref(cell, None, model, B, seed, tree)[0]
    assert not any(ch in nm for nm in res.row_names for ch in "()[]':;, \t")  # plain names: newick_ref does not quote
    return (br.newick_ref(res.row_names, tree[0], tree[1], tree[2], support, B),
            br.table_ref(res.row_names, tree[0], tree[1], support, B, seed, model), support)


def test_the_three_drivers_write_the_restatements_bytes(ctx, tmp_path):
    from dafs_amd import pipeline, stockholm
    names, seqs = _fasta(RF00005)
    nwk, tab, sto = tmp_path / "t.nwk", tmp_path / "s.tsv", tmp_path / "a.sto"
    plain = _cli("--stockholm", sto, RF00005)
    assert _cli("--phylogeny", nwk, "--phylogeny-bootstrap", 20, "--phylogeny-support", tab, RF00005) == plain  # stdout never changes
    res = pipeline.run(names, seqs, ctx=ctx, phylogeny="jc", phylogeny_bootstrap=20)
    newick, table, support = _restated(res, 20, 12345)
    assert res.output == plain and res.phylogeny.replicates == 20 and res.phylogeny.seed == 12345
    assert (res.phylogeny.support == support).all() and (support >= 0).sum() >= 7 and support.max() > 0
    assert nwk.read_text() == res.phylogeny.newick == newick
    assert tab.read_text() == res.phylogeny.support_table == table and table.count("\n") == 1 + 7  # ten rows: seven splits
    unlabelled = pipeline.run(names, seqs, ctx=ctx, phylogeny="jc").phylogeny
    assert not hasattr(unlabelled, "support") and unlabelled.newick != newick
    assert capi.newick(res.row_names, res.phylogeny.left, res.phylogeny.right, res.phylogeny.length) == unlabelled.newick
    # --describe of the Stockholm output: the same rows, the same bytes
    nwk2, tab2 = tmp_path / "t2.nwk", tmp_path / "s2.tsv"
    assert _cli("--describe", sto, "--phylogeny", nwk2, "--phylogeny-bootstrap", 20, "--phylogeny-support", tab2) == ""
    assert nwk2.read_text() == newick and tab2.read_text() == table
    d = pipeline.describe(*stockholm.read_seed_structure(str(sto)), ctx=ctx, identity=False, phylogeny="jc", phylogeny_bootstrap=20)
    assert d.phylogeny.newick == newick and d.phylogeny.support_table == table
    # another seed and the other model
    _cli("--phylogeny", nwk, "--phylogeny-model", "p", "--phylogeny-bootstrap", 9, "--phylogeny-seed", 7, "--phylogeny-support", tab, RF00005)
    resp = pipeline.run(names, seqs, ctx=ctx, phylogeny="p", phylogeny_bootstrap=9, phylogeny_seed=7)
    newick_p, table_p, _ = _restated(resp, 9, 7, "p")
    assert nwk.read_text() == resp.phylogeny.newick == newick_p and tab.read_text() == resp.phylogeny.support_table == table_p
    assert table_p.startswith("# rows 10 replicates 9 seed 7 model p\n")
    # several files: under the header lines, as --phylogeny lays its lines out
    _cli("--phylogeny", nwk, "--phylogeny-bootstrap", 20, "--phylogeny-support", tab, RF00005, RF00005)
    assert nwk.read_text() == ("==> %s <==\n%s" % (RF00005, newick)) * 2 and tab.read_text() == ("==> %s <==\n%s" % (RF00005, table)) * 2
    batch = pipeline.run_batch([(names, seqs), (names[:3], seqs[:3])], ctx=ctx, phylogeny="jc", phylogeny_bootstrap=20)
    assert batch[0].phylogeny.newick == newick and batch[1].phylogeny.support.tolist() == [-1] * 5


def test_the_drivers_refuse_with_the_librarys_text(ctx, tmp_path):
    from dafs_amd import pipeline
    names, seqs = _fasta(RF00005)
    needs_tree = capi.bootstrap_refusal(capi.BOOT_NEEDS_TREE)
    assert needs_tree in _cli("--phylogeny-bootstrap", 20, RF00005, ok=False)
    assert needs_tree in _cli("--phylogeny-support", tmp_path / "s", RF00005, ok=False)
    assert needs_tree in _cli("--phylogeny-seed", 3, RF00005, ok=False)
    assert capi.bootstrap_refusal(capi.BOOT_NEEDS_REPLICATES) in _cli("--phylogeny", tmp_path / "t", "--phylogeny-support", tmp_path / "s", RF00005, ok=False)
    for bad in ("0", "65537", "x", "-1"):
        assert capi.bootstrap_refusal(capi.BOOT_COUNT) in _cli("--phylogeny", tmp_path / "t", "--phylogeny-bootstrap", bad, RF00005, ok=False)
    with pytest.raises(ValueError) as e:
        pipeline.run(names, seqs, ctx=ctx, phylogeny_bootstrap=20)
    assert str(e.value) == needs_tree
    with pytest.raises(ValueError) as e:
        pipeline.run(names, seqs, ctx=ctx, phylogeny="jc", phylogeny_bootstrap=65537)
    assert str(e.value) == capi.bootstrap_refusal(capi.BOOT_COUNT)
    with pytest.raises(ValueError):
        pipeline.pairwise(names, seqs, ctx=ctx, phylogeny_bootstrap=20)


def test_cluster_writes_a_labelled_tree_per_printed_cluster(ctx, tmp_path):
    from dafs_amd import pipeline, synth
    a, b = synth.family_set(5, 45, seed=81), synth.family_set(5, 65, seed=82)
    recs = [("%s%d" % (fam, k), rec[1]) for k in range(5) for fam, rec in (("a", a[k]), ("b", b[k]))]
    names, seqs = [r[0] for r in recs], [r[1] for r in recs]
    fa, nwk, tab = tmp_path / "mixed.fa", tmp_path / "c.nwk", tmp_path / "c.tsv"
    fa.write_text(synth.to_fasta(recs))
    plain = _cli("--cluster-count", 2, fa)
    assert _cli("--cluster-count", 2, "--phylogeny", nwk, "--phylogeny-bootstrap", 12, "--phylogeny-support", tab, fa) == plain
    res = pipeline.cluster(names, seqs, count=2, ctx=ctx, phylogeny="jc", phylogeny_bootstrap=12)
    assert len(res.results) == 2 and all(r is not None and len(r.rows) == 5 for r in res.results)
    want = [_restated(r, 12, 12345) for r in res.results]
    assert nwk.read_text() == "".join("==> cluster %d <==\n" % (c + 1) + w[0] for c, w in enumerate(want))
    assert tab.read_text() == "".join("==> cluster %d <==\n" % (c + 1) + w[1] for c, w in enumerate(want))
    assert [r.phylogeny.newick for r in res.results] == [w[0] for w in want]
    assert all(w[1].count("\n") == 3 for w in want)  # five rows: two splits each
