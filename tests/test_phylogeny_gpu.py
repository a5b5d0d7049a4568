"""GPU tests of neighbour joining.  Every comparison of a tree is equality of the bytes of left, right
and length with the numpy restatement (nj_ref.py): the host-matrix path of dafs_hip_nj_tree over sizes from one row to more
rows than a workgroup has threads and seven kinds of matrix, the L0 launch on a torch tensor and stream, the refusals,
Context.alignment_tree, pipeline's phylogeny option, `dafs --phylogeny` and `--cov-tree nj`."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import covariation_tree_ref as tr
import nj_ref
from nj_ref import nj_ref as restate
from dafs_amd import capi, pipeline, stockholm, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
SIZES = (1, 2, 3, 4, 5, 33, 64, 65, 127, 257, 1025)
CASES = ("plane", "quarters", "equal", "nonmetric", "additive", "duplicates", "nan_below")


@functools.lru_cache(maxsize=None)
def case(n, name):
    """the n x n float64 matrix of one kind; only the upper triangle is meaningful"""
    rng = np.random.default_rng(1000 * n + CASES.index(name))
    if name in ("plane", "nan_below", "duplicates"):
        pts = np.random.default_rng(1000 * n).random((n, 2))
        if name == "duplicates":  # every third row is a copy of the row before it: zeros off the diagonal
            pts[2::3] = pts[1:-1:3][:len(pts[2::3])]
        d = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1))
        if name == "nan_below":  # the same upper triangle: the same tree
            d[np.tril_indices(n, -1)] = np.nan
        return d
    if name == "quarters":  # ties in Q at every join
        return np.round(rng.random((n, n)) * 4) / 4
    if name == "equal":
        return np.full((n, n), 0.375)
    if name == "nonmetric":  # negative lengths appear and are kept
        return rng.random((n, n))
    assert name == "additive"
    if n < 2:
        return np.zeros((n, n))
    return nj_ref.tree_distances(*nj_ref.random_tree(rng, n))


@functools.lru_cache(maxsize=None)
def reference(n, name):
    """the restatement's tree, computed once and shared"""
    return restate(case(n, "plane" if name == "nan_below" else name))


def _same(got, want):
    return all(np.asarray(g).dtype == np.asarray(w).dtype and np.asarray(g).tobytes() == np.asarray(w).tobytes() for g, w in zip(got, want))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("n", SIZES)
def test_host_matrix_equals_the_restatement(ctx, n):
    for name in CASES[:2] if n == 1025 else CASES:
        got = ctx.nj_tree(case(n, name))
        assert _same(got, reference(n, name)), (n, name)
        if name == "nonmetric" and n >= 33:
            assert (got[2] < 0).any()  # kept, not clamped


_L0_CHILD = """
import sys
import numpy as np
import torch  # before the library: both then share torch's HIP runtime, as in bench.py
torch.cuda.init()
sys.path.insert(0, %r)
from dafs_amd import capi
from test_phylogeny_gpu import case, _same
dev = torch.device("cuda", 0)
ctx = capi.Context(0)
saved = {}
for n in (5, 257):
    dist = case(n, "quarters")
    d_dist = torch.from_numpy(dist).to(dev)
    keep = d_dist.clone()
    ws = torch.zeros(capi.nj_workspace(n), dtype=torch.uint8, device=dev)
    assert ws.data_ptr() %% 256 == 0
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    out = [torch.full((2 * n - 1,), -7, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.float64)]
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(stream):
        capi.check(capi.nj_launch(n, d_dist.data_ptr(), ws.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), stream.cuda_stream))
    stream.synchronize()
    assert ws[:16].cpu().numpy().view(np.uint32).tolist() == [0, 0, n - 1, 0]
    got = (out[0].cpu().numpy().astype(np.int64), out[1].cpu().numpy().astype(np.int64), out[2].cpu().numpy())
    assert _same(got, ctx.nj_tree(dist)), n  # L0 is L1
    assert torch.equal(d_dist, keep)
    saved[str(n)] = np.concatenate([got[0], got[1], got[2].view(np.int64)])
# a non-finite entry above the diagonal: the count is in the workspace, no join ran
n = 65
for bad in (np.inf, -np.inf, np.nan):
    dist = case(n, "plane").copy()
    dist[3, 40] = dist[12, 64] = bad
    d_dist = torch.from_numpy(dist).to(dev)
    ws = torch.zeros(capi.nj_workspace(n), dtype=torch.uint8, device=dev)
    out = [torch.full((2 * n - 1,), -7, dtype=t, device=dev) for t in (torch.int32, torch.int32, torch.float64)]
    torch.cuda.synchronize(dev)
    capi.check(capi.nj_launch(n, d_dist.data_ptr(), ws.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None))
    torch.cuda.synchronize(dev)
    assert ws[:16].cpu().numpy().view(np.uint32).tolist() == [2, 0, 0, 0]
    for o in out[:2]:
        assert (o[n:].cpu().numpy() == -7).all()
ctx.close()
np.savez(sys.argv[1], **saved)
"""


def test_l0_on_a_torch_tensor_and_stream(tmp_path):
    """dafs_hipk_nj on torch's memory and a non-default torch stream equals dafs_hip_nj_tree and the restatement and leaves its
    input alone; a non-finite entry is counted in the workspace and no join runs.  A child process, so that torch starts the
    HIP runtime before the library is loaded."""
    path = str(tmp_path / "l0.npz")
    r = subprocess.run([sys.executable, "-c", _L0_CHILD % os.path.join(ROOT, "tests"), path], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.load(path)
    for n in (5, 257):
        left, right, length = reference(n, "quarters")
        assert np.array_equal(got[str(n)], np.concatenate([left, right, length.view(np.int64)])), n


def _raw(ctx, n, dist):
    T = max(2 * n - 1, 1)
    left = np.full(T, -7, np.int32); right = np.full(T, -7, np.int32); length = np.full(T, -7.0, np.float64)
    rc = capi._nj_tree(ctx._h, n, dist.ctypes.data, left.ctypes.data, right.ctypes.data, length.ctypes.data)
    return rc, capi._last_error(), bool((left == -7).all() and (right == -7).all() and (length == -7.0).all())


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_a_non_finite_entry_is_refused_before_any_join(ctx, bad):
    n = 65
    dist = case(n, "plane").copy()
    dist[3, 40] = bad
    with pytest.raises(ValueError, match="not finite"):
        ctx.nj_tree(dist)
    with pytest.raises(ValueError):
        restate(dist)
    rc, msg, untouched = _raw(ctx, n, dist)
    assert rc == -1 and b"not finite" in msg and untouched
    assert _same(ctx.nj_tree(case(n, "plane")), reference(n, "plane"))  # the context is usable afterwards


def test_too_many_rows_and_overflow_are_refused(ctx):
    small = np.zeros((2, 2))
    rc, msg, untouched = _raw(ctx, capi.NJ_MAX_ROWS + 1, small)  # refused before the matrix is read
    assert rc == -1 and b"16384" in msg and untouched
    assert _raw(ctx, 0, small)[0] == -1
    # four leaves 1e308 apart: the row sums overflow, the joins run to their end and the call refuses
    huge = np.full((4, 4), 1e308)
    with pytest.raises(ValueError):
        restate(huge)
    rc, msg, untouched = _raw(ctx, 4, huge)
    assert rc == -1 and b"overflow" in msg and untouched
    with pytest.raises(ValueError, match="overflow"):
        ctx.nj_tree(huge)
    big = np.full((4, 4), 1e300)  # large and finite throughout: a tree
    assert _same(ctx.nj_tree(big), restate(big))
    assert _same(ctx.nj_tree(case(5, "plane")), reference(5, "plane"))


def _split(recs):
    return [r[0] for r in recs], [r[1] for r in recs]


def _fasta(path):
    names, seqs = [], []
    for line in open(path):
        if line.startswith(">"):
            names.append(line[1:].strip())
            seqs.append("")
        elif line.strip():
            seqs[-1] += line.strip()
    return names, seqs


def _tree_of_rows(ctx, rows, model, use=None):
    """identity counts -> Python distances -> restatement"""
    idt = ctx.alignment_identity(rows, use=use, matrix=True, nearest=False)
    dist = nj_ref.distances_ref(idt.ident, idt.aligned, model)
    assert capi.nj_distances(idt.ident, idt.aligned, model).tobytes() == dist.tobytes()
    return restate(dist)


@functools.lru_cache(maxsize=None)
def _families():
    return _split(synth.family_set(7, 60, seed=2201)), _fasta(os.path.join(G, "RF00005_0.fa"))


@pytest.mark.parametrize("which", [0, 1])
def test_alignment_tree(ctx, which):
    names, seqs = _families()[which]
    rows = pipeline.run(names, seqs, ctx=ctx).rows
    use = np.arange(len(rows[0])) % 3 != 1
    for model in ("jc", "p"):
        assert _same(ctx.alignment_tree(rows, model=model), _tree_of_rows(ctx, rows, model)), model
        assert _same(ctx.alignment_tree(rows, use=use, model=model), _tree_of_rows(ctx, rows, model, use)), model
    assert _same(ctx.alignment_tree(rows), _tree_of_rows(ctx, rows, "jc"))
    with pytest.raises(ValueError):
        ctx.alignment_tree(rows, model="k80")


def _cli(*args, ok=True):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr
    return r.stdout if ok else r.stderr


def _newick(ctx, res, model="jc"):
    """the text capi.newick builds from the restatement's tree of a result's printed rows"""
    return capi.newick(res.row_names, *_tree_of_rows(ctx, res.rows, model))


def test_cli_and_pipeline_write_the_restatements_tree(ctx, tmp_path):
    (names, seqs), (names2, seqs2) = _families()
    fa, fa2 = tmp_path / "a.fa", tmp_path / "b.fa"
    fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    fa2.write_text(synth.to_fasta(list(zip(names2, seqs2))))
    nwk, sto, sto0 = tmp_path / "a.nwk", tmp_path / "a.sto", tmp_path / "plain.sto"
    plain = _cli("--stockholm", sto0, fa)
    assert _cli("--phylogeny", nwk, "--stockholm", sto, fa) == plain and sto.read_bytes() == sto0.read_bytes()  # nothing else changes
    res = pipeline.run(names, seqs, ctx=ctx, phylogeny="jc")
    assert res.output == plain and not hasattr(pipeline.run(names, seqs, ctx=ctx), "phylogeny")
    assert res.phylogeny.newick == nwk.read_text() == _newick(ctx, res) and res.phylogeny.newick.endswith(";\n")
    assert _same((res.phylogeny.left, res.phylogeny.right, res.phylogeny.length), _tree_of_rows(ctx, res.rows, "jc"))
    assert sorted(res.row_names) == sorted(stockholm.names(names)) and all(nm in res.phylogeny.newick for nm in res.row_names)
    _cli("--phylogeny", nwk, "--phylogeny-model", "p", fa)
    resp = pipeline.run(names, seqs, ctx=ctx, phylogeny="p")
    assert nwk.read_text() == resp.phylogeny.newick == _newick(ctx, resp, "p") != res.phylogeny.newick
    # two files: a line per file under its header line, as --identity lays its tables out
    res2 = pipeline.run(names2, seqs2, ctx=ctx, phylogeny="jc")
    both = _cli("--phylogeny", nwk, fa, fa2)
    assert both == "==> %s <==\n%s==> %s <==\n%s" % (fa, plain, fa2, res2.output)
    assert nwk.read_text() == "==> %s <==\n%s==> %s <==\n%s" % (fa, _newick(ctx, res), fa2, _newick(ctx, res2))
    batch = pipeline.run_batch([(names, seqs), (names2, seqs2), (names[:1], seqs[:1])], ctx=ctx, phylogeny="jc")
    assert [b.phylogeny.newick for b in batch[:2]] == [res.phylogeny.newick, res2.phylogeny.newick]
    assert batch[2].phylogeny.newick == stockholm.names(names[:1])[0] + ";\n"  # one row
    # --describe: the finished alignment's rows
    aln = tmp_path / "aln"
    aln.write_text(plain)
    assert _cli("--describe", aln, "--phylogeny", nwk) == ""
    got = stockholm.read_seed_structure(str(aln))
    d = pipeline.describe(*got, ctx=ctx, identity=False, phylogeny="jc")
    assert nwk.read_text() == d.phylogeny.newick == capi.newick(d.row_names, *_tree_of_rows(ctx, d.rows, "jc"))
    # --seed: the added sequences and the seed rows, in printed order
    seed_aln, new_fa = tmp_path / "seed.aln", tmp_path / "new.fa"
    seed_aln.write_text(pipeline.run(names[:4], seqs[:4], ctx=ctx).output)
    new_fa.write_text(synth.to_fasta(list(zip(names[4:], seqs[4:]))))
    snames, srows = stockholm.read_seed(str(seed_aln))
    added = pipeline.add(snames, srows, names[4:], seqs[4:], ctx=ctx, phylogeny="jc")
    assert _cli("--seed", seed_aln, "--phylogeny", nwk, new_fa) == added.output == pipeline.add(snames, srows, names[4:], seqs[4:], ctx=ctx).output
    assert nwk.read_text() == added.phylogeny.newick == _newick(ctx, added)
    # refused where --identity is refused
    with pytest.raises(ValueError):
        pipeline.pairwise(names, seqs, ctx=ctx, phylogeny="jc")
    with pytest.raises(ValueError):
        pipeline.add_each(snames, srows, names[4:], seqs[4:], ctx=ctx, phylogeny="jc")


def test_cli_cluster_writes_a_tree_per_printed_cluster(ctx, tmp_path):
    a, b = synth.family_set(3, 45, seed=81), synth.family_set(3, 65, seed=82)
    recs = [("a0", a[0][1]), ("b0", b[0][1]), ("a1", a[1][1]), ("b1", b[1][1]), ("a2", a[2][1]), ("b2", b[2][1])]
    names, seqs = _split(recs)
    fa, nwk = tmp_path / "mixed.fa", tmp_path / "c.nwk"
    fa.write_text(synth.to_fasta(recs))
    plain = _cli("--cluster-count", 2, fa)
    assert _cli("--cluster-count", 2, "--phylogeny", nwk, fa) == plain
    res = pipeline.cluster(names, seqs, count=2, ctx=ctx, phylogeny="jc")
    assert len(res.results) == 2 and all(r is not None for r in res.results)
    assert plain == "".join("==> cluster %d <==\n" % (c + 1) + r.output for c, r in enumerate(res.results))
    assert nwk.read_text() == "".join("==> cluster %d <==\n" % (c + 1) + _newick(ctx, r) for c, r in enumerate(res.results))
    assert [r.phylogeny.newick for r in res.results] == [_newick(ctx, r) for r in res.results]


def test_cov_tree_nj_hands_the_null_the_restatements_tree(ctx, tmp_path):
    code, ss = tr.phylo(3, 6)
    structure = ["."] * len(ss)
    for c in np.nonzero(ss != tr.NONE)[0]:
        structure[c], structure[int(ss[c])] = "(", ")"
    sto = tmp_path / "x.sto"
    sto.write_text("# STOCKHOLM 1.0\n" + "".join("row%d %s\n" % (r, "".join("ACGU-"[v] for v in row)) for r, row in enumerate(code)) +
                   "#=GC SS_cons " + "".join(structure) + "\n//\n")
    tsv, tsv0, tsv1 = tmp_path / "nj.tsv", tmp_path / "plain.tsv", tmp_path / "average.tsv"
    opts = ("--describe", sto, "--cov-shuffles", "10", "--cov-seed", "5", "--cov-null", "tree")
    assert _cli(*opts, "--covariation", tsv, "--cov-tree", "nj") == ""
    got = stockholm.read_seed_structure(str(sto))
    left, right, _ = _tree_of_rows(ctx, got[1], "jc")
    want = ctx.alignment_covariation(got[1], got[2], shuffles=10, seed=5, null="tree", tree=(left, right))
    restated = tr.restate(code, ss, 10, seed=5, null="tree", tree=(left, right), matrix=False)
    for k in ("best_e", "pair_e", "best_score", "pair_score"):
        assert np.asarray(want[k]).tobytes() == np.asarray(restated[k]).tobytes(), k
    d = pipeline.describe(*got, ctx=ctx, identity=False, covariation=dict(shuffles=10, seed=5, null="tree", tree="nj"))
    for k in ("best_e", "pair_e", "best", "best_score", "pair_score"):
        assert np.asarray(d.covariation[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    assert tsv.read_text() == pipeline.covariation_tsv(d)
    # without --cov-tree, and with the default by its name: the tree null as it was
    _cli(*opts, "--covariation", tsv0)
    _cli(*opts, "--covariation", tsv1, "--cov-tree", "average")
    d0 = pipeline.describe(*got, ctx=ctx, identity=False, covariation=dict(shuffles=10, seed=5, null="tree"))
    assert tsv0.read_bytes() == tsv1.read_bytes() and tsv0.read_text() == pipeline.covariation_tsv(d0)
    default = tr.restate(code, ss, 10, seed=5, null="tree", matrix=False)
    assert np.asarray(d0.covariation["best_e"]).tobytes() == np.asarray(default["best_e"]).tobytes()
