"""GPU tests of the linkage rules.  Every comparison is equality of the bytes of all three arrays with the
numpy restatement (linkage_ref.py): the host-matrix path of dafs_hip_linkage_tree over sizes from one wavefront to more rows
than the workgroup has threads, the same with the per-row state in global memory (DAFS_HIP_LINKAGE_LDS=0, in a child process),
the context's own similarity block, the L0 launch on a torch tensor and stream, the refusals, pipeline.cluster and the command
line."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_ref
from linkage_ref import RULES, chain_case, linkage_ref
from dafs_amd import capi, pipeline, synth
from test_cluster_gpu import _log, _mixed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
SIZES = (1, 2, 3, 5, 33, 64, 65, 127, 257, 1025, 1100)


def _sym(upper):
    u = np.triu(np.asarray(upper, np.float32), 1)
    s = u + u.T
    iu = np.triu_indices(s.shape[0], 1)
    s[iu] = upper[iu]  # the bits of the upper triangle as given (u + u.T turns -0 into 0)
    s.T[iu] = upper[iu]
    np.fill_diagonal(s, 1.0)
    return s


def cases(n, seed=0):
    """name -> symmetric float32 matrix with a unit diagonal"""
    rng = np.random.default_rng(1000 * n + seed)
    rnd = rng.random((n, n)).astype(np.float32)
    out = {"random": _sym(rnd), "quarters": _sym((np.round(rnd * 4) / 4).astype(np.float32)),
           "equal": _sym(np.full((n, n), 0.375, np.float32))}
    hub = (0.05 + 0.1 * rng.random((n, n))).astype(np.float32)  # one row is near to all the others, the rest are far
    h = n // 2
    hub[h, :] = hub[:, h] = 0.9
    if n > 2:
        hub[min(h + 1, n - 1), h] = hub[h, min(h + 1, n - 1)] = 0.95
    out["hub"] = _sym(np.maximum(hub, hub.T))
    block = rng.integers(0, max(1, n // 6) + 1, n)  # planted blocks, every score inside a block the same
    out["blocks"] = _sym(np.where(block[:, None] == block[None, :], np.float32(0.75), (np.round(rnd * 8) / 32).astype(np.float32)))
    signed = (np.round(rnd * 4) / 4 - 0.5).astype(np.float32)  # 0, -0 and negative values
    signed[(signed == 0) & (rng.random((n, n)) < 0.5)] = -0.0
    out["signed"] = _sym(signed)
    nan_below = out["random"].copy()  # the same upper triangle: the same tree
    nan_below[np.tril_indices(n, -1)] = np.nan
    out["nan_below"] = nan_below
    return out


def _same(got, want):
    return all(np.asarray(g).dtype == w.dtype and np.asarray(g).tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("n", SIZES)
def test_host_matrix_equals_the_restatement(ctx, n, rule):
    refs = {}
    for name, sim in cases(n).items():
        want = refs["random"] if name == "nan_below" else linkage_ref(sim, rule)
        refs[name] = want
        assert _same(ctx.linkage_tree(rule, sim), want), (n, rule, name)


@pytest.mark.parametrize("n", [10224, 10225])
def test_the_largest_lds_form_and_the_first_global_form(ctx, n):
    """16 bytes of per-row state per row fill the workgroup's LDS at n = 10 224; one row more takes the global form.  The
    matrix has a closed-form tree (chain_case; test_linkage_cpu.py holds it against the restatement)"""
    sim, want = chain_case(n)
    for rule in RULES:
        assert _same(ctx.linkage_tree(rule, sim), want), (n, rule)


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from dafs_amd import capi
from test_linkage_gpu import cases
ctx = capi.Context(0)
out = {}
for n in (65, 257):
    for name, sim in cases(n).items():
        for rule in ("single", "complete", "average"):
            score, left, right = ctx.linkage_tree(rule, sim)
            out["%%d %%s %%s" %% (n, name, rule)] = np.concatenate([score.view(np.int32).astype(np.int64), left, right])
ctx.close()
np.savez(sys.argv[1], **out)
"""


def test_per_row_state_in_global_memory_changes_no_result(tmp_path):
    """DAFS_HIP_LINKAGE_LDS=0 is read per call; a fresh child process keeps the switch out of this one"""
    path = str(tmp_path / "trees.npz")
    env = dict(os.environ, DAFS_HIP_LINKAGE_LDS="0")
    r = subprocess.run([sys.executable, "-c", _CHILD % os.path.join(ROOT, "tests"), path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.load(path)
    assert len(got.files) == 2 * 7 * 3
    for n in (65, 257):
        for name, sim in cases(n).items():
            for rule in RULES:
                score, left, right = linkage_ref(sim, rule)
                want = np.concatenate([score.view(np.int32).astype(np.int64), left, right])
                assert np.array_equal(got["%d %s %s" % (n, name, rule)], want), (n, name, rule)


@pytest.fixture(scope="module")
def mixed():
    return _mixed()


def _context_trees(ctx):
    before = ctx.sim()
    for rule in RULES:
        assert _same(ctx.linkage_tree(rule), linkage_ref(before, rule)), rule
        assert _same(ctx.linkage_tree(rule, before), linkage_ref(before, rule)), rule
    assert ctx.sim().tobytes() == before.tobytes()
    return before


def test_the_contexts_own_block(ctx, mixed):
    names, seqs = mixed
    n = len(seqs)
    ctx.set_sequences(seqs)
    assert ctx.similarity()[1] == 1
    one = _context_trees(ctx)
    assert ctx.similarity(max_bytes=1)[1] == n * (n - 1) // 2  # one pair per range
    assert _context_trees(ctx).tobytes() == one.tobytes()
    # after a plain align_posteriors the stores stay valid: the transform gives what it gives without the linkage calls
    ctx.align_posteriors(capi.ALIGN_PROBCONS, 0.01, fetch=False)
    ctx.consistency_match(0.25)
    want = ctx.mp(1)
    ctx.align_posteriors(capi.ALIGN_PROBCONS, 0.01, fetch=False)
    assert _context_trees(ctx).tobytes() == one.tobytes()
    ctx.consistency_match(0.25)
    got = ctx.mp(1)
    assert got._val.tobytes() == want._val.tobytes() and got._col.tobytes() == want._col.tobytes() and len(got._val) > 0


_L0_CHILD = """
import sys
import numpy as np
import torch  # before the library: both then share torch's HIP runtime, as in bench.py
torch.cuda.init()
sys.path.insert(0, %r)
from dafs_amd import capi
from test_linkage_gpu import cases, _same
dev = torch.device("cuda", 0)
ctx = capi.Context(0)
saved = {}
for n in (5, 257):
    sim = cases(n)["quarters"]
    d_sim = torch.from_numpy(sim).to(dev)
    keep = d_sim.clone()
    ws = torch.zeros(capi.linkage_workspace(n), dtype=torch.uint8, device=dev)
    assert ws.data_ptr() %% 256 == 0
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != 0
    for code, rule in enumerate(("single", "complete", "average"), 1):
        out = [torch.full((2 * n - 1,), -7, dtype=t, device=dev) for t in (torch.float32, torch.int32, torch.int32)]
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            capi.check(capi.linkage_launch(code, n, d_sim.data_ptr(), ws.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                           stream.cuda_stream))
        stream.synchronize()
        assert ws[:8].cpu().numpy().view(np.uint32).tolist() == [0, n - 1]
        got = (out[0].cpu().numpy(), out[1].cpu().numpy().astype(np.int64), out[2].cpu().numpy().astype(np.int64))
        assert _same(got, ctx.linkage_tree(rule, sim)), (n, rule)  # L0 is L1
        assert torch.equal(d_sim, keep)
        saved["%%d %%s" %% (n, rule)] = np.concatenate([got[0].view(np.int32).astype(np.int64), got[1], got[2]])
# a non-finite entry above the diagonal: the count is in the workspace, no join ran
n = 65
for bad in (np.inf, -np.inf, np.nan):
    sim = cases(n)["random"]
    sim[3, 40] = sim[12, 64] = bad
    d_sim = torch.from_numpy(sim).to(dev)
    ws = torch.zeros(capi.linkage_workspace(n), dtype=torch.uint8, device=dev)
    out = [torch.full((2 * n - 1,), -7, dtype=t, device=dev) for t in (torch.float32, torch.int32, torch.int32)]
    torch.cuda.synchronize(dev)
    capi.check(capi.linkage_launch(2, n, d_sim.data_ptr(), ws.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None))
    torch.cuda.synchronize(dev)
    assert ws[:8].cpu().numpy().view(np.uint32).tolist() == [2, 0]
    for o in out:
        assert (o[n:].cpu().numpy() == -7).all()
ctx.close()
np.savez(sys.argv[1], **saved)
"""


def test_l0_on_a_torch_tensor_and_stream(tmp_path):
    """dafs_hipk_linkage on torch's memory and a non-default torch stream equals dafs_hip_linkage_tree and the restatement and
    leaves its input alone; a non-finite entry is counted in the workspace and no join runs.  A child process, so that torch
    starts the HIP runtime before the library is loaded."""
    path = str(tmp_path / "l0.npz")
    r = subprocess.run([sys.executable, "-c", _L0_CHILD % os.path.join(ROOT, "tests"), path], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.load(path)
    for n in (5, 257):
        for rule in RULES:
            score, left, right = linkage_ref(cases(n)["quarters"], rule)
            assert np.array_equal(got["%d %s" % (n, rule)], np.concatenate([score.view(np.int32).astype(np.int64), left, right])), (n, rule)


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_a_non_finite_entry_is_refused_before_any_join(ctx, bad):
    n = 65
    sim = cases(n)["random"]
    sim[3, 40] = bad
    sim[12, 64] = bad
    # the Python binding refuses first; the library's own check is the device's count
    with pytest.raises(ValueError, match="not finite"):
        ctx.linkage_tree("average", sim)
    score = np.full(2 * n - 1, -7, np.float32); left = np.full(2 * n - 1, -7, np.int32); right = np.full(2 * n - 1, -7, np.int32)
    rc = capi._linkage_tree(ctx._h, 3, n, sim.ctypes.data, score.ctypes.data, left.ctypes.data, right.ctypes.data)
    assert rc == -1 and b"2 entries above the diagonal are not finite" in capi._last_error()
    assert (score == -7).all() and (left == -7).all() and (right == -7).all()
    # the context is usable afterwards
    good = cases(n)["random"]
    assert _same(ctx.linkage_tree("average", good), linkage_ref(good, "average"))


def test_the_contexts_block_is_refused_where_there_is_none(mixed):
    names, seqs = mixed
    c = capi.Context(0)
    try:
        with pytest.raises(ValueError, match="no sequences"):
            c.linkage_tree("single")
        c.set_sequences(seqs)
        with pytest.raises(ValueError, match="holds no similarity block"):
            c.linkage_tree("single")
        c.set_families([0, 7, len(seqs)])
        c.align_posteriors(capi.ALIGN_PROBCONS, 0.01, fetch=False)
        with pytest.raises(ValueError, match="one family"):
            c.linkage_tree("single")
        c.set_sequences(seqs)
        c.similarity()
        score = np.zeros(64, np.float32); left = np.zeros(64, np.int32); right = np.zeros(64, np.int32)
        assert capi._linkage_tree(c._h, 1, len(seqs) - 1, None, score.ctypes.data, left.ctypes.data, right.ctypes.data) == -1
        assert b"number of sequences" in capi._last_error()
        assert _same(c.linkage_tree("single"), linkage_ref(c.sim(), "single"))
    finally:
        c.close()


def _middle(tree):
    n = (len(tree[0]) + 1) // 2
    return float(tree[0][n + math.ceil((n - 1) / 2) - 1])


@pytest.mark.parametrize("rule", RULES)
def test_pipeline_cluster_cuts_the_linkage_tree(ctx, mixed, rule):
    names, seqs = mixed
    n = len(seqs)
    lens = [len(s) for s in seqs]
    ctx.set_sequences(seqs)
    sim, _ = ctx.similarity()
    tree = linkage_ref(sim, rule)
    threshold = _middle(tree)
    res = pipeline.cluster(names, seqs, threshold=threshold, ctx=ctx, linkage=rule)
    assert res.linkage == rule and res.sim.tobytes() == sim.tobytes() and _same(res.tree, tree)
    assert set(res.seconds) == {"similarity", "tree", "batch", "total"}
    want = cluster_ref.cut(tree, threshold=threshold)[0]
    assert np.array_equal(res.labels, want) and np.array_equal(res.labels, capi.cluster_cut(tree, threshold=threshold)[0])
    assert res.clusters == [[i for i in range(n) if want[i] == c] for c in range(int(want.max()) + 1)]
    assert 1 < len(res.clusters) < n
    assert res.tree_line == pipeline.tree_string(tree[0], tree[1], tree[2], names)
    assert res.table == capi.cluster_table(names, lens, want, tree, sim) == cluster_ref.table(names, lens, want, tree, sim)
    for members, got in zip(res.clusters, res.results):  # every aligned cluster is the plain run of its members
        run = pipeline.run([names[i] for i in members], [seqs[i] for i in members], ctx=ctx)
        assert got.output == run.output and _log(got) == _log(run) and got.sim.tobytes() == run.sim.tobytes()
    # by count (nothing aligned: the partition, the tree and the table)
    k = len(res.clusters)
    by_count = pipeline.cluster(names, seqs, count=k, ctx=ctx, linkage=rule, min_size=n + 1)
    want_k = cluster_ref.cut(tree, count=k)[0]
    assert _same(by_count.tree, tree) and np.array_equal(by_count.labels, want_k) and by_count.results == [None] * k
    assert by_count.table == capi.cluster_table(names, lens, want_k, tree, sim) and by_count.tree_line == res.tree_line
    one = pipeline.cluster(names[:1], seqs[:1], count=1, ctx=ctx, linkage=rule, min_size=2)  # the one-leaf tree
    assert _same(one.tree, linkage_ref(np.ones((1, 1), np.float32), rule)) and one.clusters == [[0]]


def test_pipeline_cluster_guide_is_the_call_without_the_argument(ctx, mixed):
    names, seqs = mixed
    a = pipeline.cluster(names, seqs, count=5, ctx=ctx, min_size=4)
    b = pipeline.cluster(names, seqs, count=5, ctx=ctx, min_size=4, linkage="guide")
    assert b.linkage == "guide" and a.linkage == "guide" and _same(a.tree, b.tree) and _same(a.tree, capi.build_tree(a.sim))
    assert a.table == b.table and a.tree_line == b.tree_line and a.clusters == b.clusters
    assert [r and r.output for r in a.results] == [r and r.output for r in b.results]


def _cli(*args):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_equals_python(ctx, mixed, tmp_path):
    names, seqs = mixed
    fa = tmp_path / "mixed.fa"
    fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    res = pipeline.cluster(names, seqs, count=5, ctx=ctx, linkage="average", min_size=3)
    assert _same(res.tree, linkage_ref(res.sim, "average"))
    tsv, tree = tmp_path / "t.tsv", tmp_path / "tree.txt"
    out = _cli("--cluster-linkage", "average", "--cluster-count", 5, "--cluster-min-size", 3, "--cluster-table", tsv, "--cluster-tree", tree, fa)
    assert out == "".join("==> cluster %d <==\n" % (c + 1) + r.output for c, r in enumerate(res.results) if r is not None) and out
    assert tsv.read_text() == res.table
    assert tree.read_text() == res.tree_line + "\n"
    # the default rule by its name: byte for byte the command without the option
    t1, t2, g1, g2 = (tmp_path / x for x in ("a.tsv", "b.tsv", "a.txt", "b.txt"))
    plain = _cli("--cluster-count", 5, "--cluster-min-size", 3, "--cluster-table", t1, "--cluster-tree", g1, fa)
    guide = _cli("--cluster-linkage", "guide", "--cluster-count", 5, "--cluster-min-size", 3, "--cluster-table", t2, "--cluster-tree", g2, fa)
    assert plain == guide and plain and t1.read_bytes() == t2.read_bytes() and g1.read_bytes() == g2.read_bytes()
    assert g1.read_text() != tree.read_text()
