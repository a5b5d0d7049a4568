"""CPU tests of the structural pair score: the known answers of the contract on the numpy restatement,
the two host formulas against it, the test set of test_cluster_structure_gpu.py under stores the oracle computes on the CPU
(the check that those inputs exercise the kernel), synth.structured_family_set, and every refusal that needs no device -- of
capi, of pipeline.cluster and of `dafs --cluster-score`."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import structure_sim_ref as ref
from dafs_amd import capi, pipeline, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
RF00005 = os.path.join(ROOT, "tests", "golden", "RF00005_0.fa")  # ten sequences


def csr(nrows, rows):
    """(rowptr, col, val) from {row: [(col, val), ...]}"""
    rp, col, val = np.zeros(nrows + 1, np.uint32), [], []
    for i in range(nrows):
        for k, v in rows.get(i, []):
            col.append(k)
            val.append(v)
        rp[i + 1] = len(col)
    return rp, np.array(col, np.uint32), np.array(val, np.float32)


def test_known_answers():
    bx, by = csr(6, {0: [(5, 0.5)]}), csr(6, {0: [(5, 0.75)]})
    mp = csr(6, {0: [(0, 0.5)], 5: [(5, 0.25)]})
    assert ref.pair_terms(mp, bx, by) == (51539607552, 1)
    assert (ref.weight(bx), ref.weight(by)) == (549755813888, 824633720832)
    assert ref.structure_score(51539607552, 549755813888, 824633720832).tobytes() == np.float32(0.09375).tobytes()
    # a second base pair on each side
    bx2, by2 = csr(6, {0: [(5, 0.5)], 1: [(4, 0.3)]}), csr(6, {0: [(5, 0.75)], 1: [(4, 0.7)]})
    mp2 = csr(6, {0: [(0, 0.5)], 1: [(1, 0.9)], 4: [(4, 0.6)], 5: [(5, 0.25)]})
    assert ref.pair_terms(csr(6, {1: [(1, 0.9)], 4: [(4, 0.6)]}), csr(6, {1: [(4, 0.3)]}), csr(6, {1: [(4, 0.7)]})) == (124684623072, 1)
    assert ref.pair_terms(mp2, bx2, by2) == (176224230624, 2)
    assert (ref.weight(bx2), ref.weight(by2)) == (879609315328, 1594291847168)
    s = ref.structure_score(176224230624, 879609315328, 1594291847168)
    assert int(s.view(np.uint32)) == 1045243626 and "%.8f" % s == "0.20034376"
    # the columns of rows 0 and 5 swapped: k = 5 > l = 0 contributes nothing, and neither does k = l
    mp3 = csr(6, {0: [(5, 0.5)], 1: [(1, 0.9)], 4: [(4, 0.6)], 5: [(0, 0.25)]})
    assert ref.pair_terms(mp3, bx2, by2) == (124684623072, 1)
    assert ref.pair_terms(csr(6, {0: [(3, 0.5)], 5: [(3, 0.25)]}), bx, csr(6, {3: [(3, 0.75)]})) == (0, 0)
    # the clamp, and a term of 0 still counts
    assert [float(ref.c(v)) for v in (1.5, -0.25, np.nan, 0.25, -0.0)] == [1.0, 0.0, 0.0, 0.25, 0.0]
    assert ref.pair_terms(mp, csr(6, {0: [(5, -0.25)]}), by) == (0, 1)
    assert ref.pair_terms(mp, csr(6, {0: [(5, 1.5)]}), csr(6, {0: [(5, np.nan)]})) == (0, 1)
    assert ref.pair_terms(mp, csr(6, {0: [(5, 1.5)]}), by) == (int(0.75 * 0.125 * 2 ** 40), 1)


def test_host_formulas_equal_the_restatement():
    rng = np.random.default_rng(24)
    cases = [(0, 0, 0), (5, 0, 9), (5, 9, 0), (10, 9, 12), (9, 9, 12), (8, 9, 12), (2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1), (2 ** 64 - 1, 1, 2),
             (1, 2 ** 64 - 1, 2 ** 64 - 1), (2 ** 53 + 1, 2 ** 54 + 3, 2 ** 63)]
    for _ in range(400):
        bits = int(rng.integers(1, 65))
        w = [int(rng.integers(0, 2 ** 63, dtype=np.uint64)) >> (64 - bits) for _ in range(2)]
        t = int(rng.integers(0, 2 ** 63, dtype=np.uint64)) >> int(rng.integers(0, 63))
        cases += [(t, w[0], w[1]), (min(w) // 3, w[0], w[1])]
    for t, wx, wy in cases:
        got = np.float32(capi.structure_score(t, wx, wy))
        assert got.tobytes() == ref.structure_score(t, wx, wy).tobytes(), (t, wx, wy)
        assert 0.0 <= got <= 1.0
    assert capi.structure_score(5, 0, 9) == 0.0 and capi.structure_score(10, 9, 12) == 1.0 and capi.structure_score(9, 12, 9) == 1.0
    vals = rng.random((400, 3)).astype(np.float32)
    edges = [(0.25, 0.75, 0.0), (0.25, 0.75, 1.0), (1.0, 1.0, 0.3), (0.0, 1.0, 0.5), (0.1, 0.1, 0.7), (np.float32(1 / 3), np.float32(0.7), np.float32(0.1))]
    for s, t, w in list(vals) + edges:
        assert np.float32(capi.mix_score(s, t, w)).tobytes() == ref.mix_score(s, t, w).tobytes(), (s, t, w)
    assert capi.mix_score(0.25, 0.75, 0.0) == 0.25 and capi.mix_score(0.25, 0.75, 1.0) == 0.75


def test_structured_family_set_is_deterministic_and_keeps_its_stems():
    fam = synth.structured_family_set(4, 60, stems=2, seed=92)
    assert fam == synth.structured_family_set(4, 60, stems=2, seed=92) and fam != synth.structured_family_set(4, 60, stems=2, seed=93)
    assert [n for n, _ in fam] == ["f0", "f1", "f2", "f3"] and all(set(s) <= set("ACGU") and 50 <= len(s) <= 70 for _, s in fam)
    assert len({s for _, s in fam}) == 4
    # without indels the planted positions stay put: every member pairs them canonically, and compensatory changes occur
    flat = synth.structured_family_set(6, 60, stems=2, seed=92, indel=0.0)
    planted = [(s + 1 + d, s + 30 - 2 - d) for s in (0, 30) for d in range(6)]
    for _, s in flat:
        assert len(s) == 60 and all(s[i] + s[j] in synth._PAIRS for i, j in planted)
    assert any(len({s[i] + s[j] for _, s in flat}) > 1 for i, j in planted)


@pytest.fixture(scope="module")
def oracle_stores():
    """the test set with ProbCons rows at th 0.01 and CONTRAfold rows at 0.01, both from the oracle on the CPU"""
    import oracle_lib
    orc = oracle_lib.load_oracle()
    names, seqs, family = ref.test_set()
    n = len(seqs)
    bps = []
    for s in seqs:
        L = len(s)
        rp = np.zeros(L + 1, np.uint32); col = np.zeros(L * L, np.uint32); val = np.zeros(L * L, np.float32)
        k = orc.lib.orc_fold_calculate(s.encode(), L, None, C.c_float(0.01), rp.ctypes.data, col.ctypes.data, val.ctypes.data)
        assert k >= 0
        bps.append((rp, col[:k].copy(), val[:k].copy()))
    mps = {(x, y): orc.align_calculate(seqs[x], seqs[y], 0.01) for x in range(n) for y in range(x + 1, n)}
    return names, seqs, family, mps, bps


def test_the_test_set_exercises_the_kernel(oracle_stores):
    names, seqs, family, mps, bps = oracle_stores
    n = len(seqs)
    assert n == 15 and sorted(len(s) for s in seqs)[:2] == [3, 9] and max(len(s) for s in seqs) == 130
    T, terms, W, st, _ = ref.matrices(n, mps, bps)
    tiny = names.index("r3")
    assert W[tiny] == 0 and all(W[x] > 0 for x in range(n) if x not in (tiny, names.index("r9")))
    for x in range(n):
        for y in range(x + 1, n):
            # symmetric by construction: the transposed rows with the roles of x and y exchanged
            assert ref.pair_terms(ref.transpose(mps[(x, y)], len(seqs[y])), bps[y], bps[x]) == (T[(x, y)], terms[(x, y)])
            if family[x] is not None and family[x] == family[y]:
                assert T[(x, y)] > 0 and terms[(x, y)] > 0, (names[x], names[y])
            if tiny in (x, y):
                assert st[x, y] == 0.0 and T[(x, y)] == 0
            assert terms[(x, y)] < ref.MAX_TERMS and 0.0 <= st[x, y] <= 1.0
    assert st.tobytes() == st.T.copy().tobytes() and np.all(np.diag(st) == 1.0)


def test_capi_refuses_a_bad_score_before_it_needs_a_context():
    assert capi.SCORES == ("sequence", "structure", "mix")
    for name in ("dafs_hip_structure_scores", "dafs_hip_similarity_scored", "dafs_hip_get_pair_scores", "dafs_host_structure_score", "dafs_host_mix_score"):
        assert getattr(capi.lib, name) is not None
    ctx = object.__new__(capi.Context)
    ctx._h, ctx._lens = None, None
    with pytest.raises(ValueError, match="unknown score"):
        ctx.similarity(score="shape")
    for bad in (-0.01, 1.01, float("nan"), float("inf"), "much"):
        with pytest.raises(ValueError, match=r"0 \.\. 1"):
            ctx.similarity(score="mix", structure_weight=bad)
    # the library's own refusals that come before any device work
    assert capi._similarity_scored(None, 0, 0.01, 0, 7, 0.5, None) == -1 and b"unknown kind" in capi._last_error()
    assert capi._similarity_scored(None, 0, 0.01, 0, 2, 1.5, None) == -1 and b"weight" in capi._last_error()
    assert capi._similarity_scored(None, 0, 0.01, 0, 2, float("nan"), None) == -1 and b"weight" in capi._last_error()
    assert capi._similarity_scored(None, 0, 0.01, 0, 1, 0.5, None) == -1
    assert capi._structure_scores(None, None, None, None) == -1
    assert capi._get_pair_scores(None, None, None) == -1


def test_pipeline_cluster_refuses_before_it_opens_a_context(monkeypatch):
    def no_context(*a, **k):
        raise AssertionError("a context was opened")
    monkeypatch.setattr(capi, "Context", no_context)
    names, seqs = ["a", "b", "c"], ["ACGUACGU", "ACGGACGU", "UUUUCCCC"]
    for bad in ("shape", "Structure", "", None, 1):
        with pytest.raises(ValueError, match="unknown score"):
            pipeline.cluster(names, seqs, threshold=0.5, score=bad)
    for bad in (-0.5, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"0 \.\. 1"):
            pipeline.cluster(names, seqs, threshold=0.5, score="mix", structure_weight=bad)
    for score in ("sequence", "structure"):
        with pytest.raises(ValueError, match="structure_weight is the weight of"):
            pipeline.cluster(names, seqs, threshold=0.5, score=score, structure_weight=0.5)
    for kw in (dict(), dict(score="sequence"), dict(score="structure"), dict(score="mix"), dict(score="mix", structure_weight=0.0),
               dict(score="mix", structure_weight=1.0)):  # the checks passed: the next step is the context
        with pytest.raises(AssertionError, match="a context was opened"):
            pipeline.cluster(names, seqs, count=2, **kw)


@pytest.mark.parametrize("args,message", [
    (["--cluster", "0.5", "--cluster-score", "shape", RF00005], "--cluster-score: unknown score 'shape'"),
    (["--cluster-count", "2", "--cluster-score", "Mix", RF00005], "--cluster-score: unknown score 'Mix'"),
    (["--cluster-score", "structure", RF00005], "--cluster-score and --cluster-structure-weight need --cluster or --cluster-count"),
    (["--cluster-structure-weight", "0.5", RF00005], "--cluster-score and --cluster-structure-weight need --cluster or --cluster-count"),
    (["--cluster", "0.5", "--cluster-score", "mix", "--cluster-structure-weight", "1.5", RF00005], "--cluster-structure-weight needs a weight in 0 .. 1"),
    (["--cluster", "0.5", "--cluster-score", "mix", "--cluster-structure-weight", "-0.1", RF00005], "--cluster-structure-weight needs a weight in 0 .. 1"),
    (["--cluster", "0.5", "--cluster-score", "mix", "--cluster-structure-weight", "nan", RF00005], "--cluster-structure-weight needs a weight in 0 .. 1"),
    (["--cluster", "0.5", "--cluster-score", "mix", "--cluster-structure-weight", "inf", RF00005], "--cluster-structure-weight needs a weight in 0 .. 1"),
    (["--cluster", "0.5", "--cluster-score", "mix", "--cluster-structure-weight", "0.5x", RF00005], "--cluster-structure-weight needs a weight in 0 .. 1"),
    (["--cluster", "0.5", "--cluster-structure-weight", "0.5", RF00005], "--cluster-structure-weight is the weight of --cluster-score mix"),
    (["--cluster", "0.5", "--cluster-score", "structure", "--cluster-structure-weight", "0.5", RF00005], "--cluster-structure-weight is the weight of --cluster-score mix"),
    (["--cluster-count", "2", "--cluster-score", "structure", "--devices", "0,1", RF00005], "--devices cannot be combined with --cluster"),
])
def test_cli_refuses_while_parsing(args, message, tmp_path):
    assert os.path.exists(DAFS), "the dafs executable is built by build()"
    r = subprocess.run([DAFS] + args, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 1
    assert message in r.stderr, r.stderr
    assert r.stderr.count("\n") == 1 and "HIP" not in r.stderr
    assert r.stdout == ""
    assert os.listdir(str(tmp_path)) == []


def test_cli_help_names_the_options():
    r = subprocess.run([DAFS, "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert text.index("--cluster-linkage RULE") < text.index("--cluster-score NAME") < text.index("--cluster-structure-weight W") < text.index("Aligning options")
