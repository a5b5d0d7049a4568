"""CPU tests of the all-against-all pairwise mode (pipeline.pairwise, `dafs --pairwise`): the default pair list, the chunking
under a byte budget, the refusal of bad pair lists and inputs before any context is opened, the score table's exact bytes,
and the command line's refusal of the options a pairwise run does not take -- no HIP call."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
G = os.path.join(ROOT, "tests", "golden")


def test_default_pairs_are_row_major():
    from dafs_amd import pipeline
    assert pipeline.check_pairs(4, None) == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    assert pipeline.check_pairs(2, None) == [(0, 1)]
    ps = pipeline.check_pairs(13, None)
    assert len(ps) == 13 * 12 // 2 and ps == sorted(ps) and all(x < y for x, y in ps)
    # the source pair index of (x, y) in the row-major enumeration (dafs_hip_pairs_from's gather)
    n = 13
    assert all(x * n - x * (x + 1) // 2 + (y - x - 1) == k for k, (x, y) in enumerate(ps))
    # a given list keeps its order
    assert pipeline.check_pairs(5, [(3, 4), (0, 2), (1, 4)]) == [(3, 4), (0, 2), (1, 4)]
    assert pipeline.check_pairs(5, np.array([[0, 1], [2, 3]])) == [(0, 1), (2, 3)]


def test_pair_bytes_counts_the_node():
    from dafs_amd import pipeline
    assert pipeline.pair_bytes(100, 120) == pipeline.family_bytes([100, 120]) + pipeline.node_bytes(100, 120)
    assert pipeline.node_bytes(100, 120) > 40 * 100 * 100  # the node is most of a pair's memory (~40 L^2 bytes, ctx.h)
    assert pipeline.pair_bytes(200, 200) > pipeline.pair_bytes(100, 200) > pipeline.pair_bytes(100, 100)


def test_chunks_cover_every_pair_once():
    from dafs_amd import pipeline
    rng = np.random.default_rng(7)
    lens = [int(v) for v in rng.integers(40, 300, 17)]
    pairs = pipeline.check_pairs(len(lens), None)
    sizes = [pipeline.pair_bytes(lens[x], lens[y]) for x, y in pairs]
    for budget in (1, max(sizes), 3 * max(sizes), sum(sizes) // 5, sum(sizes), 1 << 62):
        chunks = pipeline.pair_chunks(lens, pairs, budget)
        flat = [k for c in chunks for k in c]
        assert flat == list(range(len(pairs)))          # every pair in exactly one chunk, in pair order
        for c in chunks:
            assert len(c) == 1 or sum(sizes[k] for k in c) <= budget
    assert len(pipeline.pair_chunks(lens, pairs, 1 << 62)) == 1
    assert pipeline.pair_chunks(lens, pairs, 1) == [[k] for k in range(len(pairs))]
    # a pair over the budget runs alone, its neighbours pack around it
    lens = [50, 50, 50, 400]
    pairs = [(0, 1), (0, 3), (1, 2), (0, 2)]
    small = pipeline.pair_bytes(50, 50)
    assert pipeline.pair_chunks(lens, pairs, 2 * small) == [[0], [1], [2, 3]]


class _NoContext:
    def __init__(self, *a, **k):
        raise AssertionError("a context was opened before the arguments were checked")


@pytest.mark.parametrize("pairs", [[(1, 1)], [(2, 1)], [(0, 4)], [(-1, 2)], [(0, 1), (1, 2), (0, 1)], []])
def test_bad_pair_lists_refused_before_any_context(monkeypatch, pairs):
    from dafs_amd import capi, pipeline
    monkeypatch.setattr(capi, "Context", _NoContext)
    with pytest.raises(ValueError):
        pipeline.pairwise(["a", "b", "c", "d"], ["ACGU", "GGCC", "AUAU", "CCGG"], pairs=pairs)


def test_bad_inputs_refused_before_any_context(monkeypatch):
    from dafs_amd import capi, pipeline
    monkeypatch.setattr(capi, "Context", _NoContext)
    with pytest.raises(ValueError):
        pipeline.pairwise(["a"], ["ACGU"])
    with pytest.raises(ValueError):
        pipeline.pairwise([], [])
    with pytest.raises(ValueError):
        pipeline.pairwise(["a", "b"], ["ACGU"])
    for kw in (dict(mp=None), dict(bp=None), dict(shard=None), dict(level_sync=True, bp_update=True)):
        with pytest.raises(ValueError):
            pipeline.pairwise(["a", "b"], ["ACGU", "GGCC"], **kw)
    with pytest.raises(TypeError):
        pipeline.pairwise(["a", "b"], ["ACGU", "GGCC"], no_such_option=1)


def test_scores_table_bytes():
    from dafs_amd import pipeline
    n = 4
    names = ["tRNA-1 desc", "b", "c_3", "d"]
    sim = np.eye(n, dtype=np.float32)
    sim[0, 1] = sim[1, 0] = np.float32(0.123456789)
    sim[0, 3] = sim[3, 0] = np.float32(1e-7)
    sim[2, 3] = sim[3, 2] = np.float32(np.nan)
    score = np.full((n, n), np.nan, np.float32)
    score[0, 1] = score[1, 0] = np.float32(-12.5)
    score[0, 3] = score[3, 0] = np.float32(1234567.875)
    score[2, 3] = score[3, 2] = np.float32(np.inf)
    its = np.full((n, n), -1, np.int64)
    its[0, 1] = its[1, 0] = 37
    its[0, 3] = its[3, 0] = 600
    its[2, 3] = its[3, 2] = 1
    got = pipeline.pairwise_scores_tsv(names, [(0, 1), (0, 3), (1, 2), (2, 3)], sim, score, its)
    want = ("1\t2\ttRNA-1 desc\tb\t0.123456791\t-12.5\t37\n"
            "1\t4\ttRNA-1 desc\td\t1.00000001e-07\t1234567.88\t600\n"
            "2\t3\tb\tc_3\t0\tnan\t-1\n"            # a pair that was not asked: NaN score, -1 iterations
            "3\t4\tc_3\td\tnan\tinf\t1\n")
    assert got == want
    # a negative NaN is written as C's writer writes it here, plain "nan"
    score[1, 2] = -np.float32(np.nan)
    assert math.isnan(score[1, 2])
    assert pipeline.pairwise_scores_tsv(names, [(1, 2)], sim, score, its) == "2\t3\tb\tc_3\t0\tnan\t-1\n"
    assert pipeline.pairwise_scores_tsv(names, [], sim, score, its) == ""


def _cli(*args, timeout=60):
    if not os.path.exists(DAFS):
        pytest.skip("the dafs executable is built by build()")
    return subprocess.run([DAFS] + list(args), capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("opt, msg", [(["-r", "2"], "-r cannot be combined"), (["--seed", "S.sto"], "--seed cannot be combined"),
                                      (["--devices", "0,1"], "--devices cannot be combined"),
                                      (["--align-aux", "X"], "--align-aux"), (["--fold-aux", "X"], "--fold-aux"),
                                      (["--save-align-aux", "X"], "--save-align-aux"), (["--save-fold-aux", "X"], "--save-fold-aux")])
def test_cli_refuses_options_pairwise_does_not_take(opt, msg):
    r = _cli("--pairwise", *opt, os.path.join(G, "RF00005_0.fa"))
    assert r.returncode != 0
    assert msg in r.stderr and "--pairwise" in r.stderr
    assert r.stdout == ""


def test_cli_refuses_bad_pairwise_inputs(tmp_path):
    a, b = os.path.join(G, "RF00005_0.fa"), os.path.join(G, "RF00017_4.fa")
    r = _cli("--pairwise", a, b)
    assert r.returncode != 0 and "exactly one input FILE" in r.stderr and r.stdout == ""
    one = tmp_path / "one.fa"
    one.write_text(">only\nACGUACGUACGU\n")
    r = _cli("--pairwise", str(one))
    assert r.returncode != 0 and "at least two sequences" in r.stderr and r.stdout == ""
    r = _cli("--pairwise-scores", str(tmp_path / "t.tsv"), a)
    assert r.returncode != 0 and "--pairwise-scores needs --pairwise" in r.stderr and r.stdout == ""
    assert not (tmp_path / "t.tsv").exists()


def test_cli_help_names_pairwise():
    r = _cli("--help")
    assert r.returncode == 0
    assert "--pairwise " in r.stdout and "--pairwise-scores OUT" in r.stdout
