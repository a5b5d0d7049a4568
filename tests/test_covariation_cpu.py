"""CPU tests of the covariation statistics: the restatement of the definitions (tests/covariation_ref.py) against the known
answers of DESIGN.md section 13, the code mapping, the cov_SS_cons line and the table from a hand-made result, the command
line's and pipeline.pairwise's refusals, and the exported symbol."""
import os
import subprocess
import types

import numpy as np
import pytest

import covariation_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = cr.NONE
EIGHT = "AUA AUC CGA CGC GCA G-C UAA NAC".split()


def test_mix_and_permutations_known_answers():
    assert cr.mix(1) == 0x5692161D100B05E5
    assert cr.perm(12345, 0, 0, 8) == [4, 6, 5, 2, 7, 3, 1, 0]
    assert cr.perm(1, 3, 7, 10) == [3, 9, 0, 1, 2, 5, 4, 6, 8, 7]
    for seed, k, c, n in ((0, 0, 0, 1), (7, 2, 5, 2), (2 ** 64 - 1, 99, 28499, 65), (3, 1, 2 ** 20, 200)):
        assert sorted(cr.perm(seed, k, c, n)) == list(range(n))


def test_vector_shuffle_is_the_scalar_permutation():
    code = np.random.RandomState(1).randint(0, 5, (37, 11)).astype(np.uint8)
    for seed, k in ((12345, 0), (1, 3), (2 ** 63 + 5, 7)):
        sh = cr.shuffled(code, seed, k)
        for c in range(code.shape[1]):
            assert sh[:, c].tolist() == code[cr.perm(seed, k, c, len(code)), c].tolist(), (seed, k, c)
        assert np.array_equal(np.sort(sh, axis=0), np.sort(code, axis=0))  # the marginals stay


def test_eight_rows_known_answers():
    code = cr.encode(EIGHT)
    out = cr.restate(code, None, 0)
    assert out["g"].tolist() == [[0, 1045692, 81456], [1045692, 0, 81456], [81456, 81456, 0]]
    assert cr.gq_pair(code, 0, 1) == 1045692 and cr.gq_pair(code, 0, 2) == cr.gq_pair(code, 1, 2) == 81456 and cr.gq_pair(code, 1, 1) == 0
    assert out["col_sum"].tolist() == [1127148, 1127148, 162912] and out["total"] == 2417208
    s01 = cr.s_scalar(1045692, 1127148, 1127148, 2417208, 3)
    s02 = cr.s_scalar(81456, 1127148, 162912, 2417208, 3)
    assert abs(s01 - 3.92617183) < 5e-9 and abs(s02 + 0.49580679) < 5e-9
    assert out["best"].tolist() == [1, 0, 0]  # column 2: S(2, 0) = S(2, 1), the smaller column wins
    assert out["best_score"].tolist() == [s01, s01, s02]
    assert np.isnan(out["best_e"]).all()
    # without the third column: len = 2, S is 0 everywhere, and every shuffled pair reaches it
    two = cr.restate(code[:, :2], np.array([1, NONE], np.uint32), 4, seed=9)
    assert two["best_score"].tolist() == [0.0, 0.0] and two["pair_score"].tolist() == [0.0, 0.0]
    assert two["best_e"].tolist() == [1.0, 1.0] and two["pair_e"].tolist() == [1.0, 0.0]
    assert two["pair_rows"].tolist() == [6, 0] and two["pair_canonical"].tolist() == [6, 0] and two["pair_types"].tolist() == [4, 0]


def test_matrix_form_equals_scalar_form_and_s_is_symmetric():
    rs = np.random.RandomState(2)
    code = rs.randint(0, 5, (23, 9)).astype(np.uint8)
    code[:, 4] = 4
    out = cr.restate(code, None, 0)
    g, r, t = out["g"], out["col_sum"], out["total"]
    table = cr.lnq(len(code))
    s = cr.s_matrix(g, r, t, 9)
    for c1 in range(9):
        for c2 in range(9):
            assert int(g[c1, c2]) == cr.gq_pair(code, c1, c2, table)
            if c1 != c2:
                want = cr.s_scalar(int(g[c1, c2]), int(r[c1]), int(r[c2]), t, 9)
                assert s[c1, c2] == want and s[c2, c1] == want
    assert not g[4].any() and out["col_sum"][4] == 0  # an all-gap column pairs with nothing
    assert cr.lnq(3) == [0, 0, 45426, 71999]  # ln 2 = 0.693147..., ln 3 = 1.098612... in units of 2^-16


def test_degenerate_alignments():
    for code in (np.zeros((1, 5), np.uint8), np.zeros((4, 1), np.uint8)):
        for k in (0, 3):
            out = cr.restate(code, None, k)
            assert not out["col_sum"].any() and out["total"] == 0 and (out["best"] == NONE).all() and not out["best_score"].any()
            assert np.isnan(out["best_e"]).all() if k == 0 else not out["best_e"].any()


def test_restatement_finds_exactly_the_planted_pairs():
    """the condition test_covariation_gpu.py puts to the device, met by the restatement alone on the same generator"""
    code, ss = cr.planted_alignment()
    out = cr.restate(code, ss, 100, seed=12345, matrix=False)
    cr.check_planted(out, ss)
    lefts = np.nonzero(ss != NONE)[0]
    assert len(lefts) == 8 and out["pair_score"][lefts].min() > 80 and out["pair_score"][lefts].max() < 102


def test_code_mapping():
    from dafs_amd import capi
    rows = ["ACGUT", "acgut", "N-.RY", "KMSWB", "DHVnX"]
    want = [[0, 1, 2, 3, 3], [0, 1, 2, 3, 3]] + [[4] * 5] * 3
    assert cr.encode(rows).tolist() == want
    got = capi.encode_alignment(rows)
    assert got.dtype == np.uint8 and got.tolist() == want
    assert capi.encode_alignment([r.encode() for r in rows]).tolist() == want
    with pytest.raises(ValueError):
        capi.encode_alignment(["AC", "A"])
    with pytest.raises(ValueError):
        capi.encode_alignment([])


def _result():
    """a hand-made result: columns 0-7, consensus pairs (0, 7) and (1, 5)"""
    res = types.SimpleNamespace()
    res.rows = ["AGCAAUCU", "GGCA-UCC", "CACAAUGG", "UGAA-UUA"]
    res.ss = np.array([7, 5, NONE, NONE, NONE, NONE, NONE, NONE], np.uint32)
    nan = float("nan")
    res.covariation = dict(
        best=np.array([7, 6, 6, NONE, 1, 1, 2, 0], np.uint32),
        best_score=np.array([12.5, 3.25, 3.25, 0.0, -0.125, 1e-5, 3.25, 12.5]),
        best_e=np.array([0.0, 0.04, 0.04, 0.0, 7.5, 0.05, 0.04, 0.0]),
        pair_score=np.array([12.5, 1 / 3.0, 0, 0, 0, 0, 0, 0]), pair_e=np.array([0.0, 123456.789, 0, 0, 0, 0, 0, 0]),
        pair_rows=np.array([4, 4, 0, 0, 0, 0, 0, 0], np.uint32), pair_canonical=np.array([3, 4, 0, 0, 0, 0, 0, 0], np.uint32),
        pair_types=np.array([3, 2, 0, 0, 0, 0, 0, 0], np.uint32), e_max=0.05, shuffles=100, seed=1)
    return res, nan


def test_table_and_cov_line_from_a_hand_made_result():
    from dafs_amd import pipeline, stockholm
    res, nan = _result()
    # other: {1, 6} (E 0.04) named by column 1; {2, 6} by columns 2 and 6, once; {1, 5} is a consensus pair (column 5, E = 0.05
    # exactly, counts); {0, 7} too; column 4's E is too large; column 3 has no partner
    got = pipeline.covariation_tsv(res)
    lines = got.split("\n")
    assert lines[0] == "1\t8\tss\t12.5\t0\t4\t3\t3" and lines[1] == "2\t6\tss\t0.333333333\t123456.789\t4\t4\t2"
    # columns 1 and 6 of the rows: GC GC AG GU -> 4 rows, canonical GC GC GU = 3, types 2
    assert lines[2] == "2\t7\tother\t3.25\t0.04\t4\t3\t2"
    # columns 2 and 6: CC CC CG AU -> canonical CG AU = 2, types 2
    assert lines[3] == "3\t7\tother\t3.25\t0.04\t4\t2\t2"
    assert lines[4:] == [""]
    res.covariation["e_max"] = 2e5  # moves the cov_SS_cons line only: the table's cut stays at 0.05, as on the command line
    assert pipeline.covariation_tsv(res) == got
    assert stockholm.cov_ss_cons(res.ss, res.covariation["pair_e"], 0.05) == "2......2"
    assert stockholm.cov_ss_cons(res.ss, res.covariation["pair_e"], 2e5) == "22...2.2"
    # without shuffles every E is NaN: no column is marked, no other pair is listed, the consensus pairs say nan
    res.covariation["pair_e"] = np.array([nan, nan, 0, 0, 0, 0, 0, 0])
    res.covariation["best_e"] = np.full(8, nan)
    assert stockholm.cov_ss_cons(res.ss, res.covariation["pair_e"]) == "........"
    assert pipeline.covariation_tsv(res) == "1\t8\tss\t12.5\tnan\t4\t3\t3\n2\t6\tss\t0.333333333\tnan\t4\t4\t2\n"


def test_stockholm_block_with_and_without_the_cov_line():
    from dafs_amd import stockholm
    rows = ["AC-G", "A-UG"]
    rel = [np.array([0.97, 0.5, 0.04]), np.array([0.96, 0.15, 0.25])]
    col = np.array([0.965, 0.5, 0.15, 0.145])
    today = ("# STOCKHOLM 1.0\n"
             "#=GF CC [ 0.5 s1 s2 ]\n"
             "s1           AC-G\n"
             "#=GR s1 PP   *5.0\n"
             "s2           A-UG\n"
             "#=GR s2 PP   *.23\n"
             "#=GC SS_cons (..)\n"
             "#=GC PP_cons *521\n"
             "//\n")
    assert stockholm.block("[ 0.5 s1 s2 ]", ["s1", "s2"], rows, rel, col, "(..)") == today
    assert stockholm.block("[ 0.5 s1 s2 ]", ["s1", "s2"], rows, rel, col, "(..)", None, None) == today
    got = stockholm.block(None, ["s1", "s2"], rows, rel, col, "(..)", [True, False, True, True], "2..2")
    assert got == ("# STOCKHOLM 1.0\n"
                   "s1               AC-G\n"
                   "#=GR s1 PP       *5.0\n"
                   "s2               A-UG\n"
                   "#=GR s2 PP       *.23\n"
                   "#=GC SS_cons     (..)\n"
                   "#=GC PP_cons     *521\n"
                   "#=GC cov_SS_cons 2..2\n"
                   "#=GC RF          x.xx\n"
                   "//\n")


def test_covariation_options():
    from dafs_amd import pipeline
    assert pipeline.cov_options(False) is None and pipeline.cov_options(None) is None
    assert pipeline.cov_options(True) == dict(shuffles=100, seed=1, e_max=0.05)
    assert pipeline.cov_options(dict(seed=9)) == dict(shuffles=100, seed=9, e_max=0.05)
    with pytest.raises(ValueError):
        pipeline.cov_options(dict(shuffle=3))


def test_pairwise_refuses_covariation():
    from dafs_amd import pipeline
    with pytest.raises(ValueError, match="covariation"):
        pipeline.pairwise(["a", "b"], ["ACGU", "ACGA"], covariation=True)
    with pytest.raises(ValueError, match="covariation"):
        pipeline.pairwise(["a", "b"], ["ACGU", "ACGA"], covariation=dict(shuffles=0))


def _cli(*args):
    return subprocess.run([DAFS] + list(args), capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args, msg", [
    (["--cov-shuffles", "5"], "need --covariation"), (["--cov-seed", "5"], "need --covariation"),
    (["--pairwise", "--covariation", "OUT"], "--pairwise"), (["--pairwise", "--cov-seed", "2", "--covariation", "OUT"], "--pairwise"),
    (["--covariation", "OUT", "--cov-shuffles", "-1"], "non-negative integer"), (["--covariation", "OUT", "--cov-seed", "x"], "non-negative integer"),
    (["--covariation", ""], "needs a file name")])
def test_cli_refusals_happen_while_parsing(tmp_path, args, msg):
    out = str(tmp_path / "cov.tsv")
    r = _cli(*[out if a == "OUT" else a for a in args], os.path.join(G, "RF00005_0.fa"))
    assert r.returncode != 0 and msg in r.stderr and r.stdout == ""
    assert not os.path.exists(out)


def test_cli_help_names_the_options():
    r = _cli("--help")
    assert r.returncode == 0
    for opt in ("--covariation OUT", "--cov-shuffles K", "--cov-seed S"):
        assert opt in r.stdout


def test_symbol_is_exported_and_declared():
    from dafs_amd import capi
    assert hasattr(capi.lib, "dafs_hip_alignment_covariation")
    assert "dafs_hip_alignment_covariation(" in open(os.path.join(ROOT, "include", "dafs_hip.h")).read()
