"""CPU tests of the alignment comparison: the restatement's known answer and identities, the host text
that both drivers share (row matching, PP reader, table writers), every refused option combination, and the library's symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import compare_ref as cr
from dafs_amd import capi, pipeline, stockholm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
R3 = ["ACGU-", "AC-U-", "-CGUA"]
T3 = ["ACGU--", "A-CU--", "--CGUA"]


def test_known_answer():
    out = cr.compare(cr.cells(R3), cr.cells(T3), ss_r=cr.brackets("(..)."), ss_t=cr.brackets("(..).."))
    assert list(zip(out["shared"], out["refp"], out["testp"])) == [(2, 6, 5), (3, 5, 5), (1, 5, 4)]
    assert (out["total_shared"], out["total_refp"], out["total_testp"]) == (3, 8, 7)
    assert out["sps"] == 0.375 and out["ppv"] == 3.0 / 7.0
    assert out["k"] == [2, 3, 2, 3, 1] and out["colshared"] == [1, 1, 0, 1, 0]
    assert out["reproduced"] == [True, False, False, False, False] and out["tc"] == 0.25
    shared, refp, testp = cr.pair_counts(cr.keys(cr.cells(R3), cr.cells(T3)))
    assert {(r, s): (shared[r][s], refp[r][s], testp[r][s]) for r in range(3) for s in range(r + 1, 3)} == \
        {(0, 1): (2, 3, 3), (0, 2): (0, 3, 2), (1, 2): (1, 2, 2)}
    assert list(zip(out["tp"], out["nref"], out["ntest"])) == [(1, 1, 1), (1, 1, 1), (0, 0, 0)]
    with pytest.raises(ValueError, match="row 2 "):
        cr.keys(cr.cells(R3), cr.cells(["ACGU--", "A-GU--", "--CGUA"]))


def _random(seed, n, len_r):
    rs = np.random.RandomState(seed)
    len_t = len_r + 5
    cell_r, cell_t = np.full((n, len_r), 5, int), np.full((n, len_t), 5, int)
    for r in range(n):
        at = np.nonzero(rs.rand(len_r) >= 0.3)[0]
        codes = rs.randint(0, 5, len(at))
        cell_r[r, at] = codes
        cell_t[r, np.sort(rs.choice(len_t, len(at), replace=False)) if r % 2 else at + rs.randint(0, 6)] = codes
    return cell_r.tolist(), cell_t.tolist(), (rs.rand(len_r) < 0.8).tolist(), (rs.rand(len_t) < 0.8).tolist()


@pytest.mark.parametrize("seed", range(6))
def test_pair_counts_sum_to_the_row_counts(seed):
    """the two routes of the restatement: pairs from their definition, rows from k, m and cnt"""
    cell_r, cell_t, use_r, use_t = _random(seed, 4 + seed, 20 + 7 * seed)
    masks = (use_r, use_t) if seed % 2 else (None, None)
    out = cr.compare(cell_r, cell_t, *masks)
    for name, matrix in zip(("shared", "refp", "testp"), cr.pair_counts(cr.keys(cell_r, cell_t, *masks))):
        assert [sum(row) for row in matrix] == out[name], name
        assert all(matrix[r][r] == 0 and matrix[r][s] == matrix[s][r] for r in range(len(matrix)) for s in range(len(matrix)))
    assert sum(out["colshared"]) == out["total_shared"] and sum(out["colref"]) == out["total_refp"]
    assert 0 < out["total_shared"] < out["total_refp"]


def test_row_matching_and_its_refusals():
    ref_row, test_row = capi.compare_match(["a desc", "b", "c", "d"], ["d", "x", "a"])
    assert ref_row.tolist() == [0, 3] and test_row.tolist() == [2, 0]
    for ref, test, word in ((["a", "a", "b"], ["a", "b"], "reference"), (["a", "b"], ["b", "b x", "a"], "test")):
        with pytest.raises(ValueError, match="on two rows of the %s alignment" % word):
            capi.compare_match(ref, test)
    for test in (["b", "q"], ["q", "r"]):
        with pytest.raises(ValueError, match="needs two at least"):
            capi.compare_match(["a", "b"], test)


def test_pp_reader(tmp_path):
    names, rows = ["s1", "s2", "s3"], ["AC-GU-A", "A--GUCA", "-C-GU-A"]
    rel = [[0.96, 0.5, 0.04, 0.949, 0.3], [0.1, 0.2, 0.3, 0.4, 0.5], [1.0, 0.0, 0.55, 0.65]]
    text = stockholm.block(None, names, rows, rel, [0.5] * 7, "(.....)")
    path = tmp_path / "a.sto"
    path.write_text(text)
    got = stockholm.read_seed_pp(str(path))
    want = []
    for row, values in zip(rows, rel):
        it = iter(values)
        want.append("".join(stockholm.pp_char(next(it)) if ch != "-" else "." for ch in row))
    # column 2 (0-based) is all-gap: the seed reader drops it, and so does the PP reader
    assert stockholm.read_seed(str(path))[1] == [r[:2] + r[3:] for r in rows]
    assert got == [w[:2] + w[3:] for w in want]
    assert capi.encode_pp(got).tolist()[0] == [10, 5, 0, 9, 255, 3]
    plain = tmp_path / "b.sto"
    plain.write_text("# STOCKHOLM 1.0\ns1 ACGU\ns2 AC-U\n//\n")
    assert stockholm.read_seed_pp(str(plain)) is None
    fasta = tmp_path / "c.fa"
    fasta.write_text(">s1\nACGU\n>s2\nAC-U\n")
    assert stockholm.read_seed_pp(str(fasta)) is None
    short = tmp_path / "d.sto"
    short.write_text("# STOCKHOLM 1.0\ns1 ACGU\n#=GR s1 PP 99*\ns2 AC-U\n//\n")
    with pytest.raises(stockholm.SeedError, match="PP line of s1 has 3 columns"):
        stockholm.read_seed_pp(str(short))


def _u64(a):
    return np.ascontiguousarray(a, np.uint64)


def test_table_writers_equal_the_restatement():
    cell_r, cell_t, use_r, use_t = _random(3, 6, 30)
    rs = np.random.RandomState(1)
    pp = np.where(np.array(cell_t) <= 4, rs.randint(0, 11, np.array(cell_t).shape), 255).tolist()
    ss_r, ss_t = cr.brackets("((..))" + "." * 24), cr.brackets("(((...)))" + "." * 26)
    names = ["row%d" % r for r in range(6)]
    for with_ss, with_pp in ((True, True), (False, False)):
        out = cr.compare(cell_r, cell_t, use_r, use_t, ss_r if with_ss else None, ss_t if with_ss else None, pp if with_pp else None)
        arrs = [_u64(out[k]) for k in ("shared", "refp", "testp")] + [_u64([out["total_shared"], out["total_refp"], out["total_testp"]]),
                                                                      _u64([out["tc_reproduced"], out["tc_columns"]])]
        ss_arrs = [_u64(out[k]) for k in ("tp", "nref", "ntest")] if with_ss else [None] * 3
        pp_arr = _u64(out["pp_residues"] + out["pp_ref"] + out["pp_shared"]) if with_pp else None
        res = np.array(out["residues"], np.uint32)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        text = capi.host_text(capi._compare_table, 6, capi.c_strings(names), 2, 1, 30, 35, res.ctypes.data, *[a.ctypes.data for a in arrs],
                              *[ptr(a) for a in ss_arrs], ptr(pp_arr))
        assert text == cr.table(names, 2, 1, out)
        assert text.startswith("# rows 6 only_ref 2 only_test 1 columns_ref 30 columns_test 35\n# pairs shared ")
        assert ("# structure tp " in text) == with_ss and ("# pp " in text) == with_pp
    k = np.array(out["k"], np.uint32)
    rep = np.array(out["reproduced"], np.uint8)
    colref, colshared = _u64(out["colref"]), _u64(out["colshared"])  # held while the library reads them
    text = capi.host_text(capi._compare_columns_table, 30, k.ctypes.data, colref.ctypes.data, colshared.ctypes.data, rep.ctypes.data)
    assert text == cr.columns_table(out) and len(text.splitlines()) == 30
    mats = cr.pair_counts(cr.keys(cell_r, cell_t, use_r, use_t))
    m32 = [np.array(m, np.uint32) for m in mats]
    text = capi.host_text(capi._compare_matrix_table, 6, capi.c_strings(names), *[m.ctypes.data for m in m32])
    assert text == cr.matrix_table(names, *mats) and len(text.splitlines()) == 15
    # a quotient without a denominator is written as nan
    zero = np.zeros((2, 2), np.uint32)
    assert capi.host_text(capi._compare_matrix_table, 2, capi.c_strings(["a", "b"]), zero.ctypes.data, zero.ctypes.data, zero.ctypes.data) == \
        "1\t2\ta\tb\t0\t0\t0\tnan\tnan\n"


def _refused(*args):
    r = subprocess.run([DAFS] + list(args), capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == ""
    return r.stderr.strip()


def _python_refusal(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


def test_refused_option_combinations():
    for opt in ("--compare", "--compare-ref", "--compare-columns", "--compare-matrix"):
        assert _refused(opt, "", "x.fa") == opt + " needs a file name"
    both = capi.compare_refusal(capi.CMP_NEEDS_REF)
    assert "--compare-ref" in both and _refused("--compare", "o", "x.fa") == both == _refused("--compare-ref", "r", "x.fa")
    needs = capi.compare_refusal(capi.CMP_NEEDS_COMPARE)
    assert _refused("--compare-columns", "c", "x.fa") == needs == _refused("--compare-matrix", "m", "x.fa")
    pairwise = capi.compare_refusal(capi.CMP_NO_PAIRWISE)
    assert "--pairwise" in pairwise and _refused("--pairwise", "--compare", "o", "--compare-ref", "r", "x.fa") == pairwise == \
        _python_refusal(lambda: pipeline.pairwise(["a", "b"], ["ACGU", "ACGU"], compare=(["a", "b"], ["ACGU", "ACGU"])))
    merged = capi.compare_refusal(capi.CMP_NEEDS_MERGED)
    assert "--seed-merged" in merged and _refused("--seed", "s", "--seed-each", "--compare", "o", "--compare-ref", "r", "x.fa") == merged == \
        _python_refusal(lambda: pipeline.add_each(["s"], ["ACGU"], ["n"], ["ACGU"], compare=(["s", "n"], ["ACGU", "ACGU"])))
    assert "16384" in capi.compare_refusal(capi.CMP_TOO_MANY_ROWS)
    # --describe accepts the --compare options alone, and still nothing that aligns
    assert _refused("--describe", os.path.join(ROOT, "no", "such", "file"), "--compare", "o", "--compare-ref", "r").startswith("--describe: cannot open ")
    assert _refused("--describe", "a.sto", "--compare", "o", "--compare-ref", "r", "-r", "2") == \
        "--describe reads a finished alignment: --refinement cannot be combined with --describe"
    assert _refused("--describe", "a.sto", "--compare", "o") == both
    with pytest.raises(ValueError):
        pipeline.compare(["a", "b"], ["AC", "AC"], ["a"], ["AC", "AC"])  # a name per row


def test_help_text():
    r = subprocess.run([DAFS, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--compare OUT", "--compare-ref REF", "--compare-columns OUT", "--compare-matrix OUT"):
        assert opt in r.stdout, opt


def test_symbols_resolve():
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("dafs_hip_alignment_compare", "dafs_host_compare_refusal", "dafs_host_compare_match", "dafs_host_seed_pp", "dafs_host_compare_table",
                 "dafs_host_compare_columns_table", "dafs_host_compare_matrix_table"):
        assert getattr(lib, name) is not None
    assert C.sizeof(capi.CompareOut) == 22 * C.sizeof(C.c_void_p)
