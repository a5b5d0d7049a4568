"""CPU tests of the alignment statistics: the known answers of the definitions against the restatement
in tests/alistat_ref.py, the cell encoder, dafs_host_nr_select, the text writers, and the refusals and help text of the
command line."""
import math
import os
import subprocess

import numpy as np
import pytest

import alistat_ref as ar
from dafs_amd import capi, pipeline, stockholm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = ar.NONE


def test_known_answers():
    cell = ar.cells(["ACGU-", "AC-UN", "-CGUA"])
    res, ident, aligned = ar.counts(cell)
    assert res == [4, 4, 4]
    assert (aligned[0][1], ident[0][1]) == (3, 3) and (aligned[0][2], ident[0][2]) == (3, 3) and (aligned[1][2], ident[1][2]) == (3, 2)
    assert [float(ident[r][s]) / float(min(res[r], res[s])) for r, s in ((0, 1), (0, 2), (1, 2))] == [0.75, 0.75, 0.5]
    assert (aligned[0][0], ident[0][0], aligned[1][1], ident[1][1]) == (4, 4, 4, 3)  # the diagonal: res, and the cells with a base
    assert ar.nearest(res, ident)[0] == [1, 0, 0]  # row 0's tie goes to the smaller index
    assert ar.summary(res, ident) == (2.0 / 3.0, 0.5, 0.75)
    assert capi.identity_summary(np.array(ident, np.uint32), res) == (2.0 / 3.0, 0.5, 0.75)
    cell = ar.cells(["AC", "AG", "UG"])
    assert ar.v_sums(cell) == [0.75, 0.5, 0.75] and ar.weights(cell) == [1.125, 0.75, 1.125]
    assert ar.weights(ar.cells(["ACGU"])) == [1.0] and all(math.isnan(x) for x in ar.summary([4], [[4]]))
    assert all(math.isnan(x) for x in capi.identity_summary(np.array([[4]], np.uint32), [4]))
    with pytest.raises(ValueError):
        ar.counts(ar.cells(["AC", "--"]))
    # the order is the integers': 2/3 beats 3/5, and 2/4 ties 1/2
    assert ar.more_identical(2, 3, 3, 5) and not ar.more_identical(2, 4, 1, 2) and not ar.more_identical(1, 2, 2, 4)
    # the threshold: one multiplication, one comparison
    assert ar.redundant(3, 4, 0.75) and not ar.redundant(2, 4, 0.75) and ar.redundant(9, 10, 0.9) == (9.0 >= 0.9 * 10.0)


def test_encode_cells():
    assert capi.encode_cells(["ACGUTacgut", "NRYnry-.-."]).tolist() == [[0, 1, 2, 3, 3, 0, 1, 2, 3, 3], [4, 4, 4, 4, 4, 4, 5, 5, 5, 5]]
    assert capi.encode_cells([b"AC-"]).tolist() == ar.cells(["AC-"])
    every = "".join(chr(c) for c in range(256) if chr(c).isascii() and (chr(c).isalpha() or chr(c) in "-."))
    assert capi.encode_cells([every]).tolist() == ar.cells([every])
    for bad in ("AC1", "AC ", "AC*", "AC~"):
        with pytest.raises(ValueError):
            capi.encode_cells([bad])
    with pytest.raises(ValueError):
        capi.encode_cells(["AC", "A"])
    with pytest.raises(ValueError):
        capi.encode_cells([])
    # gaps are not N: encode_alignment (section 13) keeps merging them
    assert capi.encode_alignment(["AN-"]).tolist() == [[0, 4, 4]]


def _bits(pairs, n):
    red = [[False] * n for _ in range(n)]
    for r, s in pairs:
        red[r][s] = red[s][r] = True
    return red


def _select(red, rank, forced=None):
    kept, by = capi.nr_select(np.array(ar.red_bits(red), np.uint32), rank, forced)
    want = ar.nr_select(red, list(rank), forced)
    assert kept.tolist() == want[0] and by.tolist() == want[1]
    return kept.tolist(), by.tolist()


def test_nr_select():
    # forced rows that are redundant with each other are both kept
    red = _bits([(0, 1), (1, 2)], 4)
    assert _select(red, [0, 1, 2, 3], [1, 1, 0, 0]) == ([True, True, False, True], [NONE, NONE, 1, NONE])
    # a chain a~b~c with a first keeps a and c
    assert _select(red, [0, 1, 2, 3]) == ([True, False, True, True], [NONE, 0, NONE, NONE])
    assert _select(red, [1, 0, 2, 3]) == ([False, True, False, True], [1, NONE, 1, NONE])
    # by names the first remover in visiting order, not the smallest index
    red = _bits([(0, 3), (2, 3)], 4)
    assert _select(red, [2, 0, 1, 3]) == ([True, True, True, False], [NONE, NONE, NONE, 2])
    assert _select(red, [0, 2, 1, 3]) == ([True, True, True, False], [NONE, NONE, NONE, 0])
    # a forced row removes later rows, and a row over a word edge
    n = 70
    red = _bits([(0, 69), (33, 64), (5, 6)], n)
    forced = [r in (69, 6) for r in range(n)]
    kept, by = _select(red, list(range(n)), forced)
    assert kept[69] and kept[6] and not kept[64] and by[64] == 33 and sum(kept) == n - 1
    rank = [int(x) for x in np.random.RandomState(3).permutation(n)]
    _select(red, rank, forced)
    # a rank that is not a permutation is refused, with the library's message
    for bad in ([0, 1, 1, 3], [0, 1, 2, 4], [0, 1, 2]):
        with pytest.raises(ValueError, match="not a permutation"):
            capi.nr_select(np.array(ar.red_bits(_bits([], 4)), np.uint32), bad)
    with pytest.raises(ValueError):
        capi.nr_select(np.zeros((4, 2), np.uint32), [0, 1, 2, 3])
    # every refusal of the library call carries its own message, never an earlier call's
    kept, by = np.zeros(4, np.uint8), np.zeros(4, np.uint32)
    assert capi._nr_select(4, None, None, None, kept.ctypes.data, by.ctypes.data) == -1
    assert capi._last_error().decode().startswith("nr_select: no rows")


class _Identity:
    pass


def _known():
    idn = _Identity()
    cell = ar.cells(["ACGU-", "AC-UN", "-CGUA"])
    res, ident, aligned = ar.counts(cell)
    idn.res, idn.ident, idn.aligned = np.array(res, np.uint32), np.array(ident, np.uint32), np.array(aligned, np.uint32)
    near, ni, nd = ar.nearest(res, ident)
    idn.nearest, idn.nearest_ident, idn.nearest_den = np.array(near, np.uint32), np.array(ni, np.uint32), np.array(nd, np.uint32)
    idn.weights = np.array(ar.weights(cell))
    idn.summary = ar.summary(res, ident)
    idn.columns = 5
    return idn


def test_identity_tables():
    idn = _known()
    w = ["%.9g" % x for x in idn.weights]
    assert pipeline.identity_tsv(["a", "b", "c"], idn) == ("# rows 3 columns 5 average 0.666666667 min 0.5 max 0.75\n"
                                                         "1\ta\t4\t%s\t2\tb\t0.75\n2\tb\t4\t%s\t1\ta\t0.75\n3\tc\t4\t%s\t1\ta\t0.75\n" % tuple(w))
    assert pipeline.identity_matrix_tsv(["a", "b", "c"], idn) == "1\t2\ta\tb\t3\t3\t4\t0.75\n1\t3\ta\tc\t3\t3\t4\t0.75\n2\t3\tb\tc\t2\t3\t4\t0.5\n"
    # a single row: no nearest row, NaN everywhere
    one = _Identity()
    one.res, one.weights, one.nearest = np.array([4], np.uint32), np.array([1.0]), np.array([NONE], np.uint32)
    one.nearest_ident = one.nearest_den = np.array([0], np.uint32)
    one.ident = one.aligned = np.array([[4]], np.uint32)
    one.summary, one.columns = (math.nan,) * 3, 4
    assert pipeline.identity_tsv(["x"], one) == "# rows 1 columns 4 average nan min nan max nan\n1\tx\t4\t1\t0\t-\tnan\n"
    assert pipeline.identity_matrix_tsv(["x"], one) == ""
    with pytest.raises(ValueError):
        pipeline.identity_tsv(["a", "b"], idn)


BLOCK = "# STOCKHOLM 1.0\n#=GF CC [ 0.5 a b ]\na             ACGU\n#=GR a PP     9999\nb             AC-U\n#=GR b PP     99.9\n#=GC SS_cons  ....\n//\n"


def test_weight_lines_and_the_nr_block():
    got = stockholm.with_weights(BLOCK, ["a", "b"], [1.5, 0.123456789])
    lines = BLOCK.split("\n")
    assert got.split("\n") == lines[:2] + ["#=GS a WT 1.500000", "#=GS b WT 0.123457"] + lines[2:]
    # no #=GF line: directly after the first line
    bare = BLOCK.replace("#=GF CC [ 0.5 a b ]\n", "")
    assert stockholm.with_weights(bare, ["a", "b"], [1, 1]).split("\n")[:3] == ["# STOCKHOLM 1.0", "#=GS a WT 1.000000", "#=GS b WT 1.000000"]
    with pytest.raises(ValueError):
        stockholm.with_weights("a ACGU\n", ["a"], [1.0])
    with pytest.raises(ValueError):
        stockholm.with_weights(BLOCK, ["a", "b"], [1.0])
    # the writers print what they print today without the weights
    rel = [np.full(4, 0.99), np.full(3, 0.99)]
    plain = stockholm.block("[ 0.5 a b ]", ["a", "b"], ["ACGU", "AC-U"], rel, np.full(4, 0.99), "....")
    assert stockholm.block("[ 0.5 a b ]", ["a", "b"], ["ACGU", "AC-U"], rel, np.full(4, 0.99), "....", weights=None) == plain
    assert stockholm.block("[ 0.5 a b ]", ["a", "b"], ["ACGU", "AC-U"], rel, np.full(4, 0.99), "....", weights=[1.5, 0.5]) == \
        stockholm.with_weights(plain, ["a", "b"], [1.5, 0.5])
    kept = np.array([1, 0], np.uint8)
    nr = capi.host_text(capi._stockholm_nr, bare.encode(), 2, capi.c_strings(["a", "b"]), kept.ctypes.data, 1, 0.9)
    assert nr == "# STOCKHOLM 1.0\n#=GF CC nr 0.9 kept 0 of 1 hits\na             ACGU\n#=GR a PP     9999\n#=GC SS_cons  ....\n//\n"
    kept[:] = 1
    nr = capi.host_text(capi._stockholm_nr, bare.encode(), 2, capi.c_strings(["a", "b"]), kept.ctypes.data, 1, 0.75)
    assert nr == bare.replace("1.0\n", "1.0\n#=GF CC nr 0.75 kept 1 of 1 hits\n", 1)


class _Each:
    pass


def test_seed_table_with_and_without_the_nearest_row():
    each = _Each()
    each.results = [None, None]
    each.lengths, each.matched = np.array([60, 45], np.uint32), np.array([58, 0], np.uint32)
    each.score, each.iterations = np.array([12.5, -1.25], np.float32), np.array([17, 600], np.int64)
    names = ["n0 with a head", "n1"]
    old = pipeline.seed_scores_tsv(names, each)
    arrs = [np.ascontiguousarray(a, t) for a, t in ((each.lengths, np.uint32), (each.matched, np.uint32), (each.score, np.float64), (each.iterations, np.int64))]
    assert old == capi.host_text(capi._seed_table, 2, capi.c_strings(names), *[a.ctypes.data for a in arrs])  # byte-equal to dafs_host_seed_table's
    assert old == "1\tn0\t60\t58\t2\t12.5\t17\n2\tn1\t45\t0\t45\t-1.25\t600\n"
    each.nearest = _Each()
    each.nearest.names, each.nearest.row, each.nearest.pid = ["s0", "s1"], np.array([1, NONE], np.uint32), np.array([0.75, math.nan])
    assert pipeline.seed_scores_tsv(names, each) == "1\tn0\t60\t58\t2\t12.5\t17\ts1\t0.75\n2\tn1\t45\t0\t45\t-1.25\t600\t-\tnan\n"
    each.support = dict(both=[9, 0], canonical=[8, 0], half=[1, 0], expected=[7.5, 0.0])
    assert pipeline.seed_scores_tsv(names, each) == "1\tn0\t60\t58\t2\t12.5\t17\t9\t8\t1\t7.5\ts1\t0.75\n2\tn1\t45\t0\t45\t-1.25\t600\t0\t0\t0\t0\t-\tnan\n"
    del each.nearest
    assert pipeline.seed_scores_tsv(names, each) == "1\tn0\t60\t58\t2\t12.5\t17\t9\t8\t1\t7.5\n2\tn1\t45\t0\t45\t-1.25\t600\t0\t0\t0\t0\n"


def _refused(*args):
    r = subprocess.run([DAFS] + list(args), capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and r.stdout == ""
    return r.stderr.strip()


def _python_refusal(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


def test_command_line_refusals():
    assert _refused("--identity", "", "x.fa") == "--identity needs a file name"
    assert _refused("--identity-matrix", "", "x.fa") == "--identity-matrix needs a file name"
    assert _refused("--describe", "", "--identity", "o") == "--describe needs a file name"
    assert _refused("--identity-matrix", "m", "x.fa") == "--identity-matrix needs --identity"
    # the three refusals that exist in both drivers: one text, from the library
    assert _refused("--pairwise", "--identity", "o", "x.fa") == capi.alistat_refusal(capi.NO_PAIRWISE) == \
        _python_refusal(lambda: pipeline.pairwise(["a", "b"], ["ACGU", "ACGU"], identity=True))
    assert "--pairwise" in capi.alistat_refusal(capi.NO_PAIRWISE) and "--identity" in capi.alistat_refusal(capi.NO_PAIRWISE)
    assert _refused("--seed", "s", "--seed-each", "--identity", "o", "x.fa").startswith("--seed-each: --identity cannot be combined with --seed-each")
    assert _refused("--seed", "s", "--seed-each", "--seed-nearest", "x.fa") == "--seed-nearest needs --seed-each and --seed-scores"
    assert _refused("--seed", "s", "--seed-scores", "t", "--seed-nearest", "x.fa") == "--seed-nearest needs --seed-each and --seed-scores"
    assert _refused("--seed-nearest", "x.fa") == "--seed-nearest needs --seed-each and --seed-scores"
    assert _refused("--seed", "s", "--seed-each", "--seed-nr", "0.9", "x.fa") == capi.alistat_refusal(capi.NR_NEEDS_MERGED) == \
        _python_refusal(lambda: pipeline.add_each(["s"], ["ACGU"], ["n"], ["ACGU"], nr=0.9))
    assert "--seed-nr" in capi.alistat_refusal(capi.NR_NEEDS_MERGED) and "--seed-merged" in capi.alistat_refusal(capi.NR_NEEDS_MERGED)
    for bad in ("0", "1.5", "-0.1", "nan", "x", "0.9x", ""):
        assert _refused("--seed-nr", bad, "x.fa") == capi.alistat_refusal(capi.NR_THRESHOLD)
    for bad in (0.0, 1.5, -0.1, float("nan")):
        assert _python_refusal(lambda: pipeline.add_each(["s"], ["ACGU"], ["n"], ["ACGU"], merged=True, nr=bad)) == capi.alistat_refusal(capi.NR_THRESHOLD)
    assert "(0, 1]" in capi.alistat_refusal(capi.NR_THRESHOLD)
    assert _refused("--describe", "a.sto") == "--describe needs --identity or --covariation"
    assert _refused("--describe", "a.sto", "--identity", "o", "x.fa") == "--describe takes no FILE: the alignment is its argument"
    for opt, name in ((["-r", "2"], "refinement"), (["--seed", "s"], "seed"), (["--stockholm", "s"], "stockholm"), (["--pairwise"], "pairwise"),
                      (["-a", "CONTRAlign"], "align-model"), (["--devices", "0,1"], "devices"), (["-t", "0.3"], "fold-th")):
        assert _refused("--describe", "a.sto", "--identity", "o", *opt) == \
            "--describe reads a finished alignment: --%s cannot be combined with --describe" % name
    # the alignment itself is read by the seed reader, before a device is touched
    assert _refused("--describe", os.path.join(ROOT, "no", "such", "file"), "--identity", "o").startswith("--describe: cannot open ")
    # more than 32768 rows: the summary's matrix is beyond the library's limit, said in words by both drivers
    assert "32768" in capi.alistat_refusal(capi.TOO_MANY_ROWS)
    assert _python_refusal(lambda: pipeline.alignment_identity(None, ["A"] * 32769)) == capi.alistat_refusal(capi.TOO_MANY_ROWS)


def test_help_text():
    r = subprocess.run([DAFS, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for opt in ("--identity OUT", "--identity-matrix OUT", "--seed-nearest", "--seed-nr T", "--describe ALIGNMENT"):
        assert opt in r.stdout, opt
