"""CPU tests of the seed's consensus structure: the readers (stockholm.read_seed_structure and the
command line's) against the restatements of structure_ref.py, dafs_host_row_constraint, the --seed-scores table with the
support columns, and what the command line refuses.  No device work: `dafs` reads the seed before it opens a device."""
import os
import subprocess

import numpy as np
import pytest

import structure_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = 0xFFFFFFFF

# two interleaved blocks; column 4 (1-based) is all-gap and carries the '<' of a pair, column 10 is all-gap and unpaired
STO = """# STOCKHOLM 1.0
#=GF ID test
a            GGA.AC
#=GR a PP    ******
b            GGA-AC
#=GC SS_cons <<-<..
#=GC RF      xxxxxx

a            UCC-
b            U.C.
#=GC SS_cons >>>~
//
"""
STO_RAW = "<<-<..>>>~"
# what `dafs` prints: the tree line, the SS_cons record, rows over several lines
AFA = """[ 0.5 a b ]
>SS_cons
((.[{A..
a}]))
> a
GGAUCACU
GAUCC
> b
GGAUCAC-
GAUCC
"""


def _write(tmp_path, name, text):
    p = os.path.join(str(tmp_path), name)
    with open(p, "w") as fh:
        fh.write(text)
    return p


def _dafs(args):
    assert os.path.exists(DAFS), "build() makes the dafs executable"
    return subprocess.run([DAFS] + args, capture_output=True, text=True, timeout=60)


def test_stockholm_two_blocks_and_dropped_pair(tmp_path):
    from dafs_amd import stockholm
    names, rows, raw = stockholm.parse_seed_structure(STO)
    assert names == ["a", "b"] and rows == ["GGA.ACUCC-", "GGA-ACU.C."] and raw == STO_RAW
    want_rows, want_ss = ref.clean(rows, raw)
    assert want_rows == ["GGAACUCC", "GGAACU-C"]
    # the pair 4 -> 7 (1-based) lost its left column; 1 -> 9 and 2 -> 8 moved left by one
    assert want_ss == [7, 6, NONE, NONE, NONE, NONE, NONE, NONE]
    got = stockholm.read_seed_structure(_write(tmp_path, "s.sto", STO))
    assert got[0] == names and got[1] == want_rows and got[2].dtype == np.uint32 and got[2].tolist() == want_ss
    # a pair that loses its right column goes as well
    n2, r2, ss2 = stockholm.clean_seed_structure(["a", "b"], ["GGA.ACUC.", "GGA-ACU-."], "<<-...>.>")
    assert r2 == ["GGAACUC", "GGAACU-"] and ss2.tolist() == ref.clean(["GGA.ACUC.", "GGA-ACU-."], "<<-...>.>")[1] == [NONE, 5] + [NONE] * 5
    # the old readers give what they gave
    assert stockholm.parse_seed(STO) == (names, rows)
    assert stockholm.read_seed(_write(tmp_path, "s2.sto", STO)) == (names, want_rows)


def test_aligned_fasta_four_kinds_and_letters(tmp_path):
    from dafs_amd import stockholm
    names, rows, raw = stockholm.parse_seed_structure(AFA)
    assert names == ["a", "b"] and raw == "((.[{A..a}]))" and rows == ["GGAUCACUGAUCC", "GGAUCAC-GAUCC"]
    got = stockholm.read_seed_structure(_write(tmp_path, "s.aln", AFA))
    assert got[1] == rows
    assert got[2].tolist() == ref.clean(rows, raw)[1] == [12, 11, NONE, 10, 9] + [NONE] * 8
    assert stockholm.read_seed(_write(tmp_path, "s2.aln", AFA)) == (names, rows)
    # all four kinds nested in one line; letters and , : _ ~ - . unpaired
    line = "(<[{,:_~-.Aa}]>)"
    rw = ["ACGUACGUACGUACGU"]
    _, _, ss = stockholm.clean_seed_structure(["x"], rw, line)
    assert ss.tolist() == ref.clean(rw, line)[1] == [15, 14, 13, 12] + [NONE] * 12


def test_seed_without_structure(tmp_path):
    from dafs_amd import stockholm
    plain = "# STOCKHOLM 1.0\na ACGU\nb AC-U\n//\n"
    assert stockholm.parse_seed_structure(plain)[2] is None
    names, rows, ss = stockholm.read_seed_structure(_write(tmp_path, "p.sto", plain))
    assert (names, rows) == stockholm.read_seed(_write(tmp_path, "p2.sto", plain)) and ss is None
    assert stockholm.parse_seed_structure("> a\nACGU\n")[2] is None
    # only the first alignment of a Stockholm file counts
    two = "# STOCKHOLM 1.0\na ACGU\n//\n# STOCKHOLM 1.0\na ACGU\n#=GC SS_cons (..)\n//\n"
    assert stockholm.parse_seed_structure(two)[2] is None


REFUSALS = [
    ("#=GC SS_cons ((..).", "never closed"),                # an unbalanced kind
    ("#=GC SS_cons (..)).", "closes nothing"),
    ("#=GC SS_cons (<..).", "never closed"),                # '<' is not closed by ')'
    ("#=GC SS_cons (...)", "5 columns, the rows have 6"),  # a length different from the rows'
    ("#=GC SS_cons (<.)>.", "cross"),                       # crossing once the kinds are merged
    ("#=GC SS_cons (.!.).", "holds '!'"),                   # anything else
]


@pytest.mark.parametrize("line,msg", REFUSALS)
def test_refusals_same_text_in_both_drivers(tmp_path, line, msg):
    from dafs_amd import stockholm
    path = _write(tmp_path, "bad.sto", "# STOCKHOLM 1.0\na ACGUAC\nb ACGUAC\n%s\n//\n" % line)
    with pytest.raises(stockholm.SeedError) as e:
        stockholm.read_seed_structure(path)
    assert msg in str(e.value)
    assert stockholm.read_seed(path)[1] == ["ACGUAC", "ACGUAC"]  # the reader without the structure takes the file
    with pytest.raises(ref.Refused):
        ref.clean(["ACGUAC", "ACGUAC"], line.split()[-1])
    new = _write(tmp_path, "new.fa", ">n\nACGU\n")
    r = _dafs(["--seed", path, "--seed-structure", new])
    assert r.returncode != 0 and r.stdout == "" and str(e.value) in r.stderr


def test_row_constraint_hand_made():
    from dafs_amd import capi
    N = NONE
    cases = [
        # (mask row, ss, residues): two nested pairs, both kept
        ([1] * 10, [9, 8, N, N, N, N, N, N, N, N], "GGAAAAAACC"),
        # the residue at the right end of the outer pair is missing: that pair stays free, the inner one is forced
        ([1, 1, 1, 1, 1, 1, 1, 1, 1, 0], [9, 8, N, N, N, N, N, N, N, N], "GGAAAAAAC"),
        # the residue at the left end is missing
        ([0, 1, 1, 1, 1, 1, 1, 1, 1, 1], [9, 8, N, N, N, N, N, N, N, N], "GAAAAAACC"),
        # a non-complementary pair (A.G) stays free
        ([1] * 10, [9, 8, N, N, N, N, N, N, N, N], "AGAAAAAACG"),
        # a pair 3 apart in the row stays free although its columns are 5 apart; 4 apart is forced
        ([1, 0, 0, 1, 1, 1, 1, 1], [5, N, N, N, N, N, N, N], "GAAC" + "AA"),
        ([1, 0, 1, 1, 1, 1, 1, 1], [5, N, N, N, N, N, N, N], "GAAAC" + "AA"),
        # CONTRAfold's alphabet has no T: A.T and G.T stay free, lower case pairs
        ([1] * 8, [7, 6, N, N, N, N, N, N], "AGAAAACT"),
        ([1] * 8, [7, 6, N, N, N, N, N, N], "GTAAAAAC"),
        ([1] * 8, [7, 6, N, N, N, N, N, N], "guAAAAgc"),
        # an empty structure
        ([1, 0, 1, 1], [N, N, N, N], "ACG"),
    ]
    want = ["((??????))", "?(??????)", "(??????)?", "?(??????)?", "??????", "(???)??", "?(????)?", "(??????)", "((????))", "???"]
    for (mask, ss, res), w in zip(cases, want):
        assert ref.row_constraint(mask, ss, res) == w, (mask, res)
        assert capi.row_constraint(mask, ss, res) == w, (mask, res)
    for a in "ACGUTNacgut-":
        for b in "ACGUTNacgut-":
            assert capi.fold_complementary(a, b) == ref.complementary(a, b)
    with pytest.raises(capi.DafsHipError):  # one residue too few for the mask
        capi.row_constraint([1, 1, 1], [N, N, N], "AC")
    with pytest.raises(capi.DafsHipError):  # a partner to the left
        capi.row_constraint([1, 1, 1], [N, 0, N], "ACG")
    rs = np.random.RandomState(5)
    for _ in range(200):
        L = int(rs.randint(1, 40))
        mask = (rs.rand(L) < 0.8).astype(np.uint8)
        ss = [N] * L
        free = list(range(L))
        rs.shuffle(free)
        lo, hi = 0, L - 1
        while hi - lo >= 1 and rs.rand() < 0.8:  # nested pairs from the outside in
            ss[lo] = hi
            lo += int(rs.randint(1, 3)); hi -= int(rs.randint(1, 3))
        res = "".join(rs.choice(list("ACGUT")) for _ in range(int(mask.sum())))
        assert capi.row_constraint(mask, ss, res) == ref.row_constraint(mask, ss, res)


class _Each:
    pass


def _each(lengths, matched, score, iterations, support=None):
    e = _Each()
    e.results = [None] * len(lengths)
    e.lengths, e.matched = np.array(lengths, np.uint32), np.array(matched, np.uint32)
    e.score, e.iterations = np.array(score, np.float32), np.array(iterations, np.int64)
    if support is not None:
        e.support = support
    return e


def test_seed_table_with_and_without_support():
    from dafs_amd import pipeline
    headers, lengths, matched = ["hit one", "hit", "hit"], [76, 9, 30], [70, 0, 30]
    score, iterations = [np.float32(12.3456789), np.float32(np.nan), np.float32(-0.5)], [37, 600, 1]
    plain = pipeline.seed_scores_tsv(headers, _each(lengths, matched, score, iterations))
    assert plain == "1\thit\t76\t70\t6\t12.3456793\t37\n2\thit.2\t9\t0\t9\tnan\t600\n3\thit.3\t30\t30\t0\t-0.5\t1\n"  # today's bytes
    sup = dict(both=np.array([21, 0, 7], np.uint32), canonical=np.array([20, 0, 7], np.uint32), half=np.array([0, 3, 1], np.uint32),
               expected=np.array([17.25, 0.0, 1.0 / 3.0]))
    got = pipeline.seed_scores_tsv(headers, _each(lengths, matched, score, iterations, sup))
    tails = ["\t21\t20\t0\t17.25", "\t0\t0\t3\t0", "\t7\t7\t1\t0.333333333"]
    assert got == "".join(a + b + "\n" for a, b in zip(plain.split("\n"), tails))
    bad = dict(sup, canonical=np.array([22, 0, 7], np.uint32))
    with pytest.raises(ValueError):  # more canonical pairs than pairs
        pipeline.seed_scores_tsv(headers, _each(lengths, matched, score, iterations, bad))


@pytest.mark.parametrize("opt,msg", [
    (["--bp-update1"], "--bp-update1 cannot be combined with --seed-structure"),
    (["-T", "0.3"], "-T and -G cannot be combined with --seed-structure"),
    (["-G", "4"], "-T and -G cannot be combined with --seed-structure"),
])
def test_cli_refuses_combinations(tmp_path, opt, msg):
    seed = _write(tmp_path, "s.sto", STO)
    new = _write(tmp_path, "new.fa", ">n\nACGU\n")
    for each in ([], ["--seed-each"]):
        r = _dafs(["--seed", seed, "--seed-structure"] + each + opt + [new])
        assert r.returncode != 0 and msg in r.stderr and r.stdout == ""


def test_cli_needs_seed_and_a_structure(tmp_path):
    new = _write(tmp_path, "new.fa", ">n\nACGU\n")
    r = _dafs(["--seed-structure", new])
    assert r.returncode != 0 and "--seed-structure needs --seed" in r.stderr and r.stdout == ""
    plain = _write(tmp_path, "p.sto", "# STOCKHOLM 1.0\na ACGU\nb AC-U\n//\n")
    for each in ([], ["--seed-each"]):
        r = _dafs(["--seed", plain, "--seed-structure"] + each + [new])
        assert r.returncode != 0 and "holds no SS_cons" in r.stderr and r.stdout == ""


def test_cli_help_names_the_option():
    r = _dafs(["--help"])
    assert "--seed-structure" in r.stdout + r.stderr
    assert "pairs canonical half expected" in r.stdout + r.stderr


def test_python_refuses_what_decodes(tmp_path):
    """seed_ss with bp_update1 or th_s1, and a structure that does not fit the seed, are refused before any device work"""
    from dafs_amd import pipeline
    N = NONE
    rows = ["GGAAAACC", "GGAAAACC"]
    for fn in (pipeline.add, pipeline.add_each):
        for kw in (dict(bp_update1=True), dict(th_s1=0.3)):
            with pytest.raises(ValueError, match="nothing is decoded"):
                fn(["a", "b"], rows, ["n"], ["ACGU"], seed_ss=[7, 6, N, N, N, N, N, N], **kw)
        with pytest.raises(ValueError, match="8 columns"):
            fn(["a", "b"], rows, ["n"], ["ACGU"], seed_ss=[N, N, N])
        with pytest.raises(ValueError, match="no structure"):
            fn(["a", "b"], rows, ["n"], ["ACGU"], seed_ss=[7, 7, N, N, N, N, N, N])


def test_library_exports():
    import ctypes
    from dafs_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ("dafs_host_seed_parse_structure", "dafs_host_seed_clean_structure", "dafs_host_row_constraint", "dafs_host_seed_table_support",
                "dafs_hip_fold_posteriors_constrained_begin", "dafs_hip_fold_posteriors_constrained", "dafs_hip_structure_support"):
        assert hasattr(lib, sym)
