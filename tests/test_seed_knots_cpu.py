"""CPU tests of a seed structure whose pairs may cross: the reader with levels
(stockholm.clean_seed_knots / read_seed_knots and the command line's --knots) against the restatements of knots_ref.py, the
round trip of a `Levels` bracket line, dafs_host_row_constraint_levels, and what is refused.  No device work: `dafs` reads its
files and options before it opens a device."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import knots_ref as ref
import levels_ref
import structure_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE, FREE = 0xFFFFFFFF, 0xFF


def _write(tmp_path, name, text):
    p = os.path.join(str(tmp_path), name)
    with open(p, "w") as fh:
        fh.write(text)
    return p


def _dafs(args):
    assert os.path.exists(DAFS), "build() makes the dafs executable"
    return subprocess.run([DAFS] + args, capture_output=True, text=True, timeout=60)


def _row(n):
    return ("ACGU" * n)[:n]


def _read(line, rows=None):
    """(ss, level) of the new reader on rows (default: one row without gaps), checked against the restatement"""
    from dafs_amd import stockholm
    rows = [_row(len(line))] if rows is None else rows
    names = ["r%d" % k for k in range(len(rows))]
    got_names, got_rows, ss, level = stockholm.clean_seed_knots(names, rows, line)
    want_rows, want_ss, want_level = ref.clean(rows, line)
    assert got_names == names and got_rows == want_rows
    assert ss.dtype == np.uint32 and level.dtype == np.uint8
    assert ss.tolist() == want_ss and level.tolist() == want_level
    return ss.tolist(), level.tolist()


def _levels(pairs_by_level, L):
    lv = [FREE] * L
    for k, prs in enumerate(pairs_by_level):
        for i, j in prs:
            lv[i] = lv[j] = k
    return lv


def test_crossing_kinds_are_read_and_still_refused_by_the_old_reader():
    from dafs_amd import stockholm
    ss, level = _read("(<.)>.")
    assert ss == [3, 4, NONE, NONE, NONE, NONE] and level == _levels([[(0, 3)], [(1, 4)]], 6)  # "<>" is the later group: level 1
    with pytest.raises(stockholm.SeedError, match="cross"):
        stockholm.clean_seed_structure(["a"], [_row(6)], "(<.)>.")
    with pytest.raises(structure_ref.Refused):
        structure_ref.clean([_row(6)], "(<.)>.")


def test_letters_are_a_level():
    from dafs_amd import stockholm
    line = "((..AA..))..aa"
    ss, level = _read(line)
    assert ss == [9, 8, NONE, NONE, 13, 12] + [NONE] * 8
    assert level == _levels([[(0, 9), (1, 8)], [(4, 13), (5, 12)]], 14)
    # the old reader takes the letters as unpaired
    old = stockholm.clean_seed_structure(["a"], [_row(14)], line)[2].tolist()
    assert old == [9, 8] + [NONE] * 12
    # letters that nest inside the brackets share level 0; two letters that cross one another take two levels
    assert _read("((.Aa.))")[1] == _levels([[(0, 7), (1, 6), (3, 4)]], 8)
    assert _read("A.B.a.b")[1] == _levels([[(0, 4)], [(2, 6)]], 7)


def test_nested_wuss_is_all_level_0_and_the_old_reader():
    from dafs_amd import stockholm
    for line in ("<<((..))>>", "(<[{,:_~-..}]>)", "((..))..<<..>>", "....", "<.>"):
        ss, level = _read(line)
        old = stockholm.clean_seed_structure(["a"], [_row(len(line))], line)[2].tolist()
        assert ss == old
        assert level == [0 if (p != NONE or c in ss) else FREE for c, p in enumerate(ss)]


def test_the_seven_column_knot_and_three_levels():
    ss, level = _read("(.[.).]")
    assert ss == [4, NONE, 6, NONE, NONE, NONE, NONE] and level == [0, FREE, 1, FREE, 0, FREE, 1]
    # three levels: "[]" crosses "()", "{}" crosses both
    line = "(..[{)......].}."
    ss, level = _read(line)
    assert ss[0] == 5 and ss[3] == 12 and ss[4] == 14
    assert level == _levels([[(0, 5)], [(3, 12)], [(4, 14)]], 16)
    # a group takes the lowest level it fits: "{}" crosses "[]" but not "()", and goes to level 0 beside "()"
    assert _read("(.[.{.).].}")[1] == _levels([[(0, 6)], [(2, 8)], [(4, 10)]], 11)
    assert _read("(.).[.{.].}")[1] == _levels([[(0, 2), (4, 8)], [(6, 10)]], 11)
    assert _read("(.[.).].{.}")[1] == _levels([[(0, 4), (8, 10)], [(2, 6)]], 11)
    # four levels, letters among them
    assert _read("(.[.{.A.).].}.a")[1] == _levels([[(0, 8)], [(2, 10)], [(4, 12)], [(6, 14)]], 15)


def test_a_dropped_pair_lets_a_group_fall_to_level_0():
    # column 0 is all-gap and carries the '(' of the only level-0 pair: the pair goes before the levels are assigned, and "[]"
    # crosses nothing any more
    rows = ["-ACGUACG", ".ACGUACG"]
    from dafs_amd import stockholm
    _, got_rows, ss, level = stockholm.clean_seed_knots(["a", "b"], rows, "(.[.).].")
    want_rows, want_ss, want_level = ref.clean(rows, "(.[.).].")
    assert got_rows == want_rows == ["ACGUACG", "ACGUACG"]
    assert ss.tolist() == want_ss == [NONE, 5, NONE, NONE, NONE, NONE, NONE]
    assert level.tolist() == want_level == [FREE, 0, FREE, FREE, FREE, 0, FREE]
    # with the column present the same line has two levels
    assert _read("(.[.).].", ["GACGUACG", "GACGUACG"])[1] == [0, FREE, 1, FREE, 0, FREE, 1, FREE]


FIVE = "(.[.{.<.A.).].}.>.a"

REFUSALS = [
    (FIVE, "'A' 'a' pairs"),                     # five mutually crossing groups: the fifth is named
    ("((..).a", "closes nothing"),               # a lower-case letter that closes nothing
    ("A.....)", "closes nothing"),
    ("(A...).", "never closed"),                 # an upper-case letter never closed
    ("((...).", "never closed"),
    ("(<...).", "never closed"),                 # '<' is not closed by ')'
    ("(....)", "6 columns, the rows have 7"),    # a wrong length
    ("(.!..).", "holds '!'"),                    # any other character
    ("(.1..).", "holds '1'"),
]


@pytest.mark.parametrize("line,msg", REFUSALS)
def test_refusals_same_text_in_both_drivers(tmp_path, line, msg):
    from dafs_amd import stockholm
    width = 19 if line == FIVE else 7
    path = _write(tmp_path, "bad.sto", "# STOCKHOLM 1.0\na %s\nb %s\n#=GC SS_cons %s\n//\n" % (_row(width), _row(width), line))
    with pytest.raises(stockholm.SeedError) as e:
        stockholm.read_seed_knots(path)
    assert msg in str(e.value)
    with pytest.raises(structure_ref.Refused):
        ref.clean([_row(width)] * 2, line)
    new = _write(tmp_path, "new.fa", ">n\nACGU\n")
    # (the reference of --compare-ref is read when the first alignment is compared: test_seed_knots_gpu.py)
    for args in (["--seed", path, "--seed-structure", "--knots", new], ["--describe", path, "--knots", "--identity", os.path.join(str(tmp_path), "i.tsv")]):
        r = _dafs(args)
        assert r.returncode != 0 and r.stdout == "" and str(e.value) in r.stderr, args


def test_the_old_texts_where_the_case_is_the_same(tmp_path):
    """an unbalanced bracket, a wrong length and a foreign character read the same from both readers"""
    from dafs_amd import stockholm
    for line in ("((..).", "(..)).", "(...)", "(.!.)."):
        texts = []
        for fn in (stockholm.clean_seed_structure, stockholm.clean_seed_knots):
            with pytest.raises(stockholm.SeedError) as e:
                fn(["a"], ["ACGUAC"], line)
            texts.append(str(e.value))
        assert texts[0] == texts[1]


def test_read_seed_knots_files(tmp_path):
    from dafs_amd import stockholm
    sto = "# STOCKHOLM 1.0\na GGA.ACAAUCC\nb GGA-ACAAU.C\n#=GC SS_cons ((.-[[.))]]\n//\n"
    names, rows, ss, level = stockholm.read_seed_knots(_write(tmp_path, "k.sto", sto))
    want_rows, want_ss, want_level = ref.clean(["GGA.ACAAUCC", "GGA-ACAAU.C"], "((.-[[.))]]")
    assert names == ["a", "b"] and rows == want_rows and ss.tolist() == want_ss and level.tolist() == want_level
    plain = "# STOCKHOLM 1.0\na ACGU\nb AC-U\n//\n"
    got = stockholm.read_seed_knots(_write(tmp_path, "p.sto", plain))
    assert got[:2] == stockholm.read_seed(_write(tmp_path, "p2.sto", plain)) and got[2] is None and got[3] is None


def test_levels_output_round_trips():
    """the brackets of a `Levels` decode, read with the new reader, give the decode's ss and level again"""
    from dafs_amd import capi, stockholm
    for case in levels_ref.hand_cases():
        text = capi.make_brackets_levels(case.ss, case.level)
        assert text == case.text
        L = len(case.ss)
        _, _, ss, level = stockholm.clean_seed_knots(["x"], [_row(L)], text)
        assert ss.tolist() == case.ss.tolist() and level.tolist() == case.level.tolist(), case.name
        assert capi.make_brackets_levels(ss, level) == text


def test_nested_structures_read_as_the_old_reader_reads_them():
    from dafs_amd import stockholm
    rs = np.random.RandomState(26)
    for _ in range(50):
        L = int(rs.randint(1, 60))
        line, stack = [], []
        for c in range(L):
            u = rs.rand()
            if u < 0.3:
                k = int(rs.randint(0, 4))
                stack.append(k)
                line.append("(<[{"[k])
            elif u < 0.6 and stack:
                line.append(")>]}"[stack.pop()])
            else:
                line.append(".,:_-~Aa"[int(rs.randint(0, 6))])
        line = "".join(line) + "".join(")>]}"[k] for k in reversed(stack))
        rows = ["".join(ch if rs.rand() < 0.8 else "-" for ch in _row(len(line))) for _ in range(2)]
        rows = [r if r.strip("-") else "A" + r[1:] for r in rows]
        old = stockholm.clean_seed_structure(["a", "b"], rows, line)
        new = stockholm.clean_seed_knots(["a", "b"], rows, line)
        assert new[1] == old[1] and new[2].tolist() == old[2].tolist()
        paired = set(c for c, p in enumerate(old[2].tolist()) if p != NONE) | set(p for p in old[2].tolist() if p != NONE)
        assert new[3].tolist() == [0 if c in paired else FREE for c in range(len(old[2]))]


N = NONE
HAND_ROWS = [
    # (mask row, ss, level, K, residues, want)
    # the seven-column knot on GAGACAC: both pairs 4 apart and complementary (G.C, G.C)
    ([1] * 7, [4, N, 6, N, N, N, N], [0, FREE, 1, FREE, 0, FREE, 1], 2, "GAGACAC", ["(?.?)?.", ".?(?.?)"]),
    # an H-type: level 0 (0,9) (1,8), level 1 (4,13) (5,12)
    ([1] * 14, [9, 8, N, N, 13, 12] + [N] * 8, [0, 0, FREE, FREE, 1, 1, FREE, FREE, 0, 0, FREE, FREE, 1, 1], 2, "GGAAGCAACCAAGC",
     ["((??..??))??..", "..??((??..??))"]),
    # half-held pairs stay '?' in every string: the right residue of (1,8) and the left residue of (5,12) are missing
    ([1, 1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1], [9, 8, N, N, 13, 12] + [N] * 8, [0, 0, FREE, FREE, 1, 1, FREE, FREE, 0, 0, FREE, FREE, 1, 1], 2,
     "GGAAGAACAAGC", ["(???.??)???.", ".???(??.???)"]),
    # A.G at (1,8): free in its own level, '.' in the other (complementary or not)
    ([1] * 14, [9, 8, N, N, 13, 12] + [N] * 8, [0, 0, FREE, FREE, 1, 1, FREE, FREE, 0, 0, FREE, FREE, 1, 1], 2, "GAAAGCAAGCAAGC",
     ["(???..???)??..", "..??((??..??))"]),
    # T is no U: (0,9) G.T and (4,13) A.T stay free in their own strings
    ([1] * 14, [9, 8, N, N, 13, 12] + [N] * 8, [0, 0, FREE, FREE, 1, 1, FREE, FREE, 0, 0, FREE, FREE, 1, 1], 2, "GGAAAGAACTAACT",
     ["?(??..??)???..", "..???(??..??)?"]),
    # a level-1 pair 3 apart in the row stays free although its columns are 4 apart, and the string is then empty; 4 apart it is forced
    ([1, 1, 1, 0, 1, 1, 1, 1, 1, 1], [8, N, 6, N, N, N, N, N, N, N], [0, FREE, 1, FREE, FREE, FREE, 1, FREE, 0, FREE], 2, "GAGAACACA", ["(?.??.?)?", ""]),
    ([1] * 10, [8, N, 6, N, N, N, N, N, N, N], [0, FREE, 1, FREE, FREE, FREE, 1, FREE, 0, FREE], 2, "GAGAAACACA", ["(?.???.?)?", ".?(???)?.?"]),
    # no level-1 pair at all in a K = 2 call: the second string is empty, the first is row_constraint's
    ([1] * 8, [7, 6, N, N, N, N, N, N], [0, 0, FREE, FREE, FREE, FREE, 0, 0], 2, "GGAAAACC", ["((????))", ""]),
    # a level-0 string is always there, even when it forces nothing
    ([1] * 7, [4, N, 6, N, N, N, N], [0, FREE, 1, FREE, 0, FREE, 1], 2, "AAGAAAC", ["??.???.", ".?(?.?)"]),
    # three levels, the middle one skipped for this row (its left residue is missing)
    ([1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1], [5, N, N, 12, 14] + [N] * 11,
     _levels([[(0, 5)], [(3, 12)], [(4, 14)]], 16), 3, "GAAGCAAAAAAAACA", ["(??.)????????.?", "", ".??(.????????)?"]),
]


def test_row_constraint_levels_hand_made():
    from dafs_amd import capi
    for mask, ss, level, K, res, want in HAND_ROWS:
        assert ref.row_constraints(mask, ss, level, K, res) == want, res
        assert capi.row_constraint_levels(mask, ss, level, K, res) == want, res
    with pytest.raises(capi.DafsHipError):  # a level the call does not have
        capi.row_constraint_levels([1] * 7, [4, N, 6, N, N, N, N], [0, FREE, 1, FREE, 0, FREE, 1], 1, "GAGACAC")
    with pytest.raises(capi.DafsHipError):  # levels that differ at the two columns of a pair
        capi.row_constraint_levels([1] * 7, [4, N, 6, N, N, N, N], [0, FREE, 1, FREE, 1, FREE, 1], 2, "GAGACAC")
    with pytest.raises(capi.DafsHipError):  # one residue too few for the mask
        capi.row_constraint_levels([1] * 7, [4, N, 6, N, N, N, N], [0, FREE, 1, FREE, 0, FREE, 1], 2, "GAGACA")
    with pytest.raises(ValueError):
        capi.row_constraint_levels([1] * 7, [4, N, 6, N, N, N, N], [0, FREE, 1, FREE, 0, FREE, 1], 5, "GAGACAC")


def _random_knotted(rs, L):
    """a random structure with levels: per level a nested set of pairs over the columns still free"""
    ss, level = [N] * L, [FREE] * L
    K = int(rs.randint(1, 5))
    for k in range(K):
        free = [c for c in range(L) if level[c] == FREE]
        lo, hi = 0, len(free) - 1
        lo += int(rs.randint(0, 3))
        while hi - lo >= 1 and rs.rand() < 0.75:
            a, b = free[lo], free[hi]
            ss[a] = b
            level[a] = level[b] = k
            lo += int(rs.randint(1, 3)); hi -= int(rs.randint(1, 3))
    return ss, level, K


def test_row_constraint_levels_random_and_k1():
    from dafs_amd import capi
    rs = np.random.RandomState(2626)
    empties = 0
    for _ in range(200):
        L = int(rs.randint(1, 48))
        ss, level, K = _random_knotted(rs, L)
        mask = (rs.rand(L) < 0.8).astype(np.uint8)
        res = "".join(rs.choice(list("ACGUT")) for _ in range(int(mask.sum())))
        got = capi.row_constraint_levels(mask, ss, level, K, res)
        assert got == ref.row_constraints(mask.tolist(), ss, level, K, res)
        empties += sum(1 for s in got[1:] if s == "" and len(res))
        # K = 1: the structure's level-0 part alone is row_constraint's string, byte for byte
        ss0 = [p if p != N and level[c] == 0 else N for c, p in enumerate(ss)]
        lv0 = [0 if v == 0 else FREE for v in level]
        assert capi.row_constraint_levels(mask, ss0, lv0, 1, res) == [capi.row_constraint(mask, ss0, res)]
        assert capi.row_constraint(mask, ss0, res) == structure_ref.row_constraint(mask.tolist(), ss0, res)
    assert empties > 0


def test_knots_alone_is_refused_and_in_the_help(tmp_path):
    new = _write(tmp_path, "new.fa", ">n\nACGU\n>m\nACGU\n")
    r = _dafs(["--knots", new])
    assert r.returncode != 0 and r.stdout == "" and "--knots" in r.stderr and "--seed, --describe or --compare-ref" in r.stderr
    r = _dafs(["--help"])
    assert "--knots" in r.stdout + r.stderr
    assert "cannot yet be read back" not in r.stdout + r.stderr


def test_python_checks_seed_level():
    """seed_level without seed_ss, and levels that do not fit the structure, are refused before any device work"""
    from dafs_amd import pipeline
    rows = ["GAGACAC", "GAGACAC"]
    ss = [4, N, 6, N, N, N, N]
    for fn in (pipeline.add, pipeline.add_each):
        with pytest.raises(ValueError, match="needs it"):
            fn(["a", "b"], rows, ["n"], ["ACGU"], seed_level=[0, FREE, 1, FREE, 0, FREE, 1])
        for bad, msg in (([0, FREE, 1, FREE, 0, FREE], "6 entries"), ([0, FREE, 1, 0, 0, FREE, 1], "unpaired column 3"),
                         ([0, FREE, 1, FREE, 0, FREE, 2], "differs"), ([0, FREE, 0, FREE, 0, FREE, 0], "cross"),
                         ([4, FREE, 1, FREE, 4, FREE, 1], "levels are 0..3"), ([FREE, FREE, 1, FREE, FREE, FREE, 1], "levels are")):
            with pytest.raises(ValueError, match=msg):
                fn(["a", "b"], rows, ["n"], ["ACGU"], seed_ss=ss, seed_level=bad)


def test_carried_levels():
    from dafs_amd import pipeline
    ss = np.array([4, N, 6, N, N, N, N], np.uint32)
    level = np.array([0, FREE, 1, FREE, 0, FREE, 1], np.uint8)
    seed_col = np.array([0, 1, 4, 5, 6, 8, 9], np.uint32)
    got_ss, got_level = pipeline.carry_structure(ss, seed_col, 11, level)
    assert got_ss.tolist() == structure_ref.carry(ss.tolist(), seed_col.tolist(), 11)
    assert got_level.tolist() == ref.carry_levels(level.tolist(), seed_col.tolist(), 11)
    assert pipeline.carry_structure(ss, seed_col, 11).tolist() == got_ss.tolist()
    assert all(ref.nested(got_ss.tolist(), got_level.tolist(), k) for k in range(2))


def test_library_exports_and_declarations():
    import ctypes
    from dafs_amd import capi
    lib = ctypes.CDLL(capi.LIB_PATH)
    with open(os.path.join(ROOT, "include", "dafs_hip.h")) as fh:
        header = fh.read()
    for sym in ("dafs_host_seed_clean_structure_levels", "dafs_host_row_constraint_levels", "dafs_hip_fold_posteriors_levels_begin",
                "dafs_hip_fold_posteriors_levels"):
        assert hasattr(lib, sym) and ("int %s(" % sym) in header


def test_entry_points_under_sanitizers(tmp_path):
    """tests/host_knots_main.cpp calls the two new host entry points, the refusals and the empty inputs included, with output
    buffers of exactly the documented size, in a program of its own built with -fsanitize=address,undefined: exit status 0 and
    nothing on stderr"""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    flags = ["-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no usable address / undefined-behaviour sanitizer runtime: " + r.stderr.strip()[-200:])
    srcs = [os.path.join(ROOT, "tests", "host_knots_main.cpp"), os.path.join(ROOT, "dafs_amd", "csrc", "host_text.cpp"),
            os.path.join(ROOT, "dafs_amd", "csrc", "host_tree.cpp")]
    exe = str(tmp_path / "host_knots_main")
    r = subprocess.run([cxx] + flags + ["-Wall"] + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "" and r.stdout == "", (r.stdout, r.stderr)
