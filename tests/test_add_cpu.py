"""CPU tests of adding sequences to a fixed seed alignment: the merge dafs_host_merge_added
against a plain-Python restatement of its rule, the seed readers (stockholm.read_seed and the command line's), the
Stockholm block with an RF line, and the command-line combinations --seed refuses.  No device work."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = 0xFFFFFFFF


def merge_restated(C, zs):
    """The merge rule as DESIGN.md section 11 states it: (seed_col, [res_col per sequence], width)"""
    anchors = []
    for z in zs:
        a, an = -1, []
        for zi in z:
            if int(zi) != NONE:
                a = int(zi)
                an.append(None)
            else:
                an.append(a)
        anchors.append(an)
    W = {c: max([sum(1 for x in an if x == c) for an in anchors] + [0]) for c in range(-1, C)}
    cols = []
    for c in range(-1, C):
        if c >= 0:
            cols.append(("seed", c))
        cols += [("ins", c, t) for t in range(W[c])]
    at = {col: p for p, col in enumerate(cols)}
    res = []
    for z, an in zip(zs, anchors):
        used, r = {}, []
        for zi, a in zip(z, an):
            if int(zi) != NONE:
                r.append(at[("seed", int(zi))])
            else:
                t = used.get(a, 0)
                used[a] = t + 1
                r.append(at[("ins", a, t)])
        res.append(r)
    return [at[("seed", c)] for c in range(C)], res, len(cols)


def random_z(rs, n, C, frac):
    """a column map of n residues into C seed columns: a random share of residues matched, columns strictly increasing"""
    q = min(n, C, int(round(frac * n)))
    z = np.full(n, NONE, np.uint32)
    pos = np.sort(rs.choice(n, q, replace=False))
    z[pos] = np.sort(rs.choice(C, q, replace=False))
    return z


def _same(C, zs):
    from dafs_amd import capi
    seed_col, res_col, width = capi.merge_added(C, zs)
    w_seed, w_res, w_width = merge_restated(C, zs)
    assert width == w_width
    assert list(seed_col) == w_seed
    assert [list(r) for r in res_col] == w_res
    # every merged column holds a seed column or at least one new residue, and no two residues of a row share one
    used = set(int(c) for c in seed_col)
    for r in res_col:
        assert len(set(r.tolist())) == len(r)
        used |= set(r.tolist())
    assert used == set(range(width))


def test_merge_hand_made():
    Z = NONE
    # k = 1: inserts at anchor -1, inside, and after the last seed column (C - 1)
    _same(4, [np.array([Z, Z, 0, Z, 2, Z, Z], np.uint32)])
    _same(3, [np.array([Z, 0, 1, 2, Z, Z], np.uint32)])
    # k = 2: blocks as wide as the widest row, left-justified
    _same(3, [np.array([Z, 0, Z, Z, 2], np.uint32), np.array([Z, Z, 1, Z, 2, Z], np.uint32)])
    # empty maps: every residue inserted at anchor -1
    _same(5, [np.full(6, Z, np.uint32), np.full(2, Z, np.uint32)])
    # every residue matched
    _same(4, [np.arange(4, dtype=np.uint32), np.array([0, 2], np.uint32), np.array([3], np.uint32)])
    # a zero-length sequence changes nothing
    _same(2, [np.zeros(0, np.uint32), np.array([Z, 1], np.uint32)])


def test_merge_hand_made_layout():
    """the layout spelled out: seed columns s0..s2; row A = [ins, s0, ins, ins, s2], row B = [ins, ins, s1, ins]"""
    from dafs_amd import capi
    Z = NONE
    seed_col, res_col, width = capi.merge_added(3, [np.array([Z, 0, Z, Z, 2], np.uint32), np.array([Z, Z, 1, Z], np.uint32)])
    # anchor -1: 2 columns (B), s0 at 2, anchor 0: 2 columns (A), s1 at 5, anchor 1: 1 column (B), s2 at 7
    assert list(seed_col) == [2, 5, 7] and width == 8
    assert list(res_col[0]) == [0, 2, 3, 4, 7]
    assert list(res_col[1]) == [0, 1, 5, 6]


@pytest.mark.parametrize("k", [1, 2, 5])
def test_merge_random(k):
    rs = np.random.RandomState(100 + k)
    for trial in range(60):
        C = int(rs.randint(1, 30))
        frac = [0.0, 1.0, rs.uniform()][trial % 3]
        zs = [random_z(rs, int(rs.randint(0, 40)), C, frac) for _ in range(k)]
        _same(C, zs)


def test_merge_refuses_bad_maps():
    from dafs_amd import capi
    for C, zs in ((3, [np.array([1, 1], np.uint32)]), (3, [np.array([2, 0], np.uint32)]), (3, [np.array([3], np.uint32)]),
                  (2, [np.array([0, 1], np.uint32), np.array([NONE, 5], np.uint32)])):
        with pytest.raises(capi.DafsHipError):
            capi.merge_added(C, zs)


def test_merge_k1_is_project_alignment():
    """for one new sequence the merge is project_alignment((leaf), seed, z), column for column"""
    from dafs_amd import capi, pipeline
    rs = np.random.RandomState(7)
    for trial in range(80):
        m, C, n = int(rs.randint(1, 6)), int(rs.randint(1, 25)), int(rs.randint(1, 35))
        seed_mask = (rs.uniform(size=(m, C)) < 0.7).astype(np.uint8)
        seed_mask[rs.randint(m, size=C), np.arange(C)] = 1  # no all-gap column
        z = random_z(rs, n, C, [0.0, 1.0, rs.uniform()][trial % 3])
        sidx, want = pipeline.project_alignment((np.array([m], np.uint32), np.ones((1, n), np.uint8)),
                                                (np.arange(m, dtype=np.uint32), seed_mask), z)
        seed_col, res_col, width = capi.merge_added(C, [z])
        got = np.zeros((m + 1, width), np.uint8)
        got[0, res_col[0]] = 1
        got[1:, seed_col] = seed_mask
        assert list(sidx) == [m] + list(range(m))
        assert got.shape == want.shape and (got == want).all(), trial


# ---- seed readers ----
def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_bytes(text.encode("latin-1"))
    return str(p)


STO = """# STOCKHOLM 1.0
#=GF ID   test
#=GS a    DE first

a         AC-GU.
b         A--GUA
#=GR a PP 99.99.
#=GC SS_cons <<..>>

a         ..CC
b         -GC.
#=GC RF   xxxx
//
# STOCKHOLM 1.0
c         AAAA
//
"""


def test_read_stockholm_interleaved(tmp_path):
    from dafs_amd import stockholm
    names, rows = stockholm.read_seed(_write(tmp_path, "s.sto", STO))
    # a: AC-GU...CC, b: A--GUA-GC. -> columns 2 and 6 (gaps in both) dropped; the second alignment is not read
    assert names == ["a", "b"]
    assert rows == ["ACGU--CC", "A-GUAGC-"]


def test_read_aligned_fasta_as_printed(tmp_path):
    """the program's own stdout: a tree line, the SS_cons record, '> name' records; rows may span lines"""
    from dafs_amd import stockholm
    text = "[ 0.5 x y ]\n>SS_cons\n((..))--\n> x desc\nAC--\nGU-A\n>y\n-C-A\n\nGUA-\n"
    names, rows = stockholm.read_seed(_write(tmp_path, "s.aln", text))
    assert names == ["x desc", "y"]
    assert rows == ["AC-GU-A", "-CAGUA-"]  # column 2 is a gap in both rows


def test_read_gaps_normalised_and_columns_dropped(tmp_path):
    from dafs_amd import stockholm
    names, rows = stockholm.read_seed(_write(tmp_path, "s.fa", ">p\n..A-c.\n>q\n.-G.u-\n"))
    assert names == ["p", "q"] and rows == ["Ac", "Gu"]


@pytest.mark.parametrize("text,msg", [
    ("# STOCKHOLM 1.0\na ACGU\nb ACG\n//\n", "rows of unequal length"),
    (">a\nAC-U\n>b\nA*GU\n", "neither a letter nor a gap"),
    (">a\nAC-U\n>b\n-..-\n", "has no residues"),
    ("", "no rows"),
    ("# STOCKHOLM 1.0\n//\n", "no rows"),
    ("just text\n", "no rows"),
    ("# STOCKHOLM 1.0\na AC GU\n//\n", "neither a #= annotation nor 'name row'"),
])
def test_reader_refusals(tmp_path, text, msg):
    from dafs_amd import stockholm
    path = _write(tmp_path, "bad.txt", text)
    with pytest.raises(stockholm.SeedError, match=msg):
        stockholm.read_seed(path)
    # the command line reads the seed before it touches a device, with the same message
    if os.path.exists(DAFS):
        new = _write(tmp_path, "new.fa", ">n\nACGU\n")
        r = subprocess.run([DAFS, "--seed", path, new], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stderr and r.stdout == ""


def test_clean_seed_checks_direct_rows():
    from dafs_amd import stockholm
    assert stockholm.clean_seed(["a", "b"], ["A-.C", "-G.-"]) == (["a", "b"], ["A-C", "-G-"])
    with pytest.raises(stockholm.SeedError, match="has no residues"):  # so no seed is all gaps after the column removal
        stockholm.clean_seed(["a"], [""])
    with pytest.raises(stockholm.SeedError, match="no rows"):
        stockholm.clean_seed([], [])


# ---- Stockholm block ----
def test_block_without_new_arguments_is_unchanged():
    from dafs_amd import stockholm
    got = stockholm.block("[ 0.5 a b ]", ["a", "bb"], ["AC-", "A-G"], [[1.0, 0.5], [0.96, 0.04]], [0.98, 0.5, 0.2], "(.)")
    want = ("# STOCKHOLM 1.0\n"
            "#=GF CC [ 0.5 a b ]\n"
            "a            AC-\n"
            "#=GR a PP    *5.\n"
            "bb           A-G\n"
            "#=GR bb PP   *.0\n"
            "#=GC SS_cons (.)\n"
            "#=GC PP_cons *52\n"
            "//\n")
    assert got == want


def test_block_with_rf_and_without_cc():
    from dafs_amd import stockholm
    got = stockholm.block(None, ["a", "bb"], ["AC-", "A-G"], [[1.0, 0.5], [0.96, 0.04]], [0.98, 0.5, 0.2], "(.)",
                          rf=[True, False, True])
    want = ("# STOCKHOLM 1.0\n"
            "a            AC-\n"
            "#=GR a PP    *5.\n"
            "bb           A-G\n"
            "#=GR bb PP   *.0\n"
            "#=GC SS_cons (.)\n"
            "#=GC PP_cons *52\n"
            "#=GC RF      x.x\n"
            "//\n")
    assert got == want


# ---- command line ----
@pytest.mark.parametrize("opt,msg", [
    (["-r", "1"], "-r would realign"),
    (["--bp-update"], "--bp-update cannot"),
    (["--devices", "0,1"], "--devices cannot"),
    (["--align-aux", "X"], "--align-aux, --fold-aux"),
    (["--fold-aux", "X"], "--align-aux, --fold-aux"),
    (["--save-align-aux", "X"], "--align-aux, --fold-aux"),
    (["--save-fold-aux", "X"], "--align-aux, --fold-aux"),
    (["EXTRA.fa"], "exactly one FILE"),
])
def test_cli_refuses_combinations(tmp_path, opt, msg):
    if not os.path.exists(DAFS):
        pytest.skip("the dafs executable is built by build()")
    seed = _write(tmp_path, "s.sto", STO)
    new = _write(tmp_path, "new.fa", ">n\nACGU\n")
    r = subprocess.run([DAFS, "--seed", seed] + opt + [new], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert msg in r.stderr
    assert r.stdout == ""


def test_cli_help_names_seed():
    if not os.path.exists(DAFS):
        pytest.skip("the dafs executable is built by build()")
    r = subprocess.run([DAFS, "--help"], capture_output=True, text=True, timeout=60)
    assert "--seed SEED" in r.stdout
