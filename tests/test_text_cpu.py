"""CPU tests of the host text functions of libdafs_hip.so (dafs_amd/csrc/host_text.cpp: the Stockholm block, the --covariation
and --pairwise-scores tables, the seed reader, the memory estimates and the greedy packing), reached through
dafs_amd/stockholm.py and dafs_amd/pipeline.py as the Python driver reaches them: against the plain-Python restatement in
tests/text_ref.py, byte for byte, on generated cases with fixed seeds; and the stand-alone program tests/host_text_main.cpp
under the address and undefined-behaviour sanitizers.  No device."""
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

import text_ref
from dafs_amd import pipeline, stockholm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = text_ref.NONE
RESIDUES = "ACGUacguTtNn"
NEG_NAN = np.copysign(np.nan, -1.0)


def _name(rs, length):
    return "".join(rs.choice(list("abcXYZ019_.|/-"), length))


def _rows(rs, n, length, gap=0.3):
    """n rows of `length` columns; a few columns are gaps in every row"""
    rows = [[rs.choice(list(RESIDUES)) if rs.rand() > gap else "-" for _ in range(length)] for _ in range(n)]
    for c in range(length):
        if rs.rand() < 0.15:
            for row in rows:
                row[c] = "-"
    return ["".join(row) for row in rows]


def _structure(rs, length, pairs=None):
    """disjoint column pairs, left column -> right column"""
    ss = np.full(length, NONE, np.uint32)
    cols = list(rs.permutation(length))
    for _ in range(rs.randint(0, length // 2 + 1) if pairs is None else pairs):
        if len(cols) < 2:
            break
        a, b = sorted((int(cols.pop()), int(cols.pop())))
        ss[a] = b
    return ss


# ---- PP characters and names ----
def test_pp_char():
    rs = np.random.RandomState(1)
    ps = [k / 100.0 for k in range(5, 100, 10)] + [0.05, 0.15, 0.25, 0.35, 0.45, 0.55, 0.65, 0.75, 0.85, 0.95, 0.949999, 0.0, 1.0]
    ps += list(rs.rand(300)) + [np.float32(p) for p in rs.rand(50)] + [np.nextafter(0.95, 0), np.nextafter(0.05, 0), np.nextafter(0.05, 1)]
    assert [stockholm.pp_char(p) for p in ps] == [text_ref.pp_char(p) for p in ps]


def test_names():
    rs = np.random.RandomState(2)
    words = ["a", "a", "b", "seq2", "seq3", "x.2", "x", "tRNA-Ala", "\xe9t\xe9"]
    blanks = ["", " ", "\t", "  ", " \t ", "\v", "\f\r"]
    for _ in range(300):
        headers = []
        for _ in range(rs.randint(0, 9)):
            kind = rs.randint(4)
            if kind == 0:
                headers.append(rs.choice(blanks))
            else:
                headers.append(rs.choice(blanks) + rs.choice(words) + (rs.choice(blanks[1:]) + "desc " + rs.choice(words) if kind == 2 else ""))
        assert stockholm.names(headers) == text_ref.names(headers), headers


# ---- Stockholm blocks ----
def test_blocks():
    rs = np.random.RandomState(3)
    pool = [0.05, 0.15, 0.25, 0.35, 0.45, 0.55, 0.65, 0.75, 0.85, 0.95, 0.949999, 0.0, 1.0]
    decided = dict(base=0, cov=0, name=0)  # which of the three width rules set the label width, alone
    seen = dict(one_row=0, all_gap_column=0, tree=0, rf=0, cov=0, plain=0)
    for case in range(300):
        n = 1 if case % 7 == 0 else rs.randint(1, 7)
        length = rs.randint(1, 31)
        rows = _rows(rs, n, length)
        names = [_name(rs, rs.choice([1, 2, 3, 5, 7, 8, 9, 12, 20])) for _ in range(n)]
        rel = [[rs.choice(pool) if rs.rand() < 0.6 else rs.rand() for ch in row if ch != "-"] for row in rows]
        col = np.array([rs.choice(pool) if rs.rand() < 0.6 else rs.rand() for _ in range(length)])
        tree = "[ 0.5 %s ]" % " ".join(names) if rs.rand() < 0.5 else None
        rf = [bool(v) for v in rs.rand(length) < 0.7] if rs.rand() < 0.5 else None
        cov = "".join(rs.choice(list(".2"), length)) if rs.rand() < 0.5 else None
        ss = "".join(rs.choice(list(".()"), length))
        if case % 3 == 0:  # the reliabilities as the driver holds them
            rel = [np.array(r, np.float64) for r in rel]
        got = stockholm.block(tree, names, rows, rel, col, ss, rf, cov)
        assert got == text_ref.block(tree, names, rows, rel, col, ss, rf, cov), case
        w_name, w_fixed = max(len(nm) for nm in names) + 8, 12 if cov is None else 16  # "#=GR <name> PP" against the #=GC labels
        if w_name != w_fixed:
            decided["name" if w_name > w_fixed else "base" if cov is None else "cov"] += 1
        seen["one_row"] += n == 1
        seen["all_gap_column"] += any(all(row[c] == "-" for row in rows) for c in range(length))
        seen["tree"] += tree is not None
        seen["rf"] += rf is not None
        seen["cov"] += cov is not None
        seen["plain"] += tree is None and rf is None and cov is None
    assert all(decided.values()) and all(seen.values()), (decided, seen)
    assert stockholm.block(None, [], [], [], [], "") == text_ref.block(None, [], [], [], [], "")
    for bad in (dict(rows=["AC"]), dict(rel=[[0.5]]), dict(rf=[True])):  # a row, the reliabilities, rf of the wrong length
        kw = dict(rows=["A-C"], rel=[[0.5, 0.5]], rf=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            stockholm.block(None, ["a"], kw["rows"], kw["rel"], [0.1, 0.2, 0.3], "...", kw["rf"])


# ---- covariation: the cov_SS_cons characters and the table ----
def _cov_case(rs, empty_ss=False):
    n, length = rs.randint(1, 9), rs.randint(1, 25)
    rows = _rows(rs, n, length, gap=0.15)
    ss = _structure(rs, length, 0 if empty_ss else None)

    def values(scale):
        v = rs.rand(length) * scale
        v[rs.rand(length) < 0.15] = np.nan
        v[rs.rand(length) < 0.1] = NEG_NAN
        v[rs.rand(length) < 0.1] = 0.05
        v[rs.rand(length) < 0.05] = np.inf
        return v
    best = np.array([rs.choice([d for d in range(length) if d != c] or [NONE]) for c in range(length)], np.uint32)
    best[rs.rand(length) < 0.2] = NONE
    for c in range(length):  # some pairs named from both of their columns, some that are consensus pairs too
        if best[c] != NONE and rs.rand() < 0.3:
            best[best[c]] = c
        if ss[c] != NONE and rs.rand() < 0.4:
            best[c] = ss[c]
        if ss[c] != NONE and rs.rand() < 0.4:
            best[ss[c]] = c
    res = types.SimpleNamespace(rows=rows, ss=ss)
    res.covariation = dict(best=best, best_score=values(20.0) - 5.0, best_e=values(0.12), pair_score=values(20.0) - 5.0, pair_e=values(0.12),
                           pair_rows=rs.randint(0, n + 1, length).astype(np.uint32), pair_canonical=rs.randint(0, n + 1, length).astype(np.uint32),
                           pair_types=rs.randint(0, 7, length).astype(np.uint32), e_max=rs.choice([0.05, 0.01, 1.0]))
    return res


def test_covariation_tables_and_cov_lines():
    rs = np.random.RandomState(4)
    seen = dict(both_columns=0, other_is_consensus=0, negative_nan=0, no_partner=0, other=0, lower_or_t=0, empty=0)
    for case in range(300):
        res = _cov_case(rs, empty_ss=case % 10 == 0)
        cv, ss = res.covariation, res.ss
        got = pipeline.covariation_tsv(res)
        assert got == text_ref.covariation_tsv(res), case
        for e_max in (cv["e_max"], 0.05):
            assert stockholm.cov_ss_cons(ss, cv["pair_e"], e_max) == text_ref.cov_ss_cons(ss, cv["pair_e"], e_max), case
        listed = [c for c in range(len(ss)) if cv["best"][c] != NONE and cv["best_e"][c] <= 0.05]
        seen["both_columns"] += any(cv["best"][cv["best"][c]] == c and cv["best"][c] in listed for c in listed)
        seen["other_is_consensus"] += any(ss[min(c, cv["best"][c])] == max(c, cv["best"][c]) for c in listed)
        seen["negative_nan"] += bool(np.signbit(cv["pair_e"][np.isnan(cv["pair_e"])]).any()) and "nan" in got and "-nan" not in got
        seen["no_partner"] += bool((cv["best"] == NONE).any())
        seen["other"] += "\tother\t" in got
        seen["lower_or_t"] += any(ch in "acgutT" for row in res.rows for ch in row)
        seen["empty"] += got == ""
    assert all(seen.values()), seen
    assert stockholm.cov_ss_cons(np.zeros(0, np.uint32), np.zeros(0)) == ""


# ---- the --pairwise-scores table ----
def test_pairwise_tables():
    rs = np.random.RandomState(5)
    for case in range(200):
        n = rs.randint(2, 8)
        names = [_name(rs, rs.randint(1, 9)) + (" desc" if rs.rand() < 0.3 else "") for _ in range(n)]
        sim = rs.rand(n, n).astype(np.float32)
        score = ((rs.rand(n, n) - 0.5) * 10 ** rs.randint(-8, 9)).astype(np.float32)
        for a in (sim, score):
            a[rs.rand(n, n) < 0.1] = np.nan
            a[rs.rand(n, n) < 0.1] = NEG_NAN
            a[rs.rand(n, n) < 0.05] = -np.inf
            a[rs.rand(n, n) < 0.05] = 0.0
        its = rs.randint(-1, 601, (n, n)).astype(np.int64)
        pairs = [pr for pr in pipeline.all_pairs(n) if rs.rand() < 0.7] if case % 9 else []
        if case % 2:
            sim, score = sim.astype(np.float64) + rs.rand(n, n) * 1e-9, score.astype(np.float64)
        got = pipeline.pairwise_scores_tsv(names, pairs, sim, score, its)
        assert got == text_ref.pairwise_scores_tsv(names, pairs, sim, score, its), case
        assert got.count("\n") == len(pairs) and "-nan" not in got


# ---- the seed reader ----
def _both(lib, ref, *args):
    """what the library's function and the restatement make of args: the value, or the refusal's text"""
    out = []
    for fn, err in ((lib, stockholm.SeedError), (ref, text_ref.SeedError)):
        try:
            out.append(fn(*args))
        except err as e:
            out.append("refused: %s" % e)
    return out


def _same_seed(text):
    got, want = _both(stockholm.parse_seed, text_ref.parse_seed, text)
    assert got == want, text
    if not isinstance(want, str):
        got, want = _both(stockholm.clean_seed, text_ref.clean_seed, *want)
        assert got == want, text
    return want


HAND_SEEDS = [
    # interleaved Stockholm with annotations; a second alignment after the first "//"
    "# STOCKHOLM 1.0\n#=GF ID t\n\na  AC-GU.\nb  A--GUA\n#=GR a PP 99.99.\n#=GC SS_cons <<..>>\n\na  ..CC\nb  -GC.\n//\n# STOCKHOLM 1.0\nc AAAA\n//\n",
    "# STOCKHOLM 1.0\r\na AC-GU\r\nb A.CGU\r\n//\r\n",                     # CRLF line ends
    "# STOCKHOLM 1.0  \t\na\tACGU\n\n \nb  AC.U  \n",                        # no "//" at all, blanks after fields
    "[ 0.5 x y ]\n>SS_cons\n((..))--\n> x desc\nAC--\nGU-A\n>y\n-C-A\n\nGUA-\n",  # dafs' own stdout: a tree line, SS_cons, rows over lines
    ">   \nAC-U\n>\t\nACGU\n",                                              # headers of blanks only
    ">a\nAC GU\n  A\n>b\r\nACGUA\r\n",                                       # blanks inside a row, CRLF
    "stray\n# STOCKHOLM 1.0\na ACGU\n//\n",                                 # not Stockholm: the marker is not the first line
    ">a\nACGU\n>b\nACGU",                                                    # no newline at the end
    ">a\n\xc4CGU\n>b\nACGU\n", ">n\xe4me\nACGU\n",                           # bytes above 127: no letters; fine in a name
    ">SS_cons\n....\n", "\n\n", ">a\n>b\n", "# STOCKHOLM 1.0\na ACGU extra\n//\n", "# STOCKHOLM 1.0\nlonely\n",
]


def test_seed_reader_by_hand():
    for text in HAND_SEEDS:
        _same_seed(text)
    assert _same_seed(HAND_SEEDS[0]) == (["a", "b"], ["ACGU--CC", "A-GUAGC-"])
    assert _same_seed(HAND_SEEDS[3]) == (["x desc", "y"], ["AC-GU-A", "-CAGUA-"])
    assert _same_seed(HAND_SEEDS[4]) == (["", ""], ["AC-U", "ACGU"])
    with pytest.raises(stockholm.SeedError, match="NUL"):  # names and rows travel as C strings
        stockholm.parse_seed(">a\nA\0C\n")


def _seed_text(rs):
    """a random seed file in one of the two formats, now and then damaged"""
    n, length = rs.randint(1, 6), rs.randint(1, 40)
    rows = ["".join(rs.choice(list("ACGUacgun.-"), length)) for _ in range(n)]
    names = [_name(rs, rs.randint(1, 7)) for _ in range(n)]
    if rs.rand() < 0.2:
        names[rs.randint(n)] = names[0]        # a repeated name: Stockholm joins its rows
    damage = rs.randint(12)
    if damage == 0:
        rows[rs.randint(n)] += "A"
    elif damage == 1:
        k = rs.randint(n)
        rows[k] = rows[k][:length // 2] + rs.choice(list("*1?~")) + rows[k][length // 2 + 1:]
    elif damage == 2:
        rows[rs.randint(n)] = "".join(rs.choice(list(".-"), length))
    eol = "\r\n" if rs.rand() < 0.3 else "\n"
    lines = []
    if rs.rand() < 0.5:
        lines.append("# STOCKHOLM 1.0")
        step = rs.randint(1, length + 1)
        for b in range(0, length, step):
            lines += [rs.choice(["", "#=GF ID x", " "])]
            for nm, row in zip(names, rows):
                lines.append(nm + rs.choice([" ", "\t", "   "]) + row[b:b + step] + rs.choice(["", " ", "\t"]))
            lines.append("#=GC SS_cons " + "." * len(rows[0][b:b + step]))
            if damage == 3 and b == 0:
                lines.append("three fields here")
        if rs.rand() < 0.8:
            lines += ["//"] + (["# STOCKHOLM 1.0", "other ACGU", "//"] if rs.rand() < 0.5 else [])
    else:
        if rs.rand() < 0.5:
            lines.append("[ 0.5 a b ]")
        if rs.rand() < 0.5:
            lines += [">SS_cons", "." * length]
        step = rs.randint(1, length + 1)
        for nm, row in zip(names, rows):
            lines.append(">" + rs.choice(["", " ", "  \t"]) + (nm if damage != 4 else "") + rs.choice(["", " desc"]))
            lines += [row[b:b + step] for b in range(0, length, step)]
            if rs.rand() < 0.2:
                lines.append("")
    return eol.join(lines) + (eol if rs.rand() < 0.9 else "")


def test_seed_reader_generated():
    rs = np.random.RandomState(6)
    kinds = dict(read=0, refused=0)
    for _ in range(400):
        want = _same_seed(_seed_text(rs))
        kinds["refused" if isinstance(want, str) else "read"] += 1
    assert kinds["read"] > 50 and kinds["refused"] > 50, kinds


# the refusals of test_add_cpu.py::test_reader_refusals, with the whole message
REFUSALS = [
    ("# STOCKHOLM 1.0\na ACGU\nb ACG\n//\n", "seed: rows of unequal length (a: 4 columns, b: 3)"),
    (">a\nAC-U\n>b\nA*GU\n", "seed: row b holds '*', which is neither a letter nor a gap"),
    (">a\nAC-U\n>b\n-..-\n", "seed: row b has no residues"),
    ("", "seed: no rows"),
    ("# STOCKHOLM 1.0\n//\n", "seed: no rows"),
    ("just text\n", "seed: no rows"),
    ("# STOCKHOLM 1.0\na AC GU\n//\n", "seed: line 2 is neither a #= annotation nor 'name row'"),
]


@pytest.mark.parametrize("text,message", REFUSALS)
def test_seed_refusals(tmp_path, text, message):
    assert _same_seed(text) == "refused: " + message
    path = tmp_path / "seed.txt"
    path.write_bytes(text.encode("latin-1"))
    with pytest.raises(stockholm.SeedError) as e:
        stockholm.read_seed(str(path))
    assert str(e.value) == message


# ---- estimates and packing ----
def test_estimates():
    grid = (1, 2, 63, 64, 2047, 2048, 5000)
    for l1 in grid:
        for l2 in grid:
            assert pipeline.node_bytes(l1, l2) == text_ref.node_bytes(l1, l2), (l1, l2)
            assert pipeline.family_bytes([l1, l2]) == text_ref.family_bytes([l1, l2]), (l1, l2)
            assert pipeline.pair_bytes(l1, l2) == text_ref.pair_bytes(l1, l2), (l1, l2)
    rs = np.random.RandomState(7)
    for _ in range(200):
        lens = [int(v) for v in rs.randint(1, 6000, rs.randint(0, 12))]
        assert pipeline.family_bytes(lens) == text_ref.family_bytes(lens), lens
    assert pipeline.DEFAULT_BATCH_BYTES == text_ref.DEFAULT_BATCH_BYTES == 16 << 30


def test_packing():
    rs = np.random.RandomState(8)
    for case in range(300):
        sizes = [int(v) for v in rs.randint(1, 10 ** rs.randint(1, 12), rs.randint(0, 30))]
        for budget in (1, 1 << 62, int(rs.randint(1, 10 ** rs.randint(1, 13))), max(sizes + [1]), sum(sizes) // 3 + 1):
            assert pipeline.pack_families(sizes, budget) == text_ref.pack_families(sizes, budget), (sizes, budget)
    for _ in range(50):
        lens = [int(v) for v in rs.randint(1, 3000, rs.randint(2, 9))]
        pairs = pipeline.all_pairs(len(lens))
        for budget in (1, 1 << 62, int(rs.randint(1 << 20, 1 << 34))):
            assert pipeline.pair_chunks(lens, pairs, budget) == text_ref.pair_chunks(lens, pairs, budget)


# ---- memory safety of the C entry points ----
def test_entry_points_under_sanitizers(tmp_path):
    """tests/host_text_main.cpp calls every host text entry point, the refusals and the empty inputs included, in a program of
    its own built with -fsanitize=address,undefined: exit status 0 and nothing on stderr"""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    flags = ["-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no usable address / undefined-behaviour sanitizer runtime: " + r.stderr.strip()[-200:])
    srcs = [os.path.join(ROOT, "tests", "host_text_main.cpp"), os.path.join(ROOT, "dafs_amd", "csrc", "host_text.cpp"),
            os.path.join(ROOT, "dafs_amd", "csrc", "host_tree.cpp")]
    exe = str(tmp_path / "host_text_main")
    r = subprocess.run([cxx] + flags + ["-Wall"] + srcs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.stdout, r.stderr)
