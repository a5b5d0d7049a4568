"""CPU tests of the host side of the batched structure decode and the per-row structures: the
`#=GR <name> SS` lines of dafs_host_stockholm_block_rows against a plain-Python restatement of the layout, byte for byte; its
two refusals; the per-alignment memory estimate and the packing of a call's alignments into chunks; and the command line's
refusal of --row-structures without --stockholm.  No device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from dafs_amd import capi, pipeline, stockholm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = 0xFFFFFFFF


# ---- the layout, restated ----
def _pp(p):
    return "*" if p >= 0.95 else chr(ord("0") + int(math.floor(p * 10.0 + 0.5)))


def _brackets(ss):
    """one level of brackets: '(' at a left residue, ')' at its partner"""
    out = ["."] * len(ss)
    for i, j in enumerate(ss):
        if j != NONE:
            out[i], out[int(j)] = "(", ")"
    return "".join(out)


def _lay(row, own):
    """a row's own structure (over its residues) in the row's columns"""
    chars = iter(_brackets(own))
    return "".join("." if ch == "-" else next(chars) for ch in row)


def _block(tree, names, rows, rel, col, ss, rf, cov, row_ss):
    width = 12 if cov is None else 16
    width = max([width] + [len(nm) + 8 for nm in names]) + 1
    out = ["# STOCKHOLM 1.0"]
    if tree is not None:
        out.append("#=GF CC " + tree)
    for r, row in enumerate(rows):
        vals = iter(rel[r])
        out.append(names[r].ljust(width) + row)
        out.append(("#=GR %s PP" % names[r]).ljust(width) + "".join("." if ch == "-" else _pp(next(vals)) for ch in row))
        if row_ss is not None:
            out.append(("#=GR %s SS" % names[r]).ljust(width) + row_ss[r])
    cons = "".join(_pp(col[c]) if any(row[c] != "-" for row in rows) else "." for c in range(len(col)))
    out += ["#=GC SS_cons".ljust(width) + ss, "#=GC PP_cons".ljust(width) + cons]
    if cov is not None:
        out.append("#=GC cov_SS_cons".ljust(width) + cov)
    if rf is not None:
        out.append("#=GC RF".ljust(width) + "".join("x" if v else "." for v in rf))
    return "\n".join(out + ["//"]) + "\n"


def _nested(rs, n):
    """a random nested structure over n residues, pairs at least three apart"""
    ss = np.full(n, NONE, np.uint32)

    def fill(lo, hi):
        if hi - lo < 4:
            return
        i = rs.randint(lo, hi - 3)
        j = rs.randint(i + 3, hi)
        if rs.rand() < 0.8:
            ss[i] = j
        fill(lo, i)
        fill(i + 1, j)
        fill(j + 1, hi)
    fill(0, n)
    return ss


def _case(rs, rows, names):
    length = len(rows[0])
    rel = [np.array([rs.rand() for ch in row if ch != "-"]) for row in rows]
    col = rs.rand(length)
    owns = [_nested(rs, len(row) - row.count("-")) for row in rows]
    return rel, col, owns


HAND = [
    (["GGGAAACCC"], ["s"]),
    (["GG-GAAAC-CC", "-----------", "G--GAAAC--C"], ["a", "a_long_name_of_a_row.2", "b"]),
    (["---", "---"], ["x", "y"]),
    (["A"], ["only"]),
]


def test_gr_ss_lines_against_the_restated_layout():
    rs = np.random.RandomState(11)
    cases = list(HAND)
    for _ in range(200):
        n, length = rs.randint(1, 7), rs.randint(1, 41)
        rows = ["".join(rs.choice(list("ACGU")) if rs.rand() > 0.3 else "-" for _ in range(length)) for _ in range(n)]
        if rs.rand() < 0.2:
            rows[rs.randint(n)] = "-" * length  # an all-gap row
        cases.append((rows, ["".join(rs.choice(list("abcXYZ019_.|/-"), rs.choice([1, 2, 3, 5, 8, 9, 12, 20]))) for _ in range(n)]))
    seen = dict(rf=0, cov=0, neither=0, all_gap=0, paired=0)
    for k, (rows, names) in enumerate(cases):
        length = len(rows[0])
        rel, col, owns = _case(rs, rows, names)
        tree = "[ 0.5 a b ]" if k % 2 else None
        rf = [bool(v) for v in rs.rand(length) < 0.7] if k % 3 == 0 else None
        cov = "".join(rs.choice(list(".2"), length)) if k % 4 < 2 else None
        ss = "".join(rs.choice(list(".()"), length))
        row_ss = [_lay(row, own) for row, own in zip(rows, owns)]
        assert [stockholm.row_ss_str(row, own) for row, own in zip(rows, owns)] == row_ss, k
        assert stockholm.block(tree, names, rows, rel, col, ss, rf, cov, row_ss) == _block(tree, names, rows, rel, col, ss, rf, cov, row_ss), k
        seen["rf"] += rf is not None
        seen["cov"] += cov is not None
        seen["neither"] += rf is None and cov is None
        seen["all_gap"] += any(row == "-" * length for row in rows)
        seen["paired"] += any("(" in x for x in row_ss)
    assert all(seen.values()), seen


def _raw_block(fn, tree, names, rows, rel, col, ss, rf, cov, *more):
    rel = [np.ascontiguousarray(r, np.float64) for r in rel]
    col = np.ascontiguousarray(col, np.float64)
    rf8 = None if rf is None else np.ascontiguousarray(rf, np.uint8)
    enc = [None if t is None else t.encode("latin-1") for t in (tree, ss, cov)]
    return capi.host_text(fn, enc[0], len(rows), len(col), capi.c_strings(names), capi.c_strings(rows),
                          (C.c_void_p * max(len(rel), 1))(*[r.ctypes.data for r in rel]), col.ctypes.data, enc[1],
                          None if rf8 is None else rf8.ctypes.data, enc[2], *more)


def test_without_structures_the_block_is_the_old_one():
    rs = np.random.RandomState(12)
    for k, (rows, names) in enumerate(HAND):
        length = len(rows[0])
        rel, col, _ = _case(rs, rows, names)
        rf = [True] * length if k % 2 else None
        cov = "." * length if k < 2 else None
        args = ("[ 1 x ]", names, rows, rel, col, "." * length, rf, cov)
        old = _raw_block(capi._stockholm_block, *args)
        assert _raw_block(capi._stockholm_block_rows, *args, None) == old
        assert stockholm.block(*args) == old == _block(*args, None)


def test_refusals_of_row_structures():
    rows, names = ["GG-GAAAC-CC", "G--GAAAC--C"], ["a", "b"]
    rel = [[0.5] * 9, [0.5] * 8]
    col = [0.5] * 11
    good = ["((.(...).))", "(..(...)..)"]
    assert "#=GR a SS" in stockholm.block(None, names, rows, rel, col, "." * 11, None, None, good)
    with pytest.raises(ValueError, match="columns, not 11"):  # a string of another length than the row
        stockholm.block(None, names, rows, rel, col, "." * 11, None, None, [good[0], good[1][:-1]])
    with pytest.raises(ValueError, match="gap column 3"):  # a bracket on a gap column
        stockholm.block(None, names, rows, rel, col, "." * 11, None, None, ["(((....).))", good[1]])
    with pytest.raises(ValueError):
        stockholm.block(None, names, rows, rel, col, "." * 11, None, None, good[:1])
    assert "#=GR b SS" in stockholm.block(None, names, rows, rel, col, "." * 11, None, None, good)  # usable afterwards


# ---- memory estimate and chunks ----
def test_structure_bytes_is_monotone_and_covers_the_tables():
    sb = lambda n, length: int(capi._structure_bytes(n, length))  # noqa: E731
    for n in (1, 2, 5, 100):
        for length in (1, 3, 64, 257, 1100, 30000):
            assert sb(n, length) < sb(n + 1, length) and sb(n, length) < sb(n, length + 1)
            # the averaged matrix and the four tables of the decoder (20 bytes a cell), ranks and residue columns of the rows
            assert sb(n, length) >= 20 * length * length + 8 * n * length
    assert sb(0, 0) > 0
    assert int(capi._structures_batch_bytes()) > sb(2, 3000)  # a 3 000-column alignment fits a default chunk


def test_chunks_keep_order_never_split_and_run_an_oversized_alignment_alone():
    rs = np.random.RandomState(13)
    for trial in range(50):
        shapes = [(int(rs.randint(1, 6)), int(rs.choice([1, 5, 64, 150, 257, 1100]))) for _ in range(rs.randint(1, 40))]
        sizes = [int(capi._structure_bytes(n, length)) for n, length in shapes]
        budget = int(rs.choice([1, sizes[0], 3 * max(sizes) // 2, 4 * max(sizes), sum(sizes)]))
        groups = pipeline.pack_families(sizes, budget)
        assert [k for grp in groups for k in grp] == list(range(len(shapes)))  # input order, every alignment once, whole
        for g, grp in enumerate(groups):
            total = sum(sizes[k] for k in grp)
            assert total <= budget or len(grp) == 1  # over the budget: alone
            if g + 1 < len(groups):  # greedy: the next alignment would not have fitted
                assert total + sizes[groups[g + 1][0]] > budget
    assert pipeline.pack_families([10, 100, 10], 50) == [[0], [1], [2]]


# ---- the command line ----
def test_row_structures_needs_stockholm():
    if not os.path.exists(DAFS):
        pytest.fail("dafs_amd/dafs is not built (python __graft_entry__.py)")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # no device could be opened: parsing refuses first
    r = subprocess.run([DAFS, "--row-structures", os.path.join(ROOT, "no_such_input.fa")], capture_output=True, text=True, env=env)
    assert r.returncode != 0 and r.stdout == "" and r.stderr.strip() == "--row-structures needs --stockholm"
    r = subprocess.run([DAFS, "--help"], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "--row-structures" in r.stdout
