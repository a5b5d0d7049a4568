"""CPU tests of the merged alignment of all placements (pipeline.add_each(merged=True), `dafs --seed-merged`; DESIGN.md section
17) against the restatement of merged_ref.py: the merge over independent maps, the rows, RF, the carried structure, the PP
lines and PP_cons, the block's bytes, the refusals of both drivers, the help text and the new symbols -- no HIP call."""
import ctypes
import os
import re
import subprocess
import time

import numpy as np
import pytest

import merged_ref
import text_ref
from dafs_amd import capi, pipeline, stockholm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
G = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "dafs_hip.h")
Z = merged_ref.NONE

SEED_NAMES = ["s0 first", "s1", "s0"]
SEED_ROWS = ["GGCAAAGCC", "GGC-AAGCC", "GCCAA-GGC"]
SEED_SS = [8, 7, 6, Z, Z, Z, Z, Z, Z]
C = 9


def _case(k):
    """k hand-made maps over the 9 seed columns: residues before the first seed column (anchor -1), a tail past the last
    (anchor C - 1), an empty map (nothing matched) and a full one (every residue matched)"""
    maps = [[Z, Z, 0, 1, 2, Z, 5, 6, 8, Z, Z, Z],   # two residues before column 0, an insert behind column 2, a tail of three
            [0, 1, 2, 3, 4, 5, 6, 7, 8],            # full
            [Z, Z, Z, Z],                           # empty: all of it lands in the block of anchor -1
            [Z, 0, Z, Z, 2, 8, Z],                  # a wider insert behind column 0 than anyone else's
            [3, 4, Z, 5]][:k]
    rs = np.random.RandomState(k)
    seqs = ["".join(rs.choice(list("ACGU"), len(z))) for z in maps]
    pps = [rs.rand(len(z)) for z in maps]
    pps[0][:3] = [0.95, 0.949999, 0.05]  # the edges of the PP characters
    names = ["n%d hit" % j for j in range(k)]
    if k > 1:
        names[1] = "s1"  # a name the seed has already
    return names, seqs, [np.array(z, np.uint32) for z in maps], pps


@pytest.mark.parametrize("k", [1, 2, 5])
def test_merged_against_the_restatement(k):
    names, seqs, zs, pps = _case(k)
    got = pipeline._merge_each(SEED_NAMES, SEED_ROWS, np.array(SEED_SS, np.uint32), names, seqs, zs, pps)
    want = merged_ref.merged(SEED_NAMES, SEED_ROWS, SEED_SS, names, seqs, [z.tolist() for z in zs], pps)
    assert got.names == want.names and got.rows == want.rows
    assert got.rf.tolist() == want.rf and got.ss.tolist() == want.ss and got.ss_str == want.ss_str
    assert np.array(got.col).tobytes() == np.array(want.col).tobytes()
    assert got.stockholm == want.stockholm
    assert got.output == want.output
    assert [z.tobytes() for z in got.z] == [z.tobytes() for z in zs] and [p.tobytes() for p in got.pp] == [p.tobytes() for p in pps]
    # the seed is untouched: without the insert columns and the new rows it is the seed, structure included
    assert ["".join(ch for ch, x in zip(r, got.rf) if x) for r in got.rows[:3]] == SEED_ROWS
    assert "".join(ch for ch, x in zip(got.ss_str, got.rf) if x) == "(((...)))" and all(ch == "." for ch, x in zip(got.ss_str, got.rf) if not x)
    assert [r.replace("-", "") for r in got.rows[3:]] == seqs
    lines = got.stockholm.split("\n")
    assert lines[0] == "# STOCKHOLM 1.0" and lines[-2] == "//" and not any(ln.startswith("#=GF") for ln in lines)
    assert [ln.split()[1] for ln in lines if ln.startswith("#=GR")] == got.names[3:]  # PP lines for the new rows alone
    assert [ln.split()[0] for ln in lines[1 + 3 + k + k:-2]] == ["#=GC"] * 3
    cons = lines[-4].split()[-1]
    new_cols = {c for r in got.rows[3:] for c, ch in enumerate(r) if ch != "-"}
    assert all((ch == ".") == (c not in new_cols) for c, ch in enumerate(cons))
    # anchors: the block before the first seed column (two columns, four once the empty map is there), the tail behind the last
    lead = 2 if k < 3 else 4
    assert not got.rf[:lead].any() and got.rf[lead] and got.rows[3][:lead] == seqs[0][:2] + "-" * (lead - 2)
    assert not got.rf[-3:].any() and got.rf[-4] and got.rows[3].endswith(seqs[0][-3:])
    if k == 5:
        assert got.rows[5] == seqs[2] + "-" * (len(got.rf) - 4)  # the empty map, left-justified in the first block
        assert lines[1 + 3 + 5].split()[-1].replace(".", "").startswith("*91")  # 0.95, 0.949999, 0.05
    # the block can be read back as a seed with its structure
    rn, rr_, st = stockholm.parse_seed_structure(got.stockholm)
    assert rn == got.names and rr_ == got.rows and st == got.ss_str


def test_merge_of_thousands_of_maps():
    """k in the thousands: dafs_host_merge_added makes two passes over the maps and one over the columns, so 16 times the maps
    take about 16 times as long and a quadratic merge 256 times; the bound of 100 leaves a loaded machine a factor of six"""
    rs = np.random.RandomState(3)

    def maps(k):
        out = []
        for _ in range(k):
            z = np.full(100, Z, np.uint32)
            z[np.sort(rs.permutation(100)[:80])] = np.sort(rs.permutation(300)[:80]).astype(np.uint32)
            out.append(z)
        return out

    def seconds(zs):
        lens = np.array([len(z) for z in zs], np.uint32)
        z = np.ascontiguousarray(np.concatenate(zs), np.uint32)
        seed_col, res_col, width = np.zeros(300, np.uint32), np.zeros(len(z), np.uint32), ctypes.c_uint32()
        best = 1e9
        for _ in range(5):  # the library call alone, without the binding's array handling
            t = time.perf_counter()
            capi.check(capi._merge_added(300, len(zs), lens.ctypes.data, z.ctypes.data, seed_col.ctypes.data, res_col.ctypes.data, ctypes.byref(width)))
            best = min(best, time.perf_counter() - t)
        return best
    small, large = maps(2000), maps(32000)
    want = merged_ref.merge(300, [z.tolist() for z in large[:50]])
    got = capi.merge_added(300, large[:50])
    assert got[2] == want[2] and got[0].tolist() == want[0] and [r.tolist() for r in got[1]] == want[1]
    assert capi.merge_added(300, large)[2] >= want[2]
    assert seconds(large) < 100 * max(seconds(small), 2e-4)


def test_the_old_writer_is_unchanged():
    rows = ["AC-GU", "A-CGU"]
    rel = [np.array([0.9, 0.5, 0.96, 0.1]), np.array([0.3, 0.2, 0.949, 1.0])]
    col = np.array([0.6, 0.5, 0.2, 0.95, 0.55])
    for rf in (None, [True, False, True, True, True]):
        assert stockholm.block("(a,b)", ["a", "b"], rows, rel, col, "(...)", rf) == text_ref.block("(a,b)", ["a", "b"], rows, rel, col, "(...)", rf)
        assert stockholm.block(None, ["a", "b"], rows, rel, col, "(...)", rf) == text_ref.block(None, ["a", "b"], rows, rel, col, "(...)", rf)


def test_block_merged_refusals():
    with pytest.raises(ValueError):
        stockholm.block_merged(["a"], ["ACG", "ACG"], [None, None], "...", [1, 1, 1])
    with pytest.raises(ValueError, match="columns"):
        stockholm.block_merged(["a", "b"], ["ACG", "AC"], [None, None], "...", [1, 1, 1])
    with pytest.raises(ValueError, match="columns"):
        stockholm.block_merged(["a", "b"], ["ACG", "ACG"], [None, None], "..", [1, 1, 1])
    with pytest.raises(ValueError):
        stockholm.block_merged(["a", "b"], ["ACG", "ACG"], [None, np.array([0.5])], "...", [1, 1, 1])
    text, col = stockholm.block_merged(["a", "b"], ["ACG", "A-G"], [None, None], "...", [1, 1, 1])  # no placed row at all
    assert text.split("\n")[4].split()[-1] == "..." and np.isnan(col).all()


class _NoContext:
    def __init__(self, *a, **k):
        raise AssertionError("a context was opened")


def _cli(*args):
    return subprocess.run([DAFS] + list(args), capture_output=True, text=True, timeout=60)


def test_refusals_have_the_same_text_in_both_drivers(tmp_path, monkeypatch):
    monkeypatch.setattr(capi, "Context", _NoContext)
    with pytest.raises(ValueError) as e:
        pipeline.add_each(SEED_NAMES, SEED_ROWS, ["x"], ["ACGU"], merged=True)
    message = str(e.value)
    assert "seed's structure" in message
    seed = tmp_path / "seed.sto"
    seed.write_text("# STOCKHOLM 1.0\n" + "".join("%s %s\n" % (n.split()[0] + str(i), r) for i, (n, r) in enumerate(zip(SEED_NAMES, SEED_ROWS))) +
                    "#=GC SS_cons (((...)))\n//\n")
    fa, out = os.path.join(G, "RF00005_0.fa"), tmp_path / "merged.sto"
    r = _cli("--seed", str(seed), "--seed-each", "--seed-merged", str(out), fa)
    assert r.returncode != 0 and r.stderr.strip() == message and r.stdout == "" and not out.exists()
    # refused while parsing
    r = _cli("--seed", str(seed), "--seed-structure", "--seed-merged", str(out), fa)
    assert r.returncode != 0 and "--seed-merged needs --seed-each" in r.stderr and r.stdout == ""
    r = _cli("--seed-merged", str(out), fa)
    assert r.returncode != 0 and "--seed-merged needs --seed-each" in r.stderr and r.stdout == ""
    r = _cli("--seed", str(seed), "--seed-structure", "--seed-each", "--seed-merged", "", fa)
    assert r.returncode != 0 and "--seed-merged needs a file name" in r.stderr and r.stdout == ""
    # everything --seed-each refuses stays refused
    for opt in (["-r", "2"], ["--bp-update"], ["--bp-update1"], ["--devices", "0,1"], ["--pairwise"]):
        r = _cli("--seed", str(seed), "--seed-structure", "--seed-each", "--seed-merged", str(out), *opt, fa)
        assert r.returncode != 0 and "--seed" in r.stderr and r.stdout == "", opt
    assert not out.exists()
    # the Python driver's other refusals are add_each's
    with pytest.raises(ValueError):
        pipeline.add_each(SEED_NAMES, SEED_ROWS, ["x"], ["ACGU"], merged=True, seed_ss=np.array(SEED_SS, np.uint32), bp_update1=True)
    with pytest.raises(ValueError):
        pipeline.add_each(SEED_NAMES, SEED_ROWS, [], [], merged=True, seed_ss=np.array(SEED_SS, np.uint32))


def test_cli_help_names_the_option():
    r = _cli("--help")
    assert r.returncode == 0 and "--seed-merged OUT" in r.stdout and "read again as a SEED" in r.stdout


def test_estimate_and_budget():
    one = int(capi._reliability_bytes(2, 170))
    assert 18 * 2 * 170 < one < 16384 and int(capi._reliability_bytes(33, 1000)) > 17 * 33 * 1000
    assert int(capi._reliability_batch_bytes()) == 1 << 30


def test_header_declares_and_library_exports_the_new_symbols():
    text = open(HEADER).read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ("dafs_hip_alignment_reliabilities", "dafs_host_stockholm_block_merged", "dafs_host_reliability_bytes",
                "dafs_host_reliability_batch_bytes", "dafs_host_merged_refusal"):
        assert re.search(r"^(int|uint64_t|const char\*) %s\(" % sym, text, re.M), sym
        assert getattr(lib, sym) is not None
    assert hasattr(capi.Context, "alignment_reliabilities")
