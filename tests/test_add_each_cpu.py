"""CPU tests of adding each new sequence to a seed on its own (pipeline.add_each, `dafs --seed SEED --seed-each`; DESIGN.md
section 15): the score table's exact bytes, the per-sequence memory estimate and the packing under a budget, the refusal of
bad arguments before any context is opened, the command line's refusals, and the new symbols -- no HIP call."""
import ctypes
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
G = os.path.join(ROOT, "tests", "golden")
HEADER = os.path.join(ROOT, "include", "dafs_hip.h")


def _names_ref(headers):
    """the Stockholm name rule: first word, seq<k> for an empty header, .2, .3, ... for repeats"""
    out, seen = [], {}
    for k, h in enumerate(headers):
        words = h.split()
        nm = words[0] if words else "seq%d" % (k + 1)
        seen[nm] = seen.get(nm, 0) + 1
        out.append(nm if seen[nm] == 1 else "%s.%d" % (nm, seen[nm]))
    return out


def _g9(v):
    v = float(v)
    return "nan" if v != v else "%.9g" % v


def _table_ref(headers, lengths, matched, score, iterations):
    return "".join("%d\t%s\t%d\t%d\t%d\t%s\t%d\n" % (j + 1, nm, lengths[j], matched[j], lengths[j] - matched[j], _g9(score[j]), iterations[j])
                   for j, nm in enumerate(_names_ref(headers)))


class _Each:
    pass


def _each(lengths, matched, score, iterations):
    e = _Each()
    e.results = [None] * len(lengths)
    e.lengths, e.matched = np.array(lengths, np.uint32), np.array(matched, np.uint32)
    e.score, e.iterations = np.array(score, np.float32), np.array(iterations, np.int64)
    return e


def test_seed_table_bytes():
    from dafs_amd import pipeline
    headers = ["tRNA-1 a description", "hit", "", "hit", "  padded\tname", "hit again"]
    lengths = [76, 9, 30, 120, 1, 64]
    matched = [70, 0, 30, 119, 1, 33]
    score = [np.float32(12.3456789), np.float32(np.nan), np.float32(-0.5), np.float32(1234567.875), np.float32(1e-7), np.float32(0)]
    iterations = [37, 600, 1, 0, 2, 599]
    got = pipeline.seed_scores_tsv(headers, _each(lengths, matched, score, iterations))
    assert got == _table_ref(headers, lengths, matched, score, iterations)
    lines = got.split("\n")
    assert lines[0] == "1\ttRNA-1\t76\t70\t6\t12.3456793\t37"
    assert lines[1] == "2\thit\t9\t0\t9\tnan\t600"
    assert lines[2].startswith("3\tseq3\t30\t30\t0\t-0.5\t")
    assert lines[3].startswith("4\thit.2\t")
    assert lines[4].startswith("5\tpadded\t")
    assert lines[5].startswith("6\thit.3\t")
    for ln in lines[:-1]:  # matched + inserted = length
        f = ln.split("\t")
        assert int(f[3]) + int(f[4]) == int(f[2])
    assert pipeline.seed_scores_tsv([], _each([], [], [], [])) == ""
    with pytest.raises(ValueError):  # more matched residues than residues
        pipeline.seed_scores_tsv(["a"], _each([5], [6], [0.0], [1]))
    with pytest.raises(ValueError):
        pipeline.seed_scores_tsv(["a", "b"], _each([5], [5], [0.0], [1]))


def test_seed_each_bytes():
    from dafs_amd import pipeline
    grid = [1, 9, 30, 77, 200]
    for m in (1, 2, 5):
        for seed_lens in itertools.islice(itertools.product(grid, repeat=m), 0, None, 7):
            for cols in (max(seed_lens), max(seed_lens) + 13):
                for ln in grid:
                    want = pipeline.family_bytes(list(seed_lens) + [ln]) + pipeline.node_bytes(ln, cols)
                    assert pipeline.seed_each_bytes(seed_lens, cols, ln) == want
    base = pipeline.seed_each_bytes([50, 60], 70, 40)
    assert pipeline.seed_each_bytes([50, 60], 70, 41) > base      # monotone in the new sequence's length,
    assert pipeline.seed_each_bytes([50, 60], 71, 40) > base      # in the seed's columns,
    assert pipeline.seed_each_bytes([51, 60], 70, 40) > base      # in a seed sequence's length
    assert pipeline.seed_each_bytes([50, 60, 1], 70, 40) > base   # and in the number of seed sequences


def test_packing_under_a_budget():
    from dafs_amd import pipeline
    sizes = [pipeline.seed_each_bytes([60, 62, 58], 70, ln) for ln in (60, 30, 9, 61, 59, 120, 10)]
    assert pipeline.pack_families(sizes, min(sizes) - 1) == [[k] for k in range(len(sizes))]   # smaller than any item
    assert pipeline.pack_families(sizes, 0) == [[k] for k in range(len(sizes))]
    assert pipeline.pack_families([sizes[0]] * 3, sizes[0]) == [[0], [1], [2]]                  # equal to one item
    assert pipeline.pack_families(sizes, sizes[0] + sizes[1]) [0] == [0, 1]
    assert pipeline.pack_families(sizes, 1 << 62) == [list(range(len(sizes)))]                   # large
    for budget in (sizes[2], 2 * max(sizes), sum(sizes) // 3):
        groups = pipeline.pack_families(sizes, budget)
        assert [k for g in groups for k in g] == list(range(len(sizes)))
        assert all(len(g) == 1 or sum(sizes[k] for k in g) <= budget for g in groups)


class _NoContext:
    def __init__(self, *a, **k):
        raise AssertionError("a context was opened before the arguments were checked")


SEED = (["a", "b"], ["ACGU-ACGU", "ACGUAAC-U"])


@pytest.mark.parametrize("args, kw, exc", [
    ((SEED[0], SEED[1], [], []), {}, ValueError),                               # no new sequence
    ((SEED[0], SEED[1], ["x", "y"], ["ACGU"]), {}, ValueError),                 # names and sequences differ in number
    ((SEED[0], SEED[1], ["x"], [""]), {}, ValueError),                          # an empty new sequence
    (([], [], ["x"], ["ACGU"]), {}, ValueError),                                # an empty seed
    ((SEED[0], ["ACGU-ACGU", "ACGU"], ["x"], ["ACGU"]), {}, ValueError),        # seed rows of unequal length
    ((SEED[0], ["ACGU-ACGU", "AC*UAAC-U"], ["x"], ["ACGU"]), {}, ValueError),   # neither a letter nor a gap
    ((SEED[0], ["ACGU-ACGU", "---------"], ["x"], ["ACGU"]), {}, ValueError),   # a row without residues
    ((SEED[0], SEED[1], ["x"], ["ACGU"]), dict(covariation=dict(no_such_key=1)), ValueError),
    ((SEED[0], SEED[1], ["x"], ["ACGU"]), dict(max_bytes=-1), ValueError),
    ((SEED[0], SEED[1], ["x"], ["ACGU"]), dict(no_such_option=1), TypeError),
    ((SEED[0], SEED[1], ["x"], ["ACGU"]), dict(bp_update=True), TypeError),     # not an option of add
])
def test_bad_arguments_refused_before_any_context(monkeypatch, args, kw, exc):
    from dafs_amd import capi, pipeline
    monkeypatch.setattr(capi, "Context", _NoContext)
    with pytest.raises(exc):
        pipeline.add_each(*args, **kw)


def _cli(*args, timeout=60):
    return subprocess.run([DAFS] + list(args), capture_output=True, text=True, timeout=timeout)


def _seed_file(tmp_path):
    p = tmp_path / "seed.fa"
    p.write_text("> a\nACGU-ACGU\n> b\nACGUAAC-U\n")
    return str(p)


def test_cli_seed_each_needs_seed(tmp_path):
    fa = os.path.join(G, "RF00005_0.fa")
    r = _cli("--seed-each", fa)
    assert r.returncode != 0 and "--seed-each needs --seed" in r.stderr and r.stdout == ""
    tsv = tmp_path / "t.tsv"
    r = _cli("--seed", _seed_file(tmp_path), "--seed-scores", str(tsv), fa)
    assert r.returncode != 0 and "--seed-scores needs --seed-each" in r.stderr and r.stdout == ""
    assert not tsv.exists()
    r = _cli("--seed-scores", str(tsv), fa)
    assert r.returncode != 0 and "--seed-scores needs --seed-each" in r.stderr and r.stdout == ""
    r = _cli("--seed", _seed_file(tmp_path), "--seed-each", "--seed-scores", "", fa)
    assert r.returncode != 0 and "--seed-scores needs a file name" in r.stderr and r.stdout == ""


@pytest.mark.parametrize("opt", [["-r", "2"], ["--bp-update"], ["--devices", "0,1"], ["--align-aux", "X"], ["--fold-aux", "X"],
                                 ["--save-align-aux", "X"], ["--save-fold-aux", "X"], ["--pairwise"]])
def test_cli_seed_each_refuses_what_seed_refuses(tmp_path, opt):
    r = _cli("--seed", _seed_file(tmp_path), "--seed-each", *opt, os.path.join(G, "RF00005_0.fa"))
    assert r.returncode != 0 and "--seed" in r.stderr and r.stdout == ""
    r = _cli("--seed", _seed_file(tmp_path), "--seed-each", os.path.join(G, "RF00005_0.fa"), os.path.join(G, "RF00017_4.fa"))
    assert r.returncode != 0 and "exactly one FILE" in r.stderr and r.stdout == ""


def test_cli_help_names_seed_each():
    r = _cli("--help")
    assert r.returncode == 0
    assert "--seed-each " in r.stdout and "--seed-scores OUT" in r.stdout


def test_header_declares_and_library_exports_the_new_symbols():
    from dafs_amd import capi
    text = open(HEADER).read()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for sym in ("dafs_hip_families_from", "dafs_hip_consistency_match_pairs", "dafs_host_seed_table", "dafs_host_seed_each_bytes"):
        assert re.search(r"^(int|uint64_t) %s\(" % sym, text, re.M), sym
        assert getattr(lib, sym) is not None
