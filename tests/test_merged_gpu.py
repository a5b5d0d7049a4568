"""GPU tests of the merged alignment of all placements (pipeline.add_each(merged=True), `dafs --seed-merged`; DESIGN.md section
17): the unchanged per-sequence results, each placement found again in the merged alignment, the values of the new rows from the
listed transform against those of the full one, the order of the new sequences, the chunks, the command line, and the output
read back as a seed.  Every comparison is bit for bit."""
import functools
import os
import subprocess

import numpy as np
import pytest

from dafs_amd import capi, pipeline, stockholm, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = 0xFFFFFFFF


def _comp(s):
    return "".join({"A": "U", "U": "A", "G": "C", "C": "G"}[ch] for ch in reversed(s))


def _row(stem1, stem2):
    """60 nt: a stem of five pairs at 2-6 / 15-19 around 8 nt, one of five at 27-31 / 42-46 around 10 nt"""
    return "AU" + stem1 + "AAUCAAUA" + _comp(stem1) + "AUACAUA" + stem2 + "UUAACUUAAC" + _comp(stem2) + "AUAUCAUACAUAU"


SEED_STRUCTURE = ".." + "(((((" + "........" + ")))))" + "......." + "<<<<<" + ".........." + ">>>>>" + "............."
SEED_NAMES = ["s0", "s1", "s2", "s3", "s4"]


@functools.lru_cache(maxsize=None)
def _seed():
    rows = [_row("GGCGC", "CCGGA"), _row("GCCGC", "CGGCA"), _row("GGCGU", "CCGGA"), _row("GGUGC", "CUGGA"), _row("GGCGC", "CCGGC")]
    rows[1] = rows[1][:22] + "-" + rows[1][23:]    # a gap at an unpaired column
    rows[3] = rows[3][:44] + "-" + rows[3][45:]    # the right residue of a pair deleted
    assert len(SEED_STRUCTURE) == 60 and all(len(r) == 60 for r in rows)
    names, rows, ss = stockholm.clean_seed_structure(SEED_NAMES, rows, SEED_STRUCTURE)
    base = _row("GGCGC", "CUGGA")
    new_names = ["n0 with a head", "n1", "n2", "s1", "n4"]  # a name the seed has already
    new_seqs = ["GACCUGA" + base,                       # residues before the first seed column
                base + "GGAUCCA",                       # a tail past the last seed column
                base[24:50],                            # short: the second stem alone
                base[:9] + "GGG" + base[9:36] + base[39:],  # an insertion and a deletion in loops
                synth.random_set(1, 45, seed=951, jitter=0.0)[0][1]]  # unrelated
    return rows, ss, new_names, new_seqs


class World:
    pass


@pytest.fixture(scope="module")
def world():
    rows, ss, names, seqs = _seed()
    w = World()
    w.ctx = capi.Context(0)
    w.each = pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=w.ctx, seed_ss=ss, merged=True)
    w.plain = pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=w.ctx, seed_ss=ss)
    w.full = pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=w.ctx, seed_ss=ss, reliability=True)
    yield w
    w.ctx.close()


def _same_result(got, want):
    assert got.output == want.output and got.rows == want.rows and got.ss_str == want.ss_str
    assert got.ss.tobytes() == want.ss.tobytes() and got.rf.tobytes() == want.rf.tobytes()
    assert [z.tobytes() for z in got.z] == [z.tobytes() for z in want.z]
    assert {k: (v[0], v[1], v[2], np.float32(v[3]).tobytes()) for k, v in got.dd_log.items()} == \
        {k: (v[0], v[1], v[2], np.float32(v[3]).tobytes()) for k, v in want.dd_log.items()}
    for key in ("both", "canonical", "half", "expected"):
        assert got.support[key].tobytes() == want.support[key].tobytes()


def _same_merged(a, b):
    assert a.names == b.names and a.rows == b.rows and a.ss_str == b.ss_str and a.stockholm == b.stockholm and a.output == b.output
    assert a.rf.tobytes() == b.rf.tobytes() and a.ss.tobytes() == b.ss.tobytes() and a.col.tobytes() == b.col.tobytes()
    assert [z.tobytes() for z in a.z] == [z.tobytes() for z in b.z] and [p.tobytes() for p in a.pp] == [p.tobytes() for p in b.pp]


def test_results_are_unchanged(world):
    assert not hasattr(world.plain, "merged")
    for got, want in zip(world.each.results, world.plain.results):
        _same_result(got, want)
        assert not hasattr(got, "reliability")
    for key in ("score", "iterations", "lengths", "matched"):
        assert getattr(world.each, key).tobytes() == getattr(world.plain, key).tobytes()
    assert world.each.chunks == world.plain.chunks == [[0, 1, 2, 3, 4]]


def test_every_placement_is_found_again(world):
    rows, ss, names, seqs = _seed()
    mg = world.each.merged
    m, k = len(rows), len(seqs)
    assert mg.names == stockholm.names(SEED_NAMES + names) and mg.names[m + 3] == "s1.2"
    assert len(mg.rows) == m + k and [r.replace("-", "") for r in mg.rows[m:]] == seqs
    assert ["".join(ch for ch, x in zip(r, mg.rf) if x) for r in mg.rows[:m]] == rows
    # the head of n0 lies before the first seed column; the aligner ends every placement in the last seed column, so the tail of
    # n1 is the insert block in front of that column
    assert not mg.rf[0] and mg.rows[m][0] != "-" and (mg.z[0][:7] == NONE).all()
    assert mg.rf[-1] and not mg.rf[-2] and (mg.z[1][-8:-1] == NONE).all()
    assert "".join(ch for ch, x in zip(mg.ss_str, mg.rf) if x) == capi.make_brackets(ss) and (mg.ss[~mg.rf] == NONE).all()
    cells = np.array([list(r) for r in mg.rows])
    for j in range(k):
        res = world.each.results[j]
        sub = cells[list(range(m)) + [m + j]]
        keep = (sub != "-").any(0)
        assert ["".join(r) for r in sub[:, keep]] == res.rows, j  # printed order: the seed rows, then the new one
        assert keep[mg.rf].all()
        # the carried structure in the kept columns
        now = np.full(len(keep), NONE, np.int64)
        now[keep] = np.arange(int(keep.sum()))
        proj = np.full(int(keep.sum()), NONE, np.uint32)
        for c in np.flatnonzero(mg.ss != NONE):
            proj[now[c]] = now[mg.ss[c]]
        assert proj.tobytes() == res.ss.tobytes(), j
        assert mg.z[j].tobytes() == res.z[0].tobytes()
        # the new row's values: the listed transform and one wanted row against the full transform and all rows
        assert mg.pp[j].tobytes() == world.full.results[j].reliability["residue"][m].tobytes(), j
        assert len(mg.pp[j]) == len(seqs[j]) and ((mg.pp[j] >= 0) & (mg.pp[j] <= 1)).all()
    # PP_cons: the mean over the new rows of a column, a running sum in input order
    for c in range(len(mg.rf)):
        vals = [mg.pp[j][int((cells[m + j, :c] != "-").sum())] for j in range(k) if cells[m + j, c] != "-"]
        if vals:
            s = 0.0
            for v in vals:
                s += float(v)
            assert np.float64(mg.col[c]).tobytes() == np.float64(s / float(len(vals))).tobytes()
        else:
            assert np.isnan(mg.col[c])
    # with reliability as well the merged alignment is the same one
    _same_merged(pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=world.ctx, seed_ss=ss, merged=True, reliability=True).merged, mg)


def test_one_placement_alone(world):
    rows, ss, names, seqs = _seed()
    one = pipeline.add_each(SEED_NAMES, rows, names[:1], seqs[:1], ctx=world.ctx, seed_ss=ss, merged=True)
    assert one.merged.output == one.results[0].output == world.each.results[0].output
    assert one.merged.pp[0].tobytes() == world.each.merged.pp[0].tobytes()


def test_order_and_chunks_change_nothing(world):
    rows, ss, names, seqs = _seed()
    mg = world.each.merged
    m = len(rows)
    rev = pipeline.add_each(SEED_NAMES, rows, names[::-1], seqs[::-1], ctx=world.ctx, seed_ss=ss, merged=True).merged
    assert rev.rows[:m] == mg.rows[:m] and rev.rows[m:] == mg.rows[m:][::-1]
    assert rev.rf.tobytes() == mg.rf.tobytes() and rev.ss_str == mg.ss_str
    assert [p.tobytes() for p in rev.pp] == [p.tobytes() for p in mg.pp][::-1]
    chunked = pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=world.ctx, seed_ss=ss, merged=True, max_bytes=1)
    assert chunked.chunks == [[0], [1], [2], [3], [4]]
    _same_merged(chunked.merged, mg)


def _cli(*args):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_and_the_output_as_a_seed(world, tmp_path):
    rows, ss, names, seqs = _seed()
    mg = world.each.merged
    seed, new_fa, out, tsv = tmp_path / "seed.sto", tmp_path / "new.fa", tmp_path / "merged.sto", tmp_path / "hits.tsv"
    seed.write_text("# STOCKHOLM 1.0\n" + "".join("%s %s\n" % (n, r) for n, r in zip(SEED_NAMES, rows)) + "#=GC SS_cons %s\n//\n" % SEED_STRUCTURE)
    new_fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    want_out = "".join("==> %d <==\n" % (j + 1) + r.output for j, r in enumerate(world.each.results))
    assert _cli("--seed", seed, "--seed-structure", "--seed-each", "--seed-merged", out, "--seed-scores", tsv, new_fa) == want_out
    assert out.read_text() == mg.stockholm
    assert tsv.read_text() == pipeline.seed_scores_tsv(names, world.each)
    # beside --stockholm: that file and stdout as without the option, OUT the same
    sto, out2 = tmp_path / "each.sto", tmp_path / "merged2.sto"
    assert _cli("--seed", seed, "--seed-structure", "--seed-each", "--stockholm", sto, "--seed-merged", out2, new_fa) == want_out
    assert sto.read_text() == "".join(r.stockholm for r in world.full.results) and out2.read_text() == mg.stockholm
    # OUT is a seed again
    assert stockholm.read_seed(str(out)) == (mg.names, mg.rows)
    got = stockholm.read_seed_structure(str(out))
    assert got[0] == mg.names and got[1] == mg.rows and got[2].tobytes() == mg.ss.tobytes()
    extra = synth.random_set(1, 50, seed=952, jitter=0.0)[0][1]
    again = pipeline.add(got[0], got[1], ["extra"], [extra], ctx=world.ctx, seed_ss=got[2])
    assert ["".join(ch for ch, x in zip(r, again.rf) if x) for r in again.rows[:len(mg.rows)]] == mg.rows
    assert "".join(ch for ch, x in zip(again.ss_str, again.rf) if x) == mg.ss_str
