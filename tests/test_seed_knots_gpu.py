"""GPU tests of a seed structure whose pairs may cross: several folds per sequence merged into the
base-pairing store (dafs_hip_fold_posteriors_levels, k_bp_compact_levels) against the CPU oracle's folds merged by knots_ref.py,
pipeline.add / add_each with seed_level, and `dafs --knots` against the Python drivers.  Every comparison is bit for bit."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import knots_ref as ref
import structure_ref
from dafs_amd import capi, pipeline, stockholm, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE, FREE = 0xFFFFFFFF, 0xFF


def _oracle_dense(oracle, seq, constraint, th):
    """the dense triangle of one fold, from orc_fold_calculate's rows at th (0 where it keeps nothing)"""
    L = len(seq)
    rp = np.zeros(L + 1, np.uint32); col = np.zeros((L + 1) * (L + 1) + 1, np.uint32); val = np.zeros((L + 1) * (L + 1) + 1, np.float32)
    n = oracle.lib.orc_fold_calculate(seq.encode(), L, constraint.encode() if constraint else None, th, rp.ctypes.data, col.ctypes.data,
                                      val.ctypes.data)
    assert n >= 0
    dense = np.full((L + 1) * (L + 2) // 2, -np.inf if th < 0 else 0.0, np.float32)
    for i in range(1, L + 1):
        off = i * (2 * (L + 1) - i - 1) // 2
        for k in range(int(rp[i - 1]), int(rp[i])):
            dense[off + int(col[k]) + 1] = val[k]
    return dense


def _want_rows(oracle, seq, cons, th=0.01):
    """the store rows of a sequence folded under each string of cons that is neither None nor empty (once, free, when none is)"""
    folds = [c for c in ([cons] if cons is None or isinstance(cons, str) else cons) if c]
    return ref.merge_rows([_oracle_dense(oracle, seq, c, th) for c in (folds or [None])], len(seq), th)


def _same_rows(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()


def _planted(L, seed):
    """a random sequence of L nt with two crossing stems of two G.C pairs planted, and its two constraints"""
    s = list(synth.random_set(1, L, seed=seed, jitter=0.0)[0][1])
    a, b = [(1, L - 10), (2, L - 11)], [(8, L - 2), (9, L - 3)]
    for i, j in a + b:
        s[i], s[j] = "G", "C"
    cons = []
    for mine, other in ((a, b), (b, a)):
        c = ["?"] * L
        for i, j in mine:
            c[i], c[j] = "(", ")"
        for i, j in other:
            c[i] = c[j] = "."
        cons.append("".join(c))
    return "".join(s), cons


@functools.lru_cache(maxsize=None)
def _store_case():
    seqs, cons = ["GAGACAC"], [["(?.?)?.", ".?(?.?)"]]  # the smallest forced knot: both pairs of "(.[.).]"
    for L in (63, 64, 65):  # the wavefront edge of the compaction
        s, c = _planted(L, 2600 + L)
        seqs.append(s); cons.append(c)
    s, c = _planted(130, 2730)  # K = 3 with the middle level skipped
    seqs.append(s); cons.append([c[0], "", c[1]])
    seqs.append(synth.random_set(1, 50, seed=2650, jitter=0.0)[0][1]); cons.append(None)       # no string: folded once, free
    seqs.append(synth.random_set(1, 33, seed=2633, jitter=0.0)[0][1]); cons.append([None, None, ""])  # the same, said with three entries
    seqs.append("GGGAAAUCCCAUGCAUGCA"); cons.append(["((??????))?????????"])                   # K = 1
    return seqs, cons


def _launches(c, fn):
    c.stage_timing(True)
    try:
        c.stage_report()
        out = fn()
        rep = c.stage_report()
    finally:
        c.stage_timing(False)
    return out, {k: v[2] for k, v in rep.items()}


# ---------------------------------------------------------------------------------------------------------- 1. the store
def test_level_folds_into_the_store(oracle):
    seqs, cons = _store_case()
    assert [len(s) for s in seqs] == [7, 63, 64, 65, 130, 50, 33, 19]
    ctx = capi.Context(0)
    ctx.set_sequences(seqs)

    def fold():
        ctx.fold_begin(0.01, constraints=cons)
        ctx.align_posteriors(capi.ALIGN_PROBCONS, 0.01, fetch=False)  # runs beside the folding
        ctx.fold_end()
    _, launches = _launches(ctx, fold)
    assert launches.get("k_bp_compact_levels") == 1 and "k_bp_compact" not in launches
    got = ctx.bp(0)
    want = [_want_rows(oracle, s, c) for s, c in zip(seqs, cons)]
    for x, (g, w) in enumerate(zip(got, want)):
        assert _same_rows(g, w), x
    # both pairs of the seven-column knot are in the store, each at its own fold's value
    rp, col, val = got[0]
    assert 4 in col[rp[0]:rp[1]] and 6 in col[rp[2]:rp[3]]
    for lv, (i, j) in enumerate([(0, 4), (2, 6)]):
        alone = _want_rows(oracle, seqs[0], cons[0][lv])
        mine = alone[2][alone[0][i]:alone[0][i + 1]][list(alone[1][alone[0][i]:alone[0][i + 1]]).index(j)]
        assert val[rp[i]:rp[i + 1]][list(col[rp[i]:rp[i + 1]]).index(j)].tobytes() == mine.tobytes()
    # the merge changed something: no single fold of a planted sequence gives its rows
    assert not _same_rows(got[2], _want_rows(oracle, seqs[2], cons[2][0])) and not _same_rows(got[2], _want_rows(oracle, seqs[2], cons[2][1]))
    # the combined call gives the same store
    ctx.fold_posteriors(0.01, constraints=cons)
    for a, b in zip(ctx.bp(0), got):
        assert _same_rows(a, b)
    ctx.close()


def test_one_level_is_the_constrained_call():
    seqs, cons = _store_case()
    one = [c[0] if isinstance(c, list) else c for c in cons]
    ctx = capi.Context(0)
    ctx.set_sequences(seqs)
    _, launches = _launches(ctx, lambda: ctx.fold_posteriors(0.01, constraints=one))
    assert launches.get("k_bp_compact") == 1 and "k_bp_compact_levels" not in launches  # the existing call launches what it did
    want = ctx.bp(0)
    _, launches = _launches(ctx, lambda: ctx.fold_posteriors(0.01, constraints=[[c] for c in one]))
    assert launches.get("k_bp_compact_levels") == 1 and "k_bp_compact" not in launches
    for a, b in zip(ctx.bp(0), want):
        assert _same_rows(a, b)
    nnz, nrp = capi.C.c_uint64(), capi.C.c_uint64()
    capi.check(capi._bp_result_size(ctx._h, 0, capi.C.byref(nnz), capi.C.byref(nrp)))
    assert nnz.value == sum(len(r[1]) for r in want) and nrp.value == sum(len(s) + 1 for s in seqs)
    ctx.close()


def test_overflow_retry(oracle):
    """The entry pool starts at 8 entries per residue + 1 024.  At a threshold below every posterior all L (L + 1) / 2 cells of
    a sequence are kept: 8 515 for 130 nt against a pool of 2 120, so the first launch reports the overflow and the second,
    with the reported size, fills the store."""
    seqs, cons = _store_case()
    seqs, cons = [seqs[4], seqs[0]], [cons[4], cons[0]]
    assert sum(len(s) * (len(s) + 1) // 2 for s in seqs) > 8 * sum(len(s) for s in seqs) + 1024
    ctx = capi.Context(0)
    ctx.set_sequences(seqs)
    _, launches = _launches(ctx, lambda: ctx.fold_posteriors(-1.0, constraints=cons))
    assert launches.get("k_bp_compact_levels") == 2
    for x, (g, s, c) in enumerate(zip(ctx.bp(0), seqs, cons)):
        assert len(g[1]) == len(s) * (len(s) + 1) // 2
        assert _same_rows(g, _want_rows(oracle, s, c, -1.0)), x
    ctx.close()


def test_refusals_leave_the_context_usable(oracle):
    seqs = ["GAGACAC", "GGGAAAUCCCAUGCAUGCA"]
    good = [["(?.?)?.", ".?(?.?)"], ["((??????))?????????", None]]
    ctx = capi.Context(0)
    ctx.set_sequences(seqs)
    ctx.fold_posteriors(0.01, constraints=good)
    want = ctx.bp(0)
    assert _same_rows(want[0], _want_rows(oracle, seqs[0], good[0]))
    assert not structure_ref.complementary(seqs[1][5], seqs[1][8])
    bad = [(0, 1, ".?(?.?"),                   # a short string
           (1, 0, "((??????))????x????"),      # an unknown character
           (0, 1, ".?(?.??"),                  # unbalanced
           (1, 1, "??)(???????????????"),
           (1, 1, "(????(??)???)??????")]      # A.C at the inner pair: CONTRAfold cannot form it
    for x, k, con in bad:
        c2 = [list(c) for c in good]
        c2[x][k] = con
        for call in (ctx.fold_posteriors, ctx.fold_begin):
            with pytest.raises(capi.DafsHipError, match="sequence %d, level %d" % (x, k)):
                call(0.01, constraints=c2)
        with pytest.raises(capi.DafsHipError):
            ctx.fold_end()  # nothing is pending after a refusal
        ctx.fold_posteriors(0.01, constraints=good)
        assert all(_same_rows(a, b) for a, b in zip(ctx.bp(0), want))
    with pytest.raises(capi.DafsHipError, match="5 levels"):  # nlevels outside 1..4
        ctx.fold_posteriors(0.01, constraints=[["(?.?)?."] * 5, None])
    arr = (capi.C.c_char_p * 2)(None, None)
    assert capi._fold_levels(ctx._h, 0, 0.01, 0, arr) == -1 and "0 levels" in capi._last_error().decode()
    ctx.fold_posteriors(0.01, constraints=good)
    assert all(_same_rows(a, b) for a, b in zip(ctx.bp(0), want))
    with pytest.raises(ValueError):
        ctx.fold_posteriors(0.01, constraints=good[:1])
    ctx.close()


# ----------------------------------------------------------------------------------------------- the hand-made seed of 2-4
def _comp(s):
    return "".join({"A": "U", "U": "A", "G": "C", "C": "G"}[ch] for ch in reversed(s))


def _row(stem_a, stem_b):
    """40 nt with an H-type knot: stem A, five pairs, at 1-5 / 18-22; stem B, four pairs, at 10-13 / 30-33"""
    return "A" + stem_a + "AAUA" + stem_b + "AUAA" + _comp(stem_a) + "AAUAAUA" + _comp(stem_b) + "AUAUAU"


SEED_STRUCTURE = "." + "(((((" + "...." + "[[[[" + "...." + ")))))" + "......." + "]]]]" + "......"
SEED_NAMES = ["s0", "s1", "s2", "s3"]


@functools.lru_cache(maxsize=None)
def _seed():
    rows = [_row("GGCGC", "CCGG"), _row("GCCGG", "CGGC"), _row("GGCGC", "CCGG"), _row("GGUGC", "CCGG")]
    rows[1] = rows[1][:25] + "-" + rows[1][26:]    # a gap at an unpaired column
    rows[2] = rows[2][:31] + "A" + rows[2][32:]    # the level-1 pair 12 -> 31 broken by a substitution
    rows[3] = rows[3][:20] + "-" + rows[3][21:]    # the right residue of the level-0 pair 3 -> 20 deleted
    assert len(SEED_STRUCTURE) == 40 and all(len(r) == 40 for r in rows)
    _, ss, level = ref.clean(rows, SEED_STRUCTURE)
    assert [c for c, p in enumerate(ss) if p != NONE] == [1, 2, 3, 4, 5, 10, 11, 12, 13] and ss[3] == 20 and ss[12] == 31
    assert [level[c] for c in (1, 5, 18, 22)] == [0] * 4 and [level[c] for c in (10, 13, 30, 33)] == [1] * 4
    assert rows[2][12] == "G" and not structure_ref.complementary("G", rows[2][31])
    new_names = ["n0", "n1"]
    base = _row("GGCGC", "CUGG")
    new_seqs = [base[:8] + "GG" + base[8:24] + base[26:], base[1:15] + base[17:38]]  # an insertion and deletions in loops; shortened ends
    return rows, np.array(ss, np.uint32), np.array(level, np.uint8), new_names, new_seqs


def _constraints():
    rows, ss, level, _, _ = _seed()
    return [ref.row_constraints([ch != "-" for ch in r], ss.tolist(), level.tolist(), 2, r.replace("-", "")) for r in rows]


@functools.lru_cache(maxsize=None)
def _added():
    rows, ss, level, names, seqs = _seed()
    ctx = capi.Context(0)
    res = pipeline.add(SEED_NAMES, rows, names, seqs, ctx=ctx, seed_ss=ss, seed_level=level, reliability=True)
    raw, relaxed = ctx.bp(0), ctx.bp(1)
    ctx.close()
    return res, raw, relaxed


def test_add_with_the_hand_made_knotted_seed(oracle):
    rows, ss, level, names, seqs = _seed()
    res, raw, relaxed = _added()
    cons = _constraints()
    assert [c[0].count("(") for c in cons] == [5, 5, 5, 4] and [c[1].count("(") for c in cons] == [4, 4, 3, 4]
    assert cons[2][0].count(".") == 8 and cons[3][1].count(".") == 8  # a broken pair is still excluded; a half pair stays free
    seed_seqs = [r.replace("-", "") for r in rows]
    want_rows = [_want_rows(oracle, s, c) for s, c in zip(seed_seqs, cons)] + [_want_rows(oracle, s, None) for s in seqs]
    for x, (got, want) in enumerate(zip(raw, want_rows)):
        assert _same_rows(got, want), x
    # the printed structure: "()" and "[]" at the seed's columns, '.' at insert columns; without the new rows and the insert
    # columns the output is the seed
    seed_brackets = capi.make_brackets_levels(ss, level)
    assert seed_brackets == SEED_STRUCTURE
    assert "".join(ch for ch, x in zip(res.ss_str, res.rf) if x) == seed_brackets
    assert all(ch == "." for ch, x in zip(res.ss_str, res.rf) if not x)
    assert res.output.split("\n")[1] == res.ss_str and "[" in res.ss_str and "(" in res.ss_str
    assert ["".join(ch for ch, x in zip(r, res.rf) if x) for r in res.rows[:4]] == rows
    assert [r.replace("-", "") for r in res.rows[4:]] == seqs
    seed_col = np.flatnonzero(res.rf)
    assert res.ss.tolist() == structure_ref.carry(ss.tolist(), seed_col.tolist(), len(res.rf))
    assert res.ss_level.dtype == np.uint8 and res.ss_level.tolist() == ref.carry_levels(level.tolist(), seed_col.tolist(), len(res.rf))
    # .support: per printed row, the merged structure against the store the nodes read
    all_seqs = seed_seqs + seqs
    for r, row in enumerate(res.rows):
        want = structure_ref.support([ch != "-" for ch in row], res.ss.tolist(), all_seqs[r], relaxed[r])
        got = tuple(res.support[k][r] for k in ("both", "canonical", "half", "expected"))
        assert got[:3] == want[:3] and np.float64(got[3]).tobytes() == np.float64(want[3]).tobytes(), r
    assert res.support["both"][:4].tolist() == [9, 9, 9, 8] and res.support["canonical"][:4].tolist() == [9, 9, 8, 8]
    assert res.support["half"][:4].tolist() == [0, 0, 0, 1]
    assert "#=GC SS_cons" in res.stockholm and res.ss_str in res.stockholm


def test_all_zero_levels_change_no_byte():
    """a nested structure with its level array (0 at every pair) gives what seed_ss alone gives"""
    rows, ss, level, names, seqs = _seed()
    nested = np.where(level == 0, ss, NONE).astype(np.uint32)
    zeros = np.where((level == 0), 0, FREE).astype(np.uint8)
    assert (zeros[nested[nested != NONE]] == 0).all()
    ctx = capi.Context(0)
    want = pipeline.add(SEED_NAMES, rows, names, seqs, ctx=ctx, seed_ss=nested, reliability=True)
    want_raw = ctx.bp(0)
    got = pipeline.add(SEED_NAMES, rows, names, seqs, ctx=ctx, seed_ss=nested, seed_level=zeros, reliability=True)
    got_raw = ctx.bp(0)
    ctx.close()
    assert got.output == want.output and got.stockholm == want.stockholm and got.ss_str == want.ss_str and got.rows == want.rows
    assert got.ss.tobytes() == want.ss.tobytes() and [z.tobytes() for z in got.z] == [z.tobytes() for z in want.z]
    assert all(_same_rows(a, b) for a, b in zip(got_raw, want_raw))
    for key in ("both", "canonical", "half", "expected"):
        assert got.support[key].tobytes() == want.support[key].tobytes()


def _same_result(got, want):
    assert got.output == want.output and got.rows == want.rows and got.ss_str == want.ss_str
    assert got.ss.tobytes() == want.ss.tobytes() and got.rf.tobytes() == want.rf.tobytes() and got.ss_level.tobytes() == want.ss_level.tobytes()
    assert [z.tobytes() for z in got.z] == [z.tobytes() for z in want.z]
    for key in ("both", "canonical", "half", "expected"):
        assert got.support[key].tobytes() == want.support[key].tobytes()


def test_add_each_equals_add_of_each():
    rows, ss, level, names, seqs = _seed()
    ctx = capi.Context(0)
    each = pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=ctx, max_bytes=1, seed_ss=ss, seed_level=level)
    assert each.chunks == [[0], [1]]
    for j in range(2):
        want = pipeline.add(SEED_NAMES, rows, [names[j]], [seqs[j]], ctx=ctx, seed_ss=ss, seed_level=level)
        _same_result(each.results[j], want)
        for key in ("both", "canonical", "half", "expected"):
            assert each.support[key][j].tobytes() == want.support[key][4].tobytes()
    ctx.close()


def _cli(*args):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _seed_file(tmp_path, structure=SEED_STRUCTURE):
    rows = _seed()[0]
    seed = tmp_path / "seed.sto"
    seed.write_text("# STOCKHOLM 1.0\n" + "".join("%s %s\n" % (n, r) for n, r in zip(SEED_NAMES, rows)) + "#=GC SS_cons %s\n//\n" % structure)
    return seed


def test_cli_seed_structure_knots_equals_python(tmp_path):
    rows, ss, level, names, seqs = _seed()
    new_fa, sto = tmp_path / "new.fa", tmp_path / "out.sto"
    new_fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    want = _added()[0]
    # Rfam's marks for the same structure: "<>" for the nested stem, letters for the knot
    for structure in (SEED_STRUCTURE, SEED_STRUCTURE.replace("(", "<").replace(")", ">").replace("[", "A").replace("]", "a")):
        seed = _seed_file(tmp_path, structure)
        got = stockholm.read_seed_knots(str(seed))
        assert got[0] == SEED_NAMES and got[1] == rows and got[2].tobytes() == ss.tobytes() and got[3].tobytes() == level.tobytes()
        assert _cli("--seed", seed, "--seed-structure", "--knots", "--stockholm", sto, new_fa) == want.output
        assert sto.read_text() == want.stockholm
    # without --knots the seed is refused as before
    r = subprocess.run([DAFS, "--seed", str(_seed_file(tmp_path)), "--seed-structure", str(new_fa)], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "cross" in r.stderr and r.stdout == ""
    cov = tmp_path / "cov.txt"
    with_cov = pipeline.add(SEED_NAMES, rows, names, seqs, seed_ss=ss, seed_level=level, covariation=True)
    assert _cli("--seed", _seed_file(tmp_path), "--seed-structure", "--knots", "--covariation", cov, new_fa) == with_cov.output
    assert cov.read_text() == pipeline.covariation_tsv(with_cov)


def test_cli_seed_each_merged_is_a_seed_again(tmp_path):
    rows, ss, level, names, seqs = _seed()
    new_fa, out, tsv = tmp_path / "new.fa", tmp_path / "merged.sto", tmp_path / "scores.tsv"
    new_fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    seed = _seed_file(tmp_path)
    ctx = capi.Context(0)
    each = pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=ctx, seed_ss=ss, seed_level=level, merged=True)
    mg = each.merged
    want_out = "".join("==> %d <==\n" % (j + 1) + r.output for j, r in enumerate(each.results))
    assert _cli("--seed", seed, "--seed-structure", "--knots", "--seed-each", "--seed-merged", out, "--seed-scores", tsv, new_fa) == want_out
    assert out.read_text() == mg.stockholm and "[" in mg.ss_str and mg.ss_str in mg.stockholm
    assert tsv.read_text() == pipeline.seed_scores_tsv(names, each)
    seed_col = np.flatnonzero(mg.rf)
    assert mg.ss_level.tolist() == ref.carry_levels(level.tolist(), seed_col.tolist(), len(mg.rf))
    # OUT is a seed again, with --knots: its own rows and structure come back
    with pytest.raises(stockholm.SeedError, match="cross"):
        stockholm.read_seed_structure(str(out))
    got = stockholm.read_seed_knots(str(out))
    assert got[0] == mg.names and got[1] == mg.rows and got[2].tobytes() == mg.ss.tobytes() and got[3].tobytes() == mg.ss_level.tobytes()
    extra = synth.random_set(1, 38, seed=2652, jitter=0.0)[0][1]
    again = pipeline.add(got[0], got[1], ["extra"], [extra], ctx=ctx, seed_ss=got[2], seed_level=got[3])
    ctx.close()
    assert ["".join(ch for ch, x in zip(r, again.rf) if x) for r in again.rows[:len(mg.rows)]] == mg.rows
    assert "".join(ch for ch, x in zip(again.ss_str, again.rf) if x) == mg.ss_str
    extra_fa = tmp_path / "extra.fa"
    extra_fa.write_text(">extra\n%s\n" % extra)
    assert _cli("--seed", out, "--seed-structure", "--knots", extra_fa) == again.output


def test_cli_describe_and_compare_ref_read_a_levels_output(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from time_levels import planted_family
    finally:
        sys.path.pop(0)
    recs, pairs_a, pairs_b = planted_family()
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    fa, sto, cov, cmp_out = tmp_path / "knot.fa", tmp_path / "knot.sto", tmp_path / "cov.txt", tmp_path / "cmp.txt"
    fa.write_text(synth.to_fasta(recs))
    lv = ("--fold-decoder", "Levels", "-G", "2,4")
    printed = _cli(*lv, "--stockholm", sto, fa)
    brackets = printed.split("\n")[2]
    assert "[" in brackets and "(" in brackets  # the planted knot: two bracket kinds that cross
    # the reader gives the decode's structure and levels again
    rnames, rows, ss, level = stockholm.read_seed_knots(str(sto))
    assert capi.make_brackets_levels(ss, level) == brackets
    # --describe --knots prints the bracket line; the covariation table is the Python twin's
    out = _cli("--describe", sto, "--knots", "--covariation", cov)
    assert out == ">SS_cons\n%s\n" % brackets
    twin = pipeline.describe(rnames, rows, ss=ss, level=level, identity=False, covariation=True)
    assert twin.ss_str == brackets and cov.read_text() == pipeline.covariation_tsv(twin)
    r = subprocess.run([DAFS, "--describe", str(sto), "--covariation", str(cov)], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "cross" in r.stderr  # without --knots as before
    # --compare-ref --knots: the Levels output against itself; "# structure" counts the pairs of all levels
    _cli("--describe", sto, "--knots", "--compare", cmp_out, "--compare-ref", sto)
    reference = (rnames, rows, ss)
    twin = pipeline.describe(rnames, rows, ss=ss, level=level, identity=False, compare=reference, pp=stockholm.read_seed_pp(str(sto)))
    assert cmp_out.read_text() == twin.compare.table
    line = [ln for ln in twin.compare.table.split("\n") if ln.startswith("# structure")][0].split()
    held = sum(1 for row in rows for i, j in enumerate(ss.tolist()) if j != NONE and row[i] != "-" and row[j] != "-")
    assert int(line[line.index("tp") + 1]) == int(line[line.index("ref") + 1]) == int(line[line.index("test") + 1]) == held
    assert held > len(rows) * len(pairs_a)  # more than stem A alone: the crossing stem is counted
    # a run compared against the knotted reference
    _cli(*lv, "--compare", cmp_out, "--compare-ref", sto, "--knots", fa)
    run = pipeline.run(names, seqs, decoder="Levels", th_s1=(1.0 / 3.0, 1.0 / 5.0), compare=reference)
    assert cmp_out.read_text() == run.compare.table
    r = subprocess.run([DAFS, "--compare", str(cmp_out), "--compare-ref", str(sto), str(fa)], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "cross" in r.stderr
