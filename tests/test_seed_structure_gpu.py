"""GPU tests of the seed's consensus structure: constrained folds into the base-pairing store against
the CPU oracle, pipeline.add / add_each with seed_ss, `dafs --seed-structure` against the Python driver, and
dafs_hip_structure_support against the restatement of structure_ref.py.  Every comparison is bit for bit."""
import functools
import os
import subprocess

import numpy as np
import pytest

import structure_ref as ref
from dafs_amd import capi, pipeline, stockholm, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = 0xFFFFFFFF


def _oracle_rows(oracle, seq, constraint):
    L = len(seq)
    rp = np.zeros(L + 1, np.uint32); col = np.zeros(L * L + 1, np.uint32); val = np.zeros(L * L + 1, np.float32)
    n = oracle.lib.orc_fold_calculate(seq.encode(), L, constraint.encode() if constraint else None, 0.01, rp.ctypes.data, col.ctypes.data,
                                      val.ctypes.data)
    assert n >= 0
    return rp, col[:n].copy(), val[:n].copy()


def _same_rows(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2].tobytes() == want[2].tobytes()


# ---------------------------------------------------------------------------------------------------------- 1. the store
def test_constrained_folds_into_the_store(oracle):
    seqs = [synth.random_set(1, 45, seed=811, jitter=0.0)[0][1], synth.random_set(1, 30, seed=812, jitter=0.0)[0][1],
            synth.random_set(1, 20, seed=813, jitter=0.0)[0][1], "GGGAAAUCCCAUGCAUGCA", "GGGGAAAACCCCAUAU", "AUGCGCAUA"]
    assert [len(s) for s in seqs] == [45, 30, 20, 19, 16, 9]
    cons = [None, "", "?" * 20,
            "((??????))?????????",  # two nested forced pairs, G.C and G.C
            "?????.??????????",     # a forced '.'
            "???()????"]            # a forced C.G pair around a loop of no residues
    ctx = capi.Context(0)
    ctx.set_sequences(seqs)
    ctx.fold_begin(0.01, constraints=cons)
    ctx.align_posteriors(capi.ALIGN_PROBCONS, 0.01, fetch=False)  # runs beside the folding
    ctx.fold_end()
    got = ctx.bp(0)
    for s, con, rows in zip(seqs, cons, got):
        assert _same_rows(rows, _oracle_rows(oracle, s, con)), con
    # the forced pairs are there with probability 1 (to rounding), the forced '.' pairs with nothing
    rp, col, val = got[3]
    assert 9 in col[rp[0]:rp[1]] and 8 in col[rp[1]:rp[2]]
    rp, col, val = got[4]
    assert rp[6] == rp[5] and 5 not in col
    rp, col, val = got[5]
    assert list(col[rp[3]:rp[4]]) == [4]
    ctx.fold_posteriors(0.01)
    free = ctx.bp(0)
    for k in range(3):
        assert _same_rows(got[k], free[k])
    assert not _same_rows(got[3], free[3])
    # the combined call gives the same store
    ctx.fold_posteriors(0.01, constraints=cons)
    for a, b in zip(ctx.bp(0), got):
        assert _same_rows(a, b)
    # refusals name the sequence and leave the context usable
    bad = [(3, "((??????))"),                  # a short string
           (4, "?????x??????????"),            # an unknown character
           (3, "((??????)??????????"),         # unbalanced
           (5, "??)(?????"),
           (3, "(????(??)???)??????")]         # A.C at the inner pair: CONTRAfold cannot form it
    assert not ref.complementary(seqs[3][5], seqs[3][8])
    for x, con in bad:
        c2 = list(cons)
        c2[x] = con
        for call in (ctx.fold_posteriors, ctx.fold_begin):
            with pytest.raises(capi.DafsHipError, match="sequence %d" % x):
                call(0.01, constraints=c2)
        with pytest.raises(capi.DafsHipError):
            ctx.fold_end()  # nothing is pending after a refusal
        ctx.fold_posteriors(0.01, constraints=cons)
        assert _same_rows(ctx.bp(0)[3], got[3])
    with pytest.raises(ValueError):
        ctx.fold_posteriors(0.01, constraints=cons[:5])
    ctx.close()


# ----------------------------------------------------------------------------------------------- the hand-made seed of 2-5
def _comp(s):
    return "".join({"A": "U", "U": "A", "G": "C", "C": "G"}[ch] for ch in reversed(s))


def _row(stem1, stem2):
    """40 nt: a stem of four pairs at 1-4 / 11-14 around 6 nt, one at 20-23 / 32-35 around 8 nt"""
    return "A" + stem1 + "AAUAAU" + _comp(stem1) + "AUAUA" + stem2 + "UUAAUUAA" + _comp(stem2) + "AUAU"


SEED_STRUCTURE = "." + "((((" + "......" + "))))" + "....." + "<<<<" + "........" + ">>>>" + "...."
SEED_NAMES = ["s0", "s1", "s2", "s3"]


@functools.lru_cache(maxsize=None)
def _seed():
    rows = [_row("GGCG", "CCGG"), _row("GCCG", "CGGC"), _row("GGCG", "CCGG"), _row("GGUG", "CCGG")]
    rows[1] = rows[1][:17] + "-" + rows[1][18:]    # a gap at an unpaired column
    rows[2] = rows[2][:13] + "A" + rows[2][14:]    # the pair 2 -> 13 broken by a substitution
    rows[3] = rows[3][:33] + "-" + rows[3][34:]    # the right residue of the pair 22 -> 33 deleted
    assert len(SEED_STRUCTURE) == 40 and all(len(r) == 40 for r in rows)
    _, ss = ref.clean(rows, SEED_STRUCTURE)
    assert [c for c, p in enumerate(ss) if p != NONE] == [1, 2, 3, 4, 20, 21, 22, 23] and ss[2] == 13 and ss[22] == 33
    assert rows[2][2] == "G" and rows[2][13] == "A" and not ref.complementary("G", "A")
    assert rows[3][33] == "-" and rows[3][22] != "-"
    new_names = ["n0", "n1"]
    base = _row("GGCG", "CUGG")
    new_seqs = [base[:7] + "GG" + base[7:26] + base[28:], base[2:16] + base[19:38]]  # an insertion and deletions in loops; shortened ends
    return rows, np.array(ss, np.uint32), new_names, new_seqs


def _constraints():
    rows, ss, _, _ = _seed()
    return [ref.row_constraint([ch != "-" for ch in r], ss, r.replace("-", "")) for r in rows]


def test_add_with_an_empty_structure_changes_no_alignment():
    rows, _, names, seqs = _seed()
    ctx = capi.Context(0)
    want = pipeline.add(SEED_NAMES, rows, names, seqs, ctx=ctx)
    got = pipeline.add(SEED_NAMES, rows, names, seqs, ctx=ctx, seed_ss=np.full(40, NONE, np.uint32))
    ctx.close()
    assert got.rows == want.rows and [z.tobytes() for z in got.z] == [z.tobytes() for z in want.z]
    assert (got.ss == NONE).all() and got.ss_str == "." * len(got.rows[0])
    for key in ("both", "canonical", "half"):
        assert not got.support[key].any()
    assert got.support["expected"].tobytes() == np.zeros(6).tobytes()


@functools.lru_cache(maxsize=None)
def _added():
    rows, ss, names, seqs = _seed()
    ctx = capi.Context(0)
    res = pipeline.add(SEED_NAMES, rows, names, seqs, ctx=ctx, seed_ss=ss, reliability=True)
    raw, relaxed = ctx.bp(0), ctx.bp(1)
    ctx.close()
    return res, raw, relaxed


def test_add_with_the_hand_made_seed(oracle):
    rows, ss, names, seqs = _seed()
    res, raw, relaxed = _added()
    cons = _constraints()
    assert cons[0].count("(") == 8 and cons[2].count("(") == 7 and cons[3].count("(") == 7  # the broken and the half pair stay free
    seed_seqs = [r.replace("-", "") for r in rows]
    want_rows = [_oracle_rows(oracle, s, c) for s, c in zip(seed_seqs, cons)] + [_oracle_rows(oracle, s, None) for s in seqs]
    for got, want in zip(raw, want_rows):
        assert _same_rows(got, want)
    # every z_j from a context prepared by hand from public calls
    ctx = capi.Context(0)
    ctx.set_sequences(seed_seqs + seqs)
    ctx.set_bp(want_rows)
    ctx.align_posteriors(capi.ALIGN_PROBCONS, 0.01, fetch=False)
    ctx.consistency(0.25, 0.25)
    seed_mask = np.array([[ch != "-" for ch in r] for r in rows], np.uint8)
    prm = capi.dd_params(w=4.0, eta0=0.5, th_a=0.01, th_s=0.2, t_max=600, skip_uncoupled_folds=1)
    for j, s in enumerate(seqs):
        out = ctx.solve_nodes([(np.array([4 + j], np.uint32), np.ones((1, len(s)), np.uint8), np.arange(4, dtype=np.uint32), seed_mask)], prm)[0]
        assert out["z"].tobytes() == res.z[j].tobytes()
    ctx.close()
    # the printed structure: the seed's at seed columns, '.' at insert columns; without the new rows and the insert columns
    # the output is the seed
    seed_brackets = capi.make_brackets(ss)
    assert "".join(ch for ch, x in zip(res.ss_str, res.rf) if x) == seed_brackets
    assert all(ch == "." for ch, x in zip(res.ss_str, res.rf) if not x)
    assert res.output.split("\n")[1] == res.ss_str
    assert ["".join(ch for ch, x in zip(r, res.rf) if x) for r in res.rows[:4]] == rows
    assert [r.replace("-", "") for r in res.rows[4:]] == seqs
    seed_col = np.flatnonzero(res.rf)
    assert res.ss.tolist() == ref.carry(ss.tolist(), seed_col.tolist(), len(res.rf))
    # .support: per printed row, from the store the nodes read
    all_seqs = seed_seqs + seqs
    for r, row in enumerate(res.rows):
        want = ref.support([ch != "-" for ch in row], res.ss.tolist(), all_seqs[r], relaxed[r])
        got = tuple(res.support[k][r] for k in ("both", "canonical", "half", "expected"))
        assert got[:3] == want[:3] and np.float64(got[3]).tobytes() == np.float64(want[3]).tobytes(), r
    assert res.support["both"][:4].tolist() == [8, 8, 8, 7] and res.support["canonical"][:4].tolist() == [8, 8, 7, 7]
    assert res.support["half"][:4].tolist() == [0, 0, 0, 1]
    # the annotations see the carried structure
    assert res.reliability["pair_rows"][seed_col[1]] >= 4 and "#=GC SS_cons" in res.stockholm and res.ss_str in res.stockholm


def _same_result(got, want):
    assert got.output == want.output and got.rows == want.rows and got.ss_str == want.ss_str
    assert got.ss.tobytes() == want.ss.tobytes() and got.rf.tobytes() == want.rf.tobytes()
    assert [z.tobytes() for z in got.z] == [z.tobytes() for z in want.z]
    assert {k: (v[0], v[1], v[2], np.float32(v[3]).tobytes()) for k, v in got.dd_log.items()} == \
        {k: (v[0], v[1], v[2], np.float32(v[3]).tobytes()) for k, v in want.dd_log.items()}
    for key in ("both", "canonical", "half", "expected"):
        assert got.support[key].tobytes() == want.support[key].tobytes()


def test_add_each_equals_add_of_each():
    rows, ss, names, seqs = _seed()
    names, seqs = names + ["n2"], seqs + [synth.random_set(1, 25, seed=821, jitter=0.0)[0][1]]
    ctx = capi.Context(0)
    each = pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=ctx, max_bytes=1, seed_ss=ss)
    assert each.chunks == [[0], [1], [2]]
    one = pipeline.add_each(SEED_NAMES, rows, names, seqs, ctx=ctx, seed_ss=ss)
    assert one.chunks == [[0, 1, 2]]
    for j in range(3):
        want = pipeline.add(SEED_NAMES, rows, [names[j]], [seqs[j]], ctx=ctx, seed_ss=ss)
        _same_result(each.results[j], want)
        _same_result(one.results[j], want)
        for key in ("both", "canonical", "half", "expected"):
            assert each.support[key][j].tobytes() == want.support[key][4].tobytes() == one.support[key][j].tobytes()
    ctx.close()


def _cli(*args):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_equals_python(tmp_path):
    rows, ss, names, seqs = _seed()
    new_fa = tmp_path / "new.fa"
    new_fa.write_text(synth.to_fasta(list(zip(names, seqs))))
    seed_sto, seed_aln = tmp_path / "seed.sto", tmp_path / "seed.aln"
    lines = ["# STOCKHOLM 1.0"]
    for b in (0, 25):  # two interleaved blocks
        lines += [""] + [n.ljust(14) + r[b:b + 25].replace("-", ".") for n, r in zip(SEED_NAMES, rows)] + ["#=GC SS_cons".ljust(14) + SEED_STRUCTURE[b:b + 25]]
    seed_sto.write_text("\n".join(lines + ["//"]) + "\n")
    seed_aln.write_text(">SS_cons\n%s\n" % SEED_STRUCTURE + "".join("> %s\n%s\n" % (n, r) for n, r in zip(SEED_NAMES, rows)))
    for seed in (seed_sto, seed_aln):
        got = stockholm.read_seed_structure(str(seed))
        assert got[0] == SEED_NAMES and got[1] == rows and got[2].tobytes() == ss.tobytes()
    want = _added()[0]
    each = pipeline.add_each(SEED_NAMES, rows, names, seqs, seed_ss=ss, reliability=True)
    each_out = "".join("==> %d <==\n" % (j + 1) + r.output for j, r in enumerate(each.results))
    each_tsv = pipeline.seed_scores_tsv(names, each)
    assert all(len(ln.split("\t")) == 11 for ln in each_tsv.splitlines())
    plain_tsv = pipeline.seed_scores_tsv(names, pipeline.add_each(SEED_NAMES, rows, names, seqs))
    assert all(len(ln.split("\t")) == 7 for ln in plain_tsv.splitlines())
    for seed in (seed_sto, seed_aln):
        sto, tsv = tmp_path / "out.sto", tmp_path / "out.tsv"
        assert _cli("--seed", seed, "--seed-structure", "--stockholm", sto, new_fa) == want.output
        assert sto.read_text() == want.stockholm
        assert _cli("--seed", seed, "--seed-structure", new_fa) == want.output
        assert _cli("--seed", seed, "--seed-structure", "--seed-each", "--stockholm", sto, "--seed-scores", tsv, new_fa) == each_out
        assert sto.read_text() == "".join(r.stockholm for r in each.results)
        assert tsv.read_text() == each_tsv
        assert _cli("--seed", seed, "--seed-each", "--seed-structure", "--seed-scores", tsv, new_fa) == each_out  # the listed transform
        assert tsv.read_text() == each_tsv
    # without the option the table keeps its seven columns
    tsv = tmp_path / "plain.tsv"
    _cli("--seed", seed_sto, "--seed-each", "--seed-scores", tsv, new_fa)
    assert tsv.read_text() == plain_tsv


# --------------------------------------------------------------------------------------------------- 6. structure_support
def _nested(rs, width, density):
    """a random nested structure over `width` columns"""
    ss = [NONE] * width

    def fill(lo, hi):
        while hi - lo >= 1:
            if rs.rand() < density:
                ss[lo] = hi
                lo, hi = lo + 1, hi - 1
            elif rs.rand() < 0.5:
                lo += 1
            else:
                hi -= 1
            if hi - lo > 6 and rs.rand() < 0.15:
                mid = int(rs.randint(lo + 2, hi - 2))
                fill(lo, mid)
                lo = mid + 1
    fill(0, width - 1)
    return ss


@functools.lru_cache(maxsize=None)
def _support_case():
    rs = np.random.RandomState(77)
    shapes = [(1, 1), (3, 63), (4, 64), (2, 65), (5, 130), (1, 40), (3, 50)]  # (rows, columns); the last has an empty structure
    seqs, alns, sss = [], [], []
    for a, (n, width) in enumerate(shapes):
        ss = [NONE] * width if a == len(shapes) - 1 else _nested(rs, width, 0.6)
        mask = np.zeros((n, width), np.uint8)
        idx = []
        for r in range(n):
            keep = rs.rand(width) < (1.0 if width == 1 else 0.8)
            if not keep.any():
                keep[0] = True
            mask[r] = keep
            idx.append(len(seqs))
            seqs.append("".join(rs.choice(list("ACGUUGCAT")) for _ in range(int(keep.sum()))))
        alns.append((np.array(idx, np.uint32), mask))
        sss.append(np.array(ss, np.uint32))
    # the base-pairing rows: most of the structure's pairs that a row holds, some not, and entries beside them
    rows = []
    x = 0
    for (idx, mask), ss in zip(alns, sss):
        for r in range(len(idx)):
            pos = ref.residue_at(mask[r])
            cells = {}
            for c, p in enumerate(ss.tolist()):
                if p != NONE and pos[c] is not None and pos[p] is not None and rs.rand() < 0.7:
                    cells[(pos[c], pos[p])] = np.float32(0.02 + 0.97 * rs.rand())
            L = len(seqs[x])
            for _ in range(L):
                i = int(rs.randint(0, L)); j = int(rs.randint(0, L))
                if i < j and (i, j) not in cells and rs.rand() < 0.5:
                    cells[(i, j)] = np.float32(0.02 + 0.3 * rs.rand())
            rowptr, col, val = [0], [], []
            for i in range(L):
                for (_, j) in sorted(k for k in cells if k[0] == i):
                    col.append(j); val.append(cells[(i, j)])
                rowptr.append(len(col))
            rows.append((np.array(rowptr, np.uint32), np.array(col, np.uint32), np.array(val, np.float32)))
            x += 1
    # the one-row alignment of 40 columns names a sequence of its own; a second one-row alignment reuses sequence 1
    alns.append((np.array([1], np.uint32), np.ones((1, len(seqs[1])), np.uint8)))
    sss.append(np.array(_nested(rs, len(seqs[1]), 0.7), np.uint32))
    return seqs, rows, alns, sss


def _support_want(seqs, rows, alns, sss):
    out = []
    for (idx, mask), ss in zip(alns, sss):
        out.append([ref.support(mask[r].tolist(), ss.tolist(), seqs[int(x)], rows[int(x)]) for r, x in enumerate(idx)])
    return out


def _support_same(got, want):
    for g, w in zip(got, want):
        assert [tuple(int(g[k][r]) for k in ("both", "canonical", "half")) for r in range(len(w))] == [t[:3] for t in w]
        assert g["expected"].tobytes() == np.array([t[3] for t in w], np.float64).tobytes()


def test_structure_support_against_the_restatement():
    seqs, rows, alns, sss = _support_case()
    want = _support_want(seqs, rows, alns, sss)
    flat = [t for w in want for t in w]
    # the case holds what it is meant to: half pairs, non-canonical pairs, pairs that are not stored, an empty structure
    assert any(t[2] for t in flat) and any(t[1] < t[0] for t in flat) and any(t[3] > 1.0 for t in flat)
    held = stored = 0
    for (idx, mask), ss in zip(alns, sss):
        for r, x in enumerate(idx):
            pos = ref.residue_at(mask[r])
            rp, col, _ = rows[int(x)]
            for c, p in enumerate(ss.tolist()):
                if p != NONE and pos[c] is not None and pos[p] is not None:
                    held += 1
                    stored += int(pos[p] in col[rp[pos[c]]:rp[pos[c] + 1]])
    assert 0 < stored < held
    assert want[6] == [(0, 0, 0, 0.0)] * 3 and [m.shape[1] for _, m in alns[:6]] == [1, 63, 64, 65, 130, 40]
    ctx = capi.Context(0)
    ctx.set_sequences(seqs)
    with pytest.raises(capi.DafsHipError):  # no base-pairing store yet
        ctx.structure_support(alns, sss)
    ctx.set_bp(rows)
    got = ctx.structure_support(alns, sss)
    _support_same(got, want)
    assert ctx.structure_support([], []) == []
    # one alignment at a time gives the same as the batch
    for a in (1, 4, 7):
        _support_same(ctx.structure_support([alns[a]], [sss[a]]), [want[a]])
    # refusals, each with the context usable afterwards
    idx, mask = alns[2]
    ss = sss[2].copy()
    c1 = int(np.flatnonzero(ss != NONE)[0])
    bad_ss = []
    for edit in ((c1, c1), (c1, 64), (int(ss[c1]), c1)):  # a partner that is the column itself, outside, to the left
        b = ss.copy(); b[edit[0]] = edit[1]; bad_ss.append(b)
    b = ss.copy(); b[c1 + 1] = ss[c1]; bad_ss.append(b)     # a column in two pairs
    for b in bad_ss:
        with pytest.raises(capi.DafsHipError):
            ctx.structure_support([alns[1], (idx, mask)], [sss[1], b])
        _support_same(ctx.structure_support([alns[1]], [sss[1]]), [want[1]])
    short = mask.copy()
    short[0, int(np.flatnonzero(short[0])[0])] = 0          # a mask that does not place its sequence
    for bad in ((idx, short), (np.array([len(seqs)] + idx.tolist()[1:], np.uint32), mask)):  # ... and an unknown sequence
        with pytest.raises(capi.DafsHipError):
            ctx.structure_support([alns[1], bad], [sss[1], sss[2]])
        _support_same(ctx.structure_support([alns[2]], [sss[2]]), [want[2]])
    ctx.fold_begin(0.01)
    with pytest.raises(capi.DafsHipError):  # a folding in flight: the store is not there
        ctx.structure_support(alns, sss)
    ctx.fold_end()
    ctx.set_bp(rows)
    _support_same(ctx.structure_support(alns, sss), want)
    ctx.close()
