"""GPU tests of the choice of thresholds by pseudo-expected accuracy: dafs_hip_nussinov_decode_auto and
dafs_hip_consensus_structures_auto against the restatement of tests/auto_ref.py, bit for bit; the anchor to the fixed-threshold
calls; the refusals; the launch counts; the Python drivers with th_s1 a capi.AutoThresholds; the command line with -T auto /
-G auto against those drivers."""
import os
import subprocess

import numpy as np
import pytest

import auto_ref as ref
from dafs_amd import capi, pipeline, stockholm, synth

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NONE, FREE = ref.NONE, ref.FREE
LISTS = {1: (4,), 2: (2, 8), 6: ref.GAMMAS, 16: tuple(range(1, 17))}  # the candidates by their number
WIDTHS = (1, 2, 3, 4, 5, 17, 64, 65, 257, 300)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _auto(C, K):
    return capi.AutoThresholds(LISTS[C], K)


def _first(want, K):
    """the restatement at K levels from the one at four: lower levels do not depend on higher ones"""
    r = ref.Result()
    r.scores = want.scores[:K].copy()
    r.ss, r.level = want.ss.copy(), want.level.copy()
    r.ss[r.level >= K] = NONE  # FREE included: those are NONE already
    r.level[r.level >= K] = FREE
    r.chosen, r.tp, r.npairs = want.chosen[:K], want.tp[:K], want.npairs[:K]
    r.cand_tp, r.cand_pairs, r.sum_p = want.cand_tp[:K], want.cand_pairs[:K], want.sum_p
    r.kept = [c for c in r.chosen if c != NONE]
    return r


# ---- the dense call ----
@pytest.mark.parametrize("case", ref.hand_cases(), ids=lambda c: c.name)
def test_hand_made_cases(case, ctx, oracle):
    got = ctx.nussinov_auto(case.p, capi.AutoThresholds(case.gammas, case.nlevels))
    assert [int(c) for c in got[3].chosen] == case.chosen
    assert capi.make_brackets_levels(got[1], got[2]) == case.text
    want = ref.decode(oracle, case.p, case.cand, case.nlevels)
    assert ref.same(got, want)
    assert got[3].f == want.f and got[3].thresholds.tobytes() == case.cand[want.kept].tobytes()


def _knotted_matrix(rs, L):
    """a sparse random upper triangle with planted stems that cross one another, so that several levels fill"""
    p = np.triu(rs.rand(L, L).astype(np.float32), 1)
    p[rs.rand(L, L) < 0.9] = 0
    p *= np.float32(0.5)
    for _ in range(max(1, L // 12)):
        i, j = sorted(int(x) for x in rs.randint(0, L, 2))
        for k in range(min(4, (j - i - 3) // 2)):
            p[i + k, j - k] = np.float32(0.6 + 0.35 * rs.rand())
    return p


@pytest.fixture(scope="module")
def random_cases(oracle):
    """per width one matrix and, per number of candidates, its restatement at four levels: built once"""
    rs = np.random.RandomState(2727)
    out = {}
    for L in WIDTHS:
        p = _knotted_matrix(rs, L)
        out[L] = (p, {C: ref.decode(oracle, p, ref.candidates(g), 4) for C, g in LISTS.items()})
    return out


@pytest.mark.parametrize("L", WIDTHS)
def test_random_matrices(L, ctx, random_cases):
    p, wants = random_cases[L]
    for C, want in wants.items():
        for K in (1, 2, 3, 4):
            assert ref.same(ctx.nussinov_auto(p, _auto(C, K)), _first(want, K)), (L, C, K)
    if L >= 64:
        assert len(wants[6].kept) >= 2  # crossing pairs were found and kept


def test_global_table_form_gives_the_same_bits(ctx, random_cases, monkeypatch):
    p, wants = random_cases[65]
    monkeypatch.setenv("DAFS_HIP_NUSS_GLOBAL", "1")
    assert ref.same(ctx.nussinov_auto(p, _auto(6, 3)), _first(wants[6], 3))


def test_dense_anchor_to_the_fixed_calls(ctx, random_cases):
    """ss, level and score are those of the fixed-threshold decode at the chosen thresholds; one level is the plain decode"""
    for L in WIDTHS:
        p, wants = random_cases[L]
        for C in (2, 16):
            scores, ss, level, a = ctx.nussinov_auto(p, _auto(C, 4))
            m = len(a.thresholds)
            if m:
                fs, fss, flevel = ctx.nussinov_levels(p, a.thresholds)
                assert fss.tobytes() == ss.tobytes() and flevel.tobytes() == level.tobytes() and fs.tobytes() == scores[:m].tobytes()
            else:
                assert np.all(ss == NONE) and np.all(level == FREE)
            assert np.all(scores[m:] == 0)
            scores, ss, level, a = ctx.nussinov_auto(p, _auto(C, 1))
            if len(a.thresholds):
                s1, ss1 = ctx.nussinov(p, None, float(a.thresholds[0]))
                assert ss1.tobytes() == ss.tobytes() and np.float32(s1).tobytes() == scores[0].tobytes()


def test_one_candidate_is_the_fixed_decode_without_the_levels_that_lower_f(ctx, random_cases):
    """C = 1: the levels of the fixed-threshold decode, up to the first that does not raise F"""
    by_name = {c.name: c for c in ref.hand_cases()}
    dropped = {}
    for name in ("h-type-12", "crosses-nothing"):
        p = by_name[name].p
        fixed = ctx.nussinov_levels(p, (0.2, 0.2))
        scores, ss, level, a = ctx.nussinov_auto(p, capi.AutoThresholds((4,), 2))
        m = len(a.thresholds)
        dropped[name] = int(np.sum(fixed[2] == 1) > 0) - (m - 1)
        assert np.array_equal(ss[level < m], fixed[1][level < m]) and np.array_equal(level != FREE, fixed[2] < m)
        assert scores[:m].tobytes() == fixed[0][:m].tobytes()
    # the H-type's second stem raises F and stays; (3, 10) of the other case, 0.3 against the 0.9 and 0.45 below it, does not
    assert dropped == {"h-type-12": 0, "crosses-nothing": 1}
    th = ref.candidates((4,))
    for L in WIDTHS:
        p, wants = random_cases[L]
        fixed = ctx.nussinov_levels(p, [th[0]] * 4)
        scores, ss, level, a = ctx.nussinov_auto(p, _auto(1, 4))
        m = len(a.thresholds)
        assert m == len(wants[1].kept) <= int(np.sum(fixed[0] != 0))
        assert np.array_equal(level != FREE, fixed[2] < m) and np.array_equal(ss[level != FREE], fixed[1][fixed[2] < m])
        assert scores[:m].tobytes() == fixed[0][:m].tobytes() and np.all(scores[m:] == 0)


# ---- many alignments from the store ----
def _rows_of(p):
    """a dense upper triangle as base-pairing rows (rowptr, col, val); every kept value is above the library's cut-off"""
    rowptr, col, val = [0], [], []
    for i in range(p.shape[0]):
        js = np.flatnonzero(p[i] > 0.011)
        col.extend(js.tolist())
        val.extend(p[i, js].tolist())
        rowptr.append(len(col))
    return np.array(rowptr, np.uint32), np.array(col, np.uint32), np.array(val, np.float32)


def _gapped(rs, lengths, width):
    mask = np.zeros((len(lengths), width), np.uint8)
    for r, n in enumerate(lengths):
        mask[r, np.sort(rs.permutation(width)[:n])] = 1
    return mask


class Batch:
    pass


@pytest.fixture(scope="module")
def batch():
    """Two families in one context: sequences 0..5 and 6..8.  Alignments of 1, 2, 3, 40 and 300 columns, two with gaps and
    several rows, and one (the weak 40 columns) whose level 1 is empty while its neighbours go on."""
    rs = np.random.RandomState(77)
    b = Batch()
    lens = [1, 2, 3, 40, 300, 64, 40, 61, 66]
    b.seqs = ["".join(rs.choice(list("ACGU"), n)) for n in lens]
    mats = [_knotted_matrix(rs, n) for n in lens]
    weak = np.zeros((40, 40), np.float32)  # one hairpin and nothing that could cross it
    for k in range(4):
        weak[5 + k, 30 - k] = 0.9
    mats[6] = weak
    b.rows = [_rows_of(m) for m in mats]
    one = lambda k: (np.array([k], np.uint32), np.ones((1, lens[k]), np.uint8))  # noqa: E731
    b.alns = [one(0), one(1), one(2), one(3), one(4), one(6), (np.array([5, 3], np.uint32), _gapped(rs, [64, 40], 70)),
              (np.array([8, 7], np.uint32), _gapped(rs, [66, 61], 72)), one(7)]
    b.weak = 5
    return b


@pytest.fixture(scope="module")
def batch_ctx(batch):
    c = capi.Context(0)
    c.set_sequences(batch.seqs)
    c.set_families([0, 6, 9])
    c.set_bp(batch.rows)
    yield c
    c.close()


@pytest.fixture(scope="module")
def batch_p(batch, batch_ctx):
    """the matrix the single call averages, per alignment"""
    return [batch_ctx.consensus_structure(seq, mask, 0.5, want_p=True)[2] for seq, mask in batch.alns]


@pytest.fixture(scope="module")
def batch_want(batch_p, oracle):
    return {C: [ref.decode(oracle, p, ref.candidates(LISTS[C]), 4) for p in batch_p] for C in (2, 6)}


def _launches(c, fn):
    c.stage_timing(True)
    try:
        c.stage_report()
        out = fn()
        rep = c.stage_report()
    finally:
        c.stage_timing(False)
    return out, {k: v[2] for k, v in rep.items()}


def test_mixed_batch_against_the_restatement(batch, batch_ctx, batch_want):
    for C in (2, 6):
        want = batch_want[C]
        for K in (1, 2, 3, 4):
            got, launches = _launches(batch_ctx, lambda: batch_ctx.consensus_structures(batch.alns, _auto(C, K)))
            assert len(got) == len(batch.alns)
            for k, g in enumerate(got):
                assert ref.same(g, _first(want[k], K)), (C, K, k)
            # level k is launched when some alignment kept level k - 1
            going = 1 + sum(1 for k in range(1, K) if any(w.chosen[k - 1] != NONE for w in want))
            assert launches.get("k_pea_pick", 0) == going == launches.get("k_levels_merge", 0)
            assert launches.get("k_pea_total", 0) == 2  # the alignments up to 256 columns, and the one of 300
            # one decode per (level, size class with an alignment still going, candidate): the 300 columns are a class of their own
            classes = sum(len({m.shape[1] > 256 for (_, m), w in zip(batch.alns, want) if k == 0 or w.chosen[k - 1] != NONE})
                          for k in range(going))
            assert launches.get("k_nussinov_batch", 0) == C * classes
    want = batch_want[6]
    assert want[batch.weak].chosen[0] != NONE and want[batch.weak].chosen[1] == NONE and want[batch.weak].launched == 2  # empty at level 1 ...
    assert sum(1 for w in want if w.chosen[1] != NONE) >= 3                                                              # ... while others go on
    assert all(w.chosen == [NONE] * 4 and w.launched == 1 for w in want[:3])                                             # 1, 2 and 3 columns: no pair
    assert got[batch.weak][0][1:].tolist() == [0.0, 0.0, 0.0] and got[batch.weak][3].cand_pairs[2:].tolist() == [[0] * 6] * 2


def test_sum_p_is_the_numpy_sum(batch, batch_ctx, batch_p):
    got = batch_ctx.consensus_structures(batch.alns, _auto(6, 1))
    widths = [p.shape[0] for p in batch_p]
    assert 40 in widths and 300 in widths and 61 in widths and 70 in widths  # multiples of four (float4 rows) and others
    for p, g in zip(batch_p, got):
        assert g[3].sum_p == int(np.triu(ref.q(p), 1).sum(dtype=np.uint64))
    assert got[0][3].sum_p == 0 and all(g[3].sum_p > 0 for p, g in zip(batch_p, got) if p.shape[0] >= 40)  # one column: no cell


def test_store_anchor_to_the_fixed_calls(batch, batch_ctx):
    for C, K in ((6, 4), (2, 3)):
        got = batch_ctx.consensus_structures(batch.alns, _auto(C, K))
        for aln, (scores, ss, level, a) in zip(batch.alns, got):
            m = len(a.thresholds)
            if m:
                (fs, fss, flevel), = batch_ctx.consensus_structures([aln], a.thresholds)
                assert fss.tobytes() == ss.tobytes() and flevel.tobytes() == level.tobytes() and fs.tobytes() == scores[:m].tobytes()
            else:
                assert np.all(ss == NONE) and np.all(level == FREE)
            assert np.all(scores[m:] == 0)
    got = batch_ctx.consensus_structures(batch.alns, _auto(6, 1))
    for aln, (scores, ss, level, a) in zip(batch.alns, got):
        if len(a.thresholds):
            (s, pss), = batch_ctx.consensus_structures([aln], float(a.thresholds[0]))
            assert pss.tobytes() == ss.tobytes() and np.float32(s).tobytes() == scores[0].tobytes()


def _same_results(got, want):
    for g, w in zip(got, want):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g[:3], w[:3]))
        for name in ("chosen", "tp", "npairs", "cand_tp", "cand_pairs"):
            assert getattr(g[3], name).tobytes() == getattr(w[3], name).tobytes()
        assert g[3].sum_p == w[3].sum_p and g[3].f == w[3].f


def test_chunks_do_not_change_results(batch, batch_ctx, monkeypatch):
    want = batch_ctx.consensus_structures(batch.alns, _auto(6, 3))
    monkeypatch.setenv("DAFS_HIP_CS_BATCH_BYTES", "1")  # every alignment in a chunk of its own
    got, launches = _launches(batch_ctx, lambda: batch_ctx.consensus_structures(batch.alns, _auto(6, 3)))
    assert launches["k_pea_total"] == sum(1 for _, m in batch.alns if m.shape[1] >= 2)  # one column has no cell
    assert launches["k_pea_pick"] >= len(batch.alns)
    _same_results(got, want)
    for _, m in batch.alns:
        sizes = [int(capi._structure_auto_bytes(m.shape[0], m.shape[1], C)) for C in (1, 6, 16)]
        assert int(capi._structure_levels_bytes(m.shape[0], m.shape[1])) < sizes[0] < sizes[1] < sizes[2]
    assert batch_ctx.consensus_structures([], _auto(6, 3)) == []


def _raw_call(c, alns, nlevels, cand, outs):
    n_rows = np.array([m.shape[0] for _, m in alns], np.uint32)
    lens = np.array([m.shape[1] for _, m in alns], np.uint32)
    seq = np.ascontiguousarray(np.concatenate([s for s, _ in alns]), np.uint32)
    mask = np.ascontiguousarray(np.concatenate([m.reshape(-1) for _, m in alns]), np.uint8)
    th = np.array(list(cand) + [0.01] * 20, np.float32)
    return capi._consensus_structures_auto(c._h, len(alns), n_rows.ctypes.data, lens.ctypes.data, seq.ctypes.data, mask.ctypes.data,
                                           nlevels, len(cand), th.ctypes.data, *[o.ctypes.data for o in outs])


def test_refusals_leave_the_outputs_and_the_context_alone(batch, batch_ctx):
    good = [batch.alns[3], batch.alns[6]]
    want = batch_ctx.consensus_structures(good, _auto(6, 2))
    total = sum(m.shape[1] for _, m in good)
    bad_mask = batch.alns[6][1].copy()
    bad_mask[1, np.flatnonzero(bad_mask[1])[0]] = 0  # one residue of the second row is not placed
    ok = (0.5, 0.25, 0.125)
    calls = [(good, 0, ok), (good, 5, ok), (good, 2, ()), (good, 2, [0.9 - 0.05 * k for k in range(17)]), (good, 2, (0.25, 0.5)),
             (good, 2, (0.5, 0.5)), (good, 2, (0.5, 0.0)), (good, 2, (1.0, 0.5)), (good, 2, (0.5, -0.25)), (good, 2, (float("nan"),)),
             ([good[0], (batch.alns[6][0], bad_mask)], 2, ok)]
    for alns, nlevels, cand in calls:
        outs = [np.full(total, 0xABCDEF01, np.uint32), np.full(total, 0x5A, np.uint8), np.full(2 * 8, -7.5, np.float32),
                np.full(2 * 8, 77, np.uint32), np.full(2, 78, np.uint64), np.full(2 * 8, 79, np.uint64), np.full(2 * 8, 80, np.uint32),
                np.full(2 * 8 * 20, 81, np.uint64), np.full(2 * 8 * 20, 82, np.uint32)]
        assert _raw_call(batch_ctx, alns, nlevels, cand, outs) == -1  # DAFS_HIP_EINVAL
        for o, fill in zip(outs, (0xABCDEF01, 0x5A, -7.5, 77, 78, 79, 80, 81, 82)):
            assert np.all(o == fill)
        _same_results(batch_ctx.consensus_structures(good, _auto(6, 2)), want)
    p = ref.hand_cases()[4].p
    for nlevels, cand in ((0, ok), (5, ok), (2, ()), (2, (0.25, 0.5)), (2, (0.5, 0.0)), (2, (1.0,))):
        c = np.array(list(cand) + [0.01], np.float32)
        ss = np.full(12, 0xABCDEF01, np.uint32)
        assert capi._nussinov_decode_auto(batch_ctx._h, nlevels, len(cand), c.ctypes.data, 12, p.ctypes.data, ss.ctypes.data, *[None] * 8) == -1
        assert np.all(ss == 0xABCDEF01)
    assert capi.make_brackets_levels(*batch_ctx.nussinov_auto(p, capi.AutoThresholds(levels=2))[1:3]) == "((.[[))...]]"


def test_optional_outputs_may_be_absent(batch, batch_ctx):
    """every output after ss may be NULL"""
    good = [batch.alns[3], batch.alns[6]]
    want = batch_ctx.consensus_structures(good, _auto(6, 2))
    total = sum(m.shape[1] for _, m in good)
    ss = np.zeros(total, np.uint32)
    n_rows = np.array([m.shape[0] for _, m in good], np.uint32)
    lens = np.array([m.shape[1] for _, m in good], np.uint32)
    seq = np.ascontiguousarray(np.concatenate([s for s, _ in good]), np.uint32)
    mask = np.ascontiguousarray(np.concatenate([m.reshape(-1) for _, m in good]), np.uint8)
    cand = ref.candidates()
    assert capi._consensus_structures_auto(batch_ctx._h, 2, n_rows.ctypes.data, lens.ctypes.data, seq.ctypes.data, mask.ctypes.data, 2, 6,
                                           cand.ctypes.data, ss.ctypes.data, *[None] * 8) == 0
    assert ss.tobytes() == np.concatenate([w[1] for w in want]).tobytes()


# ---- the drivers ----
AUTO1, AUTO2 = capi.AutoThresholds(), capi.AutoThresholds(levels=2)


def _same_choice(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in ("chosen", "tp", "npairs", "cand_tp", "cand_pairs", "thresholds")) \
        and a.sum_p == b.sum_p and a.f == b.f


def _ss_cons_only(a, b):
    """the two outputs differ in the line after >SS_cons and nowhere else"""
    la, lb = a.split("\n"), b.split("\n")
    at = la.index(">SS_cons") + 1
    return len(la) == len(lb) and la[:at] == lb[:at] and la[at + 1:] == lb[at + 1:]


def test_run_on_the_srp_family(oracle):
    recs = oracle.fasta(os.path.join(GOLDEN, "RF00017_4.fa"))
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    c = capi.Context(0)
    try:
        plain = pipeline.run(names, seqs, ctx=c, reliability=True)
        got = pipeline.run(names, seqs, ctx=c, reliability=True, decoder="Levels", th_s1=AUTO2)
        sidx, mask = got.root
        _, _, p = c.consensus_structure(sidx, mask, 0.5, want_p=True)
        want = ref.decode(oracle, p, AUTO2.candidates, 2)
        assert ref.same((got.ss_scores, got.ss, got.ss_level, got.ss_auto), want)
        assert got.ss_str == capi.make_brackets_levels(want.ss, want.level) and "(" in got.ss_str
        assert got.ss_auto.f == want.f > 0 and list(got.ss_auto.gammas) == [ref.GAMMAS[k] for k in want.kept]
        assert _ss_cons_only(got.output, plain.output)
        sto = [ln for ln in got.stockholm.split("\n") if ln.startswith("#=GC SS_cons")]
        assert len(sto) == 1 and sto[0].split()[-1] == got.ss_str
        # the anchor: the run at the chosen thresholds prints the same bytes
        fixed = pipeline.run(names, seqs, ctx=c, reliability=True, decoder="Levels", th_s1=tuple(got.ss_auto.thresholds))
        assert fixed.output == got.output and fixed.stockholm == got.stockholm and fixed.ss_level.tobytes() == got.ss_level.tobytes()
        # one level under the default decoder: the plain structure at the chosen threshold
        one = pipeline.run(names, seqs, ctx=c, reliability=True, th_s1=AUTO1)
        want1 = ref.decode(oracle, p, AUTO1.candidates, 1)
        assert ref.same((one.ss_scores, one.ss, one.ss_level, one.ss_auto), want1)
        at = pipeline.run(names, seqs, ctx=c, reliability=True, th_s1=float(one.ss_auto.thresholds[0]))
        assert at.output == one.output and at.stockholm == one.stockholm and at.ss.tobytes() == one.ss.tobytes()
        assert not hasattr(plain, "ss_auto") and not hasattr(fixed, "ss_auto")
    finally:
        c.close()


def test_refused_options():
    for kw in (dict(th_s1=AUTO1, bp_update1=True), dict(th_s1=AUTO2), dict(decoder="Levels", th_s1=AUTO2, bp_update1=True),
               dict(th_s=AUTO1), dict(decoder="Levels", th_s=AUTO1, th_s1=AUTO1), dict(decoder="IPknot", th_s1=AUTO1)):
        with pytest.raises(ValueError):
            pipeline.run(["a"], ["ACGU"], **kw)
        with pytest.raises(ValueError):
            pipeline.run_batch([(["a"], ["ACGU"])], **kw)
        with pytest.raises(ValueError):
            pipeline.pairwise(["a", "b"], ["ACGU", "ACGU"], **kw)
    with pytest.raises(ValueError):
        pipeline.add(["s"], ["ACGU"], ["a"], ["ACGU"], th_s1=AUTO1, seed_ss=np.full(4, NONE, np.uint32))
    with pytest.raises(ValueError):
        pipeline.fold_each(["a"], ["ACGU"], th=AUTO2)  # two levels need decoder "Levels"


def test_run_batch_and_pairwise_equal_single_runs():
    recs = synth.family_set(3, 60, seed=431)
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    kw = dict(decoder="Levels", th_s1=AUTO2)
    c = capi.Context(0)
    try:
        want = pipeline.run(names, seqs, ctx=c, row_structures=True, reliability=True, **kw)
        assert len(want.row_ss_auto) == 3 and len(want.row_ss_str) == 3
        assert want.row_ss_str == [stockholm.row_ss_str(row, x, lv) for row, x, lv in zip(want.rows, want.row_ss, want.row_ss_level)]
        # every row chooses its own thresholds: each is the dense call on that sequence's own rows of the store
        own = c.consensus_structures([(np.array([k], np.uint32), np.ones((1, len(s)), np.uint8)) for k, s in enumerate(seqs)], AUTO2)
        for (scores, ss, level, a), x, lv, ra in zip(own, want.row_ss, want.row_ss_level, want.row_ss_auto):
            assert ss.tobytes() == x.tobytes() and level.tobytes() == lv.tobytes() and _same_choice(a, ra)
        got = pipeline.run_batch([(names, seqs), (names[:2], seqs[:2])], ctx=c, row_structures=True, reliability=True, **kw)
        assert got[0].output == want.output and got[0].stockholm == want.stockholm and got[0].ss_level.tobytes() == want.ss_level.tobytes()
        assert got[0].ss_scores.tobytes() == want.ss_scores.tobytes() and got[0].row_ss_str == want.row_ss_str
        assert _same_choice(got[0].ss_auto, want.ss_auto)
        pw = pipeline.pairwise(names, seqs, ctx=c, **kw)
        for (x, y), g in zip(pw.pairs, pw.results):
            single = pipeline.run([names[x], names[y]], [seqs[x], seqs[y]], ctx=c, **kw)
            assert g.output == single.output and g.ss_level.tobytes() == single.ss_level.tobytes() and _same_choice(g.ss_auto, single.ss_auto)
        assert got[1].output == pw.results[0].output
    finally:
        c.close()


def test_fold_each_add_and_cluster(oracle):
    c = capi.Context(0)
    try:
        recs = [synth.random_set(1, length, seed=970 + k, jitter=0.0)[0] for k, length in enumerate([45, 80])]
        names, seqs = ["f0", "f1"], [s for _, s in recs]
        got = pipeline.fold_each(names, seqs, th=AUTO2, ctx=c, decoder="Levels")
        for g, (rowptr, col, val) in zip(got, c.bp(0)):  # the un-relaxed rows fold_each decoded
            p = np.zeros((len(rowptr) - 1,) * 2, np.float32)
            for i in range(len(rowptr) - 1):
                p[i, col[rowptr[i]:rowptr[i + 1]]] = val[rowptr[i]:rowptr[i + 1]]
            want = ref.decode(oracle, p, AUTO2.candidates, 2)
            assert ref.same((g.score, g.ss, g.ss_level, g.ss_auto), want) and g.ss_str == capi.make_brackets_levels(want.ss, want.level)
        one = pipeline.fold_each(names, seqs, th=AUTO1, ctx=c)
        assert all(o.ss_auto.chosen.tolist() == g.ss_auto.chosen[:1].tolist() for o, g in zip(one, got))
        recs = synth.family_set(4, 60, seed=77)
        names, seqs = [n for n, _ in recs], [s for _, s in recs]
        seed = pipeline.run(names[:3], seqs[:3], ctx=c)
        snames, srows = names[:3], seed.rows
        added = pipeline.add(snames, srows, names[3:], seqs[3:], ctx=c, reliability=True, row_structures=True, decoder="Levels", th_s1=AUTO2)
        fixed = pipeline.add(snames, srows, names[3:], seqs[3:], ctx=c, reliability=True, decoder="Levels",
                             th_s1=tuple(added.ss_auto.thresholds) or (0.5,))
        assert len(added.ss_auto.thresholds) >= 1 and fixed.ss.tobytes() == added.ss.tobytes() and fixed.ss_level.tobytes() == added.ss_level.tobytes()
        assert len(added.row_ss_auto) == 4
        each = pipeline.add_each(snames, srows, names[3:], seqs[3:], ctx=c, decoder="Levels", th_s1=AUTO2)
        assert each.results[0].ss_auto.sum_p > 0 and each.results[0].ss_str == capi.make_brackets_levels(each.results[0].ss, each.results[0].ss_level)
        recs = synth.family_set(3, 50, seed=5) + synth.family_set(3, 50, seed=6)
        names, seqs = ["s%d" % k for k in range(6)], [s for _, s in recs]
        cl = pipeline.cluster(names, seqs, threshold=0.5, ctx=c, decoder="Levels", th_s1=AUTO2)
        for members, r in zip(cl.clusters, cl.results):
            single = pipeline.run([names[i] for i in members], [seqs[i] for i in members], ctx=c, decoder="Levels", th_s1=AUTO2)
            assert r.output == single.output and r.ss_level.tobytes() == single.ss_level.tobytes() and _same_choice(r.ss_auto, single.ss_auto)
    finally:
        c.close()


# ---- the command line ----
DAFS = os.path.join(os.path.dirname(os.path.dirname(GOLDEN)), "dafs_amd", "dafs")
SRP = os.path.join(GOLDEN, "RF00017_4.fa")


def _cli(*args, ok=True):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr
    return r.stdout if ok else r.stderr


def _split_auto(sto):
    """a Stockholm file without its "#=GF CC SS_cons auto" lines, and those lines"""
    lines = sto.split("\n")
    mine = [ln for ln in lines if ln.startswith("#=GF CC SS_cons auto ")]
    return "\n".join(ln for ln in lines if not ln.startswith("#=GF CC SS_cons auto ")), mine


def _auto_line(a):
    ths = ",".join("%g" % float(t) for t in a.thresholds) or "none"
    return "#=GF CC SS_cons auto thresholds %s f %.6f" % (ths, a.f)


def _check_table(text, results, auto):
    """--fold-auto-table against the drivers' .ss_auto: per alignment the header and one line per decoded (level, candidate)"""
    blocks = []
    for ln in text.split("\n"):
        if ln.startswith("# alignment "):
            blocks.append((ln.split(), []))
        elif ln and not ln.startswith("==> "):
            blocks[-1][1].append(ln.split("\t"))
    assert len(blocks) == len(results)
    C = len(auto.candidates)
    for (head, rows), res in zip(blocks, results):
        a = res.ss_auto
        assert head[3] == "columns" and int(head[4]) == len(res.ss) and head[5] == "sum_p" and int(head[6]) == a.sum_p
        assert head[2] == stockholm.names(res.row_names if hasattr(res, "row_names") else [head[2]])[0]
        launched = 1 + sum(1 for k in range(auto.levels - 1) if all(c != NONE for c in a.chosen[:k + 1]))
        assert len(rows) == launched * C
        t_low = n_low = 0
        for k in range(launched):
            for c in range(C):
                level, gamma, th, pairs, tp, f, chosen = rows[k * C + c]
                assert (int(level), float(gamma), int(pairs), int(tp)) == (k, auto.gammas[c], int(a.cand_pairs[k][c]), int(a.cand_tp[k][c]))
                assert th == "%g" % float(auto.candidates[c]) and int(chosen) == (1 if a.chosen[k] == c else 0)
                assert f == "%.6f" % capi.pseudo_f(t_low + int(tp), n_low + int(pairs), a.sum_p)
            t_low, n_low = t_low + int(a.tp[k]), n_low + int(a.npairs[k])


@pytest.fixture(scope="module")
def srp(oracle):
    recs = oracle.fasta(SRP)
    return [n for n, _ in recs], [s for _, s in recs]


CLI_CASES = {"G-auto": (("-G", "auto"), dict(th_s1=AUTO1)), "T-auto": (("-T", "auto"), dict(th_s1=AUTO1)),
             "levels-auto-auto": (("--fold-decoder", "Levels", "-G", "auto,auto"), dict(decoder="Levels", th_s1=AUTO2)),
             "auto-gammas": (("--fold-decoder", "Levels", "-G", "auto", "--auto-gammas", "2,8"),
                             dict(decoder="Levels", th_s1=capi.AutoThresholds((2, 8))))}


@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_cli_prints_what_the_python_driver_returns(case, srp, tmp_path):
    names, seqs = srp
    args, kw = CLI_CASES[case]
    sto, tab = tmp_path / "out.sto", tmp_path / "auto.tsv"
    want = pipeline.run(names, seqs, reliability=True, **kw)
    assert _cli(*args, "--stockholm", sto, "--fold-auto-table", tab, SRP) == want.output and "(" in want.ss_str
    block, lines = _split_auto(sto.read_text())
    assert block == want.stockholm and lines == [_auto_line(want.ss_auto)]
    assert sto.read_text().split("\n")[2] == lines[0]  # behind the tree line
    _check_table(tab.read_text(), [want], kw["th_s1"])


@pytest.mark.parametrize("args, kw", [(("-G", "2,4"), dict(th_s1=1.0 / 3.0)),
                                      (("--fold-decoder", "Levels", "-G", "2,4"), dict(decoder="Levels", th_s1=(1.0 / 3.0, 1.0 / 5.0)))],
                         ids=["nussinov", "levels"])
def test_cli_without_auto_prints_the_fixed_thresholds_bytes(args, kw, srp, tmp_path):
    """nothing moved: the driver's bytes at the fixed thresholds, and no auto line"""
    names, seqs = srp
    sto = tmp_path / "out.sto"
    want = pipeline.run(names, seqs, reliability=True, **kw)
    assert _cli(*args, "--stockholm", sto, SRP) == want.output and sto.read_text() == want.stockholm and " auto " not in want.stockholm


def test_cli_refusals(tmp_path):
    assert "cannot be mixed with numbers" in _cli("-G", "auto,2", SRP, ok=False)
    assert "cannot be mixed with numbers" in _cli("--fold-decoder", "Levels", "-T", "0.2,auto", SRP, ok=False)
    assert "one to four levels" in _cli("--fold-decoder", "Levels", "-G", "auto,auto,auto,auto,auto", SRP, ok=False)
    assert "needs --fold-decoder Levels" in _cli("-G", "auto,auto", SRP, ok=False)
    assert "inside the dual-decomposition loop" in _cli("-t", "auto", SRP, ok=False)
    assert "inside the dual-decomposition loop" in _cli("-g", "auto", SRP, ok=False)
    assert "--bp-update1" in _cli("-G", "auto", "--bp-update1", SRP, ok=False)
    seed = tmp_path / "seed.fa"
    seed.write_text(">SS_cons\n(..)\n> s\nACGU\n")
    assert "cannot be combined with --seed-structure" in _cli("-G", "auto", "--seed", seed, "--seed-structure", SRP, ok=False)
    assert "need -T auto or -G auto" in _cli("--auto-gammas", "1,2", SRP, ok=False)
    assert "need -T auto or -G auto" in _cli("--fold-auto-table", tmp_path / "t.tsv", SRP, ok=False)
    for bad in ("2,1", "1,1", "0,1", "-1,2", "1,x", "1,,2"):
        assert "strictly increasing" in _cli("-G", "auto", "--auto-gammas", bad, SRP, ok=False)
    assert "one to sixteen" in _cli("-G", "auto", "--auto-gammas", ",".join(str(k) for k in range(1, 18)), SRP, ok=False)


def test_cli_modes_with_auto(tmp_path):
    """several files, --pairwise, --seed, --seed-each, --row-structures, --covariation, --compare: the Python drivers' bytes"""
    recs = synth.family_set(4, 60, seed=77)
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    fa, fb, sto, tab = tmp_path / "fam.fa", tmp_path / "three.fa", tmp_path / "out.sto", tmp_path / "auto.tsv"
    fa.write_text(synth.to_fasta(recs))
    fb.write_text(synth.to_fasta(recs[:3]))
    lv = ("--fold-decoder", "Levels", "-G", "auto,auto", "--fold-auto-table", tab)
    kw = dict(decoder="Levels", th_s1=AUTO2)
    want = pipeline.run(names, seqs, reliability=True, row_structures=True, covariation=True, identity=True, **kw)
    assert _cli(*lv, "--stockholm", sto, "--row-structures", "--covariation", tmp_path / "cov.txt", "--identity", tmp_path / "id.txt", fa) == want.output
    block, lines = _split_auto(sto.read_text())
    assert block == want.stockholm and lines == [_auto_line(want.ss_auto)]
    _check_table(tab.read_text(), [want], AUTO2)
    both = pipeline.run_batch([(names, seqs), (names[:3], seqs[:3])], identity=True, **kw)
    out = _cli(*lv, fa, fb)
    assert all(r.output in out for r in both)
    _check_table(tab.read_text(), both, AUTO2)
    pw = pipeline.pairwise(names, seqs, reliability=True, row_structures=True, **kw)
    out = _cli(*lv, "--pairwise", "--stockholm", sto, "--row-structures", fa)
    assert out == "".join("==> %d %d <==\n" % (x + 1, y + 1) + r.output for (x, y), r in zip(pw.pairs, pw.results))
    block, lines = _split_auto(sto.read_text())
    assert block == "".join(r.stockholm for r in pw.results) and lines == [_auto_line(r.ss_auto) for r in pw.results]
    seed = pipeline.run(names[:3], seqs[:3])
    seed_fa, new_fa = tmp_path / "seed.fa", tmp_path / "new.fa"
    seed_fa.write_text(seed.output)
    new_fa.write_text(synth.to_fasta(recs[3:]))
    snames, srows = stockholm.read_seed(str(seed_fa))
    added = pipeline.add(snames, srows, names[3:], seqs[3:], reliability=True, row_structures=True, **kw)
    assert _cli(*lv, "--seed", seed_fa, "--stockholm", sto, "--row-structures", new_fa) == added.output
    block, lines = _split_auto(sto.read_text())
    assert block == added.stockholm and lines == [_auto_line(added.ss_auto)]
    each = pipeline.add_each(snames, srows, names[3:], seqs[3:], **kw)
    assert each.results[0].output in _cli(*lv, "--seed", seed_fa, "--seed-each", new_fa)
    ref_fa, cmp_out = tmp_path / "ref.fa", tmp_path / "cmp.txt"
    plain = pipeline.run(names, seqs)
    ref_fa.write_text(plain.output.split("\n", 1)[1])  # without the tree line
    reference = stockholm.read_seed_structure(str(ref_fa))
    cmp = pipeline.run(names, seqs, compare=reference, **kw).compare
    _cli(*lv, "--compare", cmp_out, "--compare-ref", ref_fa, fa)
    assert cmp_out.read_text() == cmp.table
