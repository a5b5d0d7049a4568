"""GPU tests of the level-by-level decode: dafs_hip_nussinov_decode_levels and
dafs_hip_consensus_structures_levels against the numpy restatement of tests/levels_ref.py, bit for bit; the refusals; the
drivers and the command line with decoder "Levels"."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import levels_ref as ref
from dafs_amd import capi, pipeline, stockholm, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
GOLDEN = os.path.join(ROOT, "tests", "golden")
NONE, FREE = ref.NONE, ref.FREE
THS = (0.2, 0.15, 0.1, 0.05)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _same(got, want):
    """(scores, ss, level) of the library against the restatement's (scores, merged, level, ...)"""
    return (np.asarray(got[0], np.float32).tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
            and got[2].tobytes() == want[2].tobytes())


@pytest.mark.parametrize("case", ref.hand_cases(), ids=lambda c: c.name)
def test_hand_made_cases(case, ctx, oracle):
    scores, ss, level = ctx.nussinov_levels(case.p, case.ths)
    assert ss.tolist() == case.ss.tolist() and level.tolist() == case.level.tolist()
    assert _same((scores, ss, level), ref.decode(oracle, case.p, case.ths))
    assert capi.make_brackets_levels(ss, level) == case.text


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
    """per width one matrix and its restatement at four levels (the first K levels are the restatement at K): built once"""
    rs = np.random.RandomState(2525)
    out = {}
    for L in (3, 4, 5, 17, 64, 65, 257, 300):
        p = _knotted_matrix(rs, L)
        out[L] = (p, ref.decode(oracle, p, THS))
    return out


def _first(want, K):
    """the restatement at K levels from the one at four: lower levels do not depend on higher ones"""
    scores, merged, level, per_level = want
    merged, level = merged.copy(), level.copy()
    merged[level >= K] = NONE  # FREE included: those are NONE already
    level[level >= K] = FREE
    return scores[:K].copy(), merged, level


@pytest.mark.parametrize("L", [3, 4, 5, 17, 64, 65, 257, 300])
def test_random_matrices(L, ctx, random_cases, oracle):
    p, want = random_cases[L]
    for K in (1, 2, 3, 4):
        got = ctx.nussinov_levels(p, THS[:K])
        assert _same(got, _first(want, K)), (L, K)
    s1, ss1 = ctx.nussinov(p, None, THS[0])  # K = 1 is the plain decode
    got = ctx.nussinov_levels(p, THS[:1])
    assert got[1].tobytes() == ss1.tobytes() and got[0][0].tobytes() == np.float32(s1).tobytes()
    if L >= 64:
        assert int(np.sum(want[2] == 1)) > 0 and int(np.sum(want[2] == 0)) > 0  # crossing pairs were found


def test_global_table_form_gives_the_same_bits(ctx, random_cases, monkeypatch):
    p, want = random_cases[65]
    monkeypatch.setenv("DAFS_HIP_NUSS_GLOBAL", "1")
    assert _same(ctx.nussinov_levels(p, THS[:3]), _first(want, 3))


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
def batch(oracle):
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
    one = lambda k: (np.array([k], np.uint32), np.ones((1, lens[k]), np.uint8))
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
def batch_want(batch, batch_ctx, oracle):
    """the restatement on the matrix the single call averages, per alignment"""
    out = []
    for seq, mask in batch.alns:
        _, _, p = batch_ctx.consensus_structure(seq, mask, THS[0], want_p=True)
        out.append(ref.decode(oracle, p, THS))
    return out


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
    for K in (2, 3, 4):
        got, launches = _launches(batch_ctx, lambda: batch_ctx.consensus_structures(batch.alns, THS[:K]))
        assert len(got) == len(batch.alns)
        for k, g in enumerate(got):
            assert _same(g, _first(batch_want[k], K)), (K, k)
        going = 1 + sum(1 for k in range(1, K) if any(ref.pairs_of(w[3][k - 1]) for w in batch_want))  # levels with a launch
        assert launches.get("k_levels_merge", 0) == going and launches.get("k_levels_mask", 0) >= going - 1
    want = batch_want
    assert not ref.pairs_of(want[batch.weak][3][1]) and ref.pairs_of(want[batch.weak][3][0])  # empty at level 1 ...
    assert sum(1 for w in want if ref.pairs_of(w[3][1])) >= 4                                  # ... while others go on
    assert all(np.all(w[2] == FREE) for w in want[:3])                                          # 1, 2 and 3 columns: no pair
    assert got[batch.weak][0][1:].tolist() == [0.0, 0.0, 0.0]


def test_one_level_is_the_plain_call(batch, batch_ctx):
    plain = batch_ctx.consensus_structures(batch.alns, THS[0])
    got = batch_ctx.consensus_structures(batch.alns, THS[:1])
    for (s, ss), (scores, gss, level) in zip(plain, got):
        assert gss.tobytes() == ss.tobytes() and scores.tobytes() == np.float32(s).tobytes()
        assert np.array_equal(level != FREE, np.isin(np.arange(len(ss)), [c for pr in ref.pairs_of(ss) for c in pr]))


def test_chunks_do_not_change_results(batch, batch_ctx, monkeypatch):
    want = batch_ctx.consensus_structures(batch.alns, THS[:3])
    monkeypatch.setenv("DAFS_HIP_CS_BATCH_BYTES", "1")  # every alignment in a chunk of its own
    got, launches = _launches(batch_ctx, lambda: batch_ctx.consensus_structures(batch.alns, THS[:3]))
    assert launches["k_levels_merge"] >= len(batch.alns)
    for g, w in zip(got, want):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(g, w))
    assert all(int(capi._structure_levels_bytes(m.shape[0], m.shape[1])) > int(capi._structure_bytes(m.shape[0], m.shape[1]))
               for _, m in batch.alns)


def _raw_call(c, alns, ths, ss, level, score):
    n_rows = np.array([m.shape[0] for _, m in alns], np.uint32)
    lens = np.array([m.shape[1] for _, m in alns], np.uint32)
    seq = np.ascontiguousarray(np.concatenate([s for s, _ in alns]), np.uint32)
    mask = np.ascontiguousarray(np.concatenate([m.reshape(-1) for _, m in alns]), np.uint8)
    th = np.array(list(ths) + [0.1] * 6, np.float32)
    return capi._consensus_structures_levels(c._h, len(alns), n_rows.ctypes.data, lens.ctypes.data, seq.ctypes.data, mask.ctypes.data,
                                             len(ths), th.ctypes.data, ss.ctypes.data, level.ctypes.data, score.ctypes.data)


def test_refusals_leave_the_outputs_and_the_context_alone(batch, batch_ctx):
    good = [batch.alns[3], batch.alns[6]]
    want = batch_ctx.consensus_structures(good, THS[:2])
    total = sum(m.shape[1] for _, m in good)
    bad_mask = batch.alns[6][1].copy()
    bad_mask[1, np.flatnonzero(bad_mask[1])[0]] = 0  # one residue of the second row is not placed
    calls = [(good, ()), (good, (0.2, 0.1, 0.1, 0.1, 0.1)), (good, (0.2, 0.0)), (good, (0.2, 0.1, -0.5)),
             ([good[0], (batch.alns[6][0], bad_mask)], (0.2, 0.1))]
    for alns, ths in calls:
        ss = np.full(total, 0xABCDEF01, np.uint32)
        level = np.full(total, 0x5A, np.uint8)
        score = np.full(2 * 8, -7.5, np.float32)
        assert _raw_call(batch_ctx, alns, ths, ss, level, score) == -1  # DAFS_HIP_EINVAL
        assert np.all(ss == 0xABCDEF01) and np.all(level == 0x5A) and np.all(score == -7.5)
        again = batch_ctx.consensus_structures(good, THS[:2])
        assert all(a.tobytes() == b.tobytes() for g, w in zip(again, want) for a, b in zip(g, w))
    p = ref.hand_cases()[2].p
    for ths in ((), (0.2,) * 5, (0.2, 0.0)):
        with pytest.raises(capi.DafsHipError):
            batch_ctx.nussinov_levels(p, ths)
    assert batch_ctx.nussinov_levels(p, (0.2, 0.2))[1].tolist() == ref.hand_cases()[2].ss.tolist()


def test_new_abi_symbols():
    lib = C.CDLL(os.path.join(ROOT, "dafs_amd", "libdafs_hip.so"))
    for name in ("dafs_hip_consensus_structures_levels", "dafs_hip_nussinov_decode_levels", "dafs_hip_make_brackets_levels",
                 "dafs_host_structure_levels_bytes"):
        assert hasattr(lib, name), name


# ---- the drivers ----
LEVELS = (1.0 / 3.0, 1.0 / 5.0)  # -G 2,4


def _ss_cons_only(a, b):
    """the two outputs differ in the line after >SS_cons and nowhere else"""
    la, lb = a.split("\n"), b.split("\n")
    at = la.index(">SS_cons") + 1
    return len(la) == len(lb) and la[:at] == lb[:at] and la[at + 1:] == lb[at + 1:]


@pytest.fixture(scope="module")
def srp(oracle):
    recs = oracle.fasta(os.path.join(GOLDEN, "RF00017_4.fa"))
    return [n for n, _ in recs], [s for _, s in recs]


def test_run_on_the_srp_family(srp, oracle):
    names, seqs = srp
    c = capi.Context(0)
    try:
        plain = pipeline.run(names, seqs, ctx=c, reliability=True)
        got = pipeline.run(names, seqs, ctx=c, reliability=True, decoder="Levels", th_s1=LEVELS)
        sidx, mask = got.root
        _, _, p = c.consensus_structure(sidx, mask, LEVELS[0], want_p=True)
        want = ref.decode(oracle, p, LEVELS)
        assert _same((got.ss_scores, got.ss, got.ss_level), want)
        assert got.ss_str == ref.brackets(want[1], want[2]) and "(" in got.ss_str
        assert _ss_cons_only(got.output, plain.output)
        sto = [ln for ln in got.stockholm.split("\n") if ln.startswith("#=GC SS_cons")]
        assert len(sto) == 1 and sto[0].split()[-1] == got.ss_str
        one = pipeline.run(names, seqs, ctx=c, reliability=True, decoder="Levels")  # one level: today's bytes
        assert one.output == plain.output and one.stockholm == plain.stockholm and one.ss.tobytes() == plain.ss.tobytes()
        assert not hasattr(plain, "ss_level") and np.array_equal(one.ss_level != FREE, (one.ss_level == 0))
    finally:
        c.close()


def test_refused_options():
    for kw in (dict(decoder="Levels", bp_update1=True), dict(decoder="Levels", th_s1=(0.3,) * 5), dict(decoder="Levels", th_s1=(0.3, 0.0)),
               dict(decoder="IPknot")):
        with pytest.raises(ValueError):
            pipeline.run(["a"], ["ACGU"], **kw)
        with pytest.raises(ValueError):
            pipeline.run_batch([(["a"], ["ACGU"])], **kw)
        with pytest.raises(ValueError):
            pipeline.pairwise(["a", "b"], ["ACGU", "ACGU"], **kw)
    with pytest.raises(ValueError):
        pipeline.add(["s"], ["ACGU"], ["a"], ["ACGU"], decoder="Levels", seed_ss=np.full(4, NONE, np.uint32))


def test_run_batch_and_pairwise_equal_single_runs():
    recs = synth.family_set(3, 60, seed=431)
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    c = capi.Context(0)
    try:
        want = pipeline.run(names, seqs, ctx=c, decoder="Levels", th_s1=LEVELS, row_structures=True, reliability=True)
        assert len(want.row_ss_str) == 3 and all(len(t) == len(row) for t, row in zip(want.row_ss_str, want.rows))
        assert all(len(x) == len(s) == len(lv) for x, lv, s in zip(want.row_ss, want.row_ss_level, seqs))
        assert want.row_ss_str == [stockholm.row_ss_str(row, x, lv) for row, x, lv in zip(want.rows, want.row_ss, want.row_ss_level)]
        got = pipeline.run_batch([(names, seqs), (names[:2], seqs[:2])], ctx=c, decoder="Levels", th_s1=LEVELS, row_structures=True,
                                 reliability=True)
        assert got[0].output == want.output and got[0].stockholm == want.stockholm and got[0].ss_level.tobytes() == want.ss_level.tobytes()
        assert got[0].ss_scores.tobytes() == want.ss_scores.tobytes() and got[0].row_ss_str == want.row_ss_str
        pw = pipeline.pairwise(names, seqs, ctx=c, decoder="Levels", th_s1=LEVELS)
        for (x, y), g in zip(pw.pairs, pw.results):
            single = pipeline.run([names[x], names[y]], [seqs[x], seqs[y]], ctx=c, decoder="Levels", th_s1=LEVELS)
            assert g.output == single.output and g.ss_level.tobytes() == single.ss_level.tobytes()
        assert got[1].output == pw.results[0].output
    finally:
        c.close()


def _cli(*args, ok=True):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert (r.returncode == 0) == ok, r.stderr
    return r.stdout if ok else r.stderr


def test_cli_prints_what_the_python_driver_returns(srp, tmp_path):
    names, seqs = srp
    fa = os.path.join(GOLDEN, "RF00017_4.fa")
    sto = tmp_path / "out.sto"
    want = pipeline.run(names, seqs, reliability=True, decoder="Levels", th_s1=LEVELS)
    assert _cli("--fold-decoder", "Levels", "-G", "2,4", "--stockholm", sto, fa) == want.output
    assert sto.read_text() == want.stockholm
    plain = pipeline.run(names, seqs, reliability=True, th_s1=LEVELS[0])
    assert _cli("-G", "2,4", "--stockholm", sto, fa) == plain.output  # the default decoder reads the first entry, as before
    assert sto.read_text() == plain.stockholm
    assert _cli("--fold-decoder", "Levels", "-G", "2", "--stockholm", sto, fa) == plain.output  # one level: the same bytes
    assert sto.read_text() == plain.stockholm


def test_cli_refusals(tmp_path):
    fa = os.path.join(GOLDEN, "RF00017_4.fa")
    assert "--bp-update1 is not built" in _cli("--fold-decoder", "Levels", "--bp-update1", fa, ok=False)
    seed = tmp_path / "seed.fa"
    seed.write_text(">SS_cons\n(..)\n> s\nACGU\n")
    err = _cli("--fold-decoder", "Levels", "--seed", seed, "--seed-structure", fa, ok=False)
    assert "--fold-decoder Levels cannot be combined with --seed-structure" in err
    assert "Levels" in _cli("--fold-decoder", "IPknot", fa, ok=False) and "Levels" in _cli("--ipknot", fa, ok=False)
    assert "one to four levels" in _cli("--fold-decoder", "Levels", "-G", "1,2,3,4,5", fa, ok=False)


def test_cli_modes_with_levels(tmp_path):
    """--pairwise, --seed, --seed-each, several files, --row-structures, --covariation, --compare: the Python drivers' bytes"""
    recs = synth.family_set(4, 60, seed=77)
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    fa, fb, sto = tmp_path / "fam.fa", tmp_path / "three.fa", tmp_path / "out.sto"
    fa.write_text(synth.to_fasta(recs))
    fb.write_text(synth.to_fasta(recs[:3]))
    lv = ("--fold-decoder", "Levels", "-G", "2,4")
    kw = dict(decoder="Levels", th_s1=LEVELS)
    want = pipeline.run(names, seqs, reliability=True, row_structures=True, covariation=True, **kw)
    assert _cli(*lv, "--stockholm", sto, "--row-structures", "--covariation", tmp_path / "cov.txt", fa) == want.output
    assert sto.read_text() == want.stockholm
    both = pipeline.run_batch([(names, seqs), (names[:3], seqs[:3])], **kw)
    out = _cli(*lv, fa, fb)
    assert all(r.output in out for r in both)
    pw = pipeline.pairwise(names, seqs, reliability=True, row_structures=True, **kw)
    out = _cli(*lv, "--pairwise", "--stockholm", sto, "--row-structures", fa)
    assert out == "".join("==> %d %d <==\n" % (x + 1, y + 1) + r.output for (x, y), r in zip(pw.pairs, pw.results))
    assert sto.read_text() == "".join(r.stockholm for r in pw.results)
    seed = pipeline.run(names[:3], seqs[:3])
    seed_fa, new_fa = tmp_path / "seed.fa", tmp_path / "new.fa"
    seed_fa.write_text(seed.output)
    new_fa.write_text(synth.to_fasta(recs[3:]))
    snames, srows = stockholm.read_seed(str(seed_fa))
    added = pipeline.add(snames, srows, names[3:], seqs[3:], reliability=True, row_structures=True, **kw)
    assert _cli(*lv, "--seed", seed_fa, "--stockholm", sto, "--row-structures", new_fa) == added.output
    assert sto.read_text() == added.stockholm
    each = pipeline.add_each(snames, srows, names[3:], seqs[3:], **kw)
    assert each.results[0].output in _cli(*lv, "--seed", seed_fa, "--seed-each", new_fa)
    # --compare against the plain run's output (a nested SS_cons, which the reader takes): "# structure" counts the pairs of all levels
    ref_fa, cmp_out = tmp_path / "ref.fa", tmp_path / "cmp.txt"
    plain = pipeline.run(names, seqs)
    ref_fa.write_text(plain.output.split("\n", 1)[1])  # without the tree line
    reference = stockholm.read_seed_structure(str(ref_fa))
    cmp = pipeline.run(names, seqs, compare=reference, **kw).compare
    _cli(*lv, "--compare", cmp_out, "--compare-ref", ref_fa, fa)
    assert cmp_out.read_text() == cmp.table
    line = [ln for ln in cmp.table.split("\n") if ln.startswith("# structure")][0].split()
    held = sum(1 for row in want.rows for i, j in ref.pairs_of(want.ss) if row[i] != "-" and row[j] != "-")  # per row, both residues there
    assert int(line[line.index("test") + 1]) == held > 0


def test_fold_each_and_cluster_with_levels(oracle, tmp_path):
    c = capi.Context(0)
    try:
        recs = [synth.random_set(1, length, seed=970 + k, jitter=0.0)[0] for k, length in enumerate([45, 80])]
        names, seqs = ["f0", "f1"], [s for _, s in recs]
        got = pipeline.fold_each(names, seqs, th=LEVELS, ctx=c, decoder="Levels")
        for g, (rowptr, col, val) in zip(got, c.bp(0)):  # the un-relaxed rows fold_each decoded
            p = np.zeros((len(rowptr) - 1,) * 2, np.float32)
            for i in range(len(rowptr) - 1):
                p[i, col[rowptr[i]:rowptr[i + 1]]] = val[rowptr[i]:rowptr[i + 1]]
            want = ref.decode(oracle, p, LEVELS)
            assert _same((g.score, g.ss, g.ss_level), want) and g.ss_str == ref.brackets(want[1], want[2])
        recs = synth.family_set(3, 50, seed=5) + synth.family_set(3, 50, seed=6)
        names, seqs = ["s%d" % k for k in range(6)], [s for _, s in recs]
        cl = pipeline.cluster(names, seqs, threshold=0.5, ctx=c, decoder="Levels", th_s1=LEVELS)
        for members, r in zip(cl.clusters, cl.results):
            single = pipeline.run([names[i] for i in members], [seqs[i] for i in members], ctx=c, decoder="Levels", th_s1=LEVELS)
            assert r.output == single.output and r.ss_level.tobytes() == single.ss_level.tobytes()
        fa = tmp_path / "mixed.fa"
        fa.write_text(synth.to_fasta(list(zip(names, seqs))))
        out = _cli("--fold-decoder", "Levels", "-G", "2,4", "--cluster", "0.5", fa)
        assert all(r.output.split("\n", 1)[1] in out for r in cl.results)  # without the tree line, whatever the record's header
    finally:
        c.close()
