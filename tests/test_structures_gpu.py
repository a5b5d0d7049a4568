"""GPU tests of dafs_hip_consensus_structures (many alignments decoded in one call), of the per-row structures built on it
(row_structures=True, `dafs --stockholm --row-structures`) and of pipeline.fold_each.  The yardsticks
are the CPU oracle's SparseNussinov on the dense matrix and the single-alignment call, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from dafs_amd import capi, pipeline, stockholm, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAFS = os.path.join(ROOT, "dafs_amd", "dafs")
NONE = 0xFFFFFFFF
TH = 0.15
LENS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1100, 40]  # the last one: every probability below TH
WEAK = 12


def _bp_rows(rs, length, weak=False):
    """Base-pairing rows of one sequence as set_bp takes them, (rowptr, col, val): hairpins of probability 0.95 laid end to
    end over the whole sequence, the outermost pair (0, length - 1) among them, and scattered entries of 0.02 .. 0.3; weak:
    everything in 0.02 .. 0.1.  Every value is above the library's cut-off of 0.01."""
    cells = {}
    for _ in range(3 * length):
        i = int(rs.randint(0, max(length - 1, 1)))
        j = int(rs.randint(i, length))
        if j > i:
            cells[(i, j)] = np.float32(0.02 + (0.08 if weak else 0.28) * rs.rand())
    if not weak and length >= 4:
        cells[(0, length - 1)] = np.float32(0.95)
        lo = 1
        while lo + 8 < length - 1:  # stems of up to six pairs closing loops of four
            hi = min(lo + int(rs.randint(10, 40)), length - 2)
            for k in range(min(6, (hi - lo - 3) // 2)):
                cells[(lo + k, hi - k)] = np.float32(0.95)
            lo = hi + 1
    rowptr, col, val = [0], [], []
    for i in range(length):
        for (a, j) in sorted(c for c in cells if c[0] == i):
            col.append(j)
            val.append(cells[(a, j)])
        rowptr.append(len(col))
    return np.array(rowptr, np.uint32), np.array(col, np.uint32), np.array(val, np.float32)


def _dense(row):
    rowptr, col, val = row
    length = len(rowptr) - 1
    p = np.zeros((length, length), np.float32)
    for i in range(length):
        p[i, col[rowptr[i]:rowptr[i + 1]]] = val[rowptr[i]:rowptr[i + 1]]
    return p


def _gapped(rs, lengths, width):
    """a mask [n, width] that places lengths[r] residues in row r at random columns"""
    mask = np.zeros((len(lengths), width), np.uint8)
    for r, n in enumerate(lengths):
        mask[r, np.sort(rs.permutation(width)[:n])] = 1
    return mask


class Batch:
    pass


@pytest.fixture(scope="module")
def batch(oracle):
    """The mixed batch, its sequences and supplied rows, and per alignment the oracle's structure: built once."""
    rs = np.random.RandomState(2024)
    b = Batch()
    b.seqs = ["".join(rs.choice(list("ACGU"), n)) for n in LENS]
    b.rows = [_bp_rows(rs, n, weak=(k == WEAK)) for k, n in enumerate(LENS)]
    b.p = [_dense(r) for r in b.rows]
    b.alns = [(np.array([k], np.uint32), np.ones((1, n), np.uint8)) for k, n in enumerate(LENS)]
    b.single_row = len(b.alns)
    # rows with gaps: two and three rows, the second one's sequences not in index order; five rows over 262 columns
    b.alns.append((np.array([6, 7], np.uint32), _gapped(rs, [64, 65], 71)))
    b.alns.append((np.array([7, 5, 6], np.uint32), _gapped(rs, [65, 63, 64], 70)))
    b.alns.append((np.array([8, 10, 9, 5, 12], np.uint32), _gapped(rs, [255, 257, 256, 63, 40], 262)))
    b.want = [oracle.nussinov(b.p[k], None, TH) for k in range(b.single_row)]
    return b


@pytest.fixture(scope="module")
def ctx(batch):
    c = capi.Context(0)
    c.set_sequences(batch.seqs)
    c.set_bp(batch.rows)
    yield c
    c.close()


def _size_class(length):
    """the launch an alignment of this width joins: by the decoder's dynamic LDS, 48 bytes a column"""
    lds = 48 * ((length + 3) & ~3) + 16
    return 0 if length <= 256 else 1 if lds <= 48 * 1024 else 2


def _launches(c, fn):
    c.stage_timing(True)
    try:
        c.stage_report()
        out = fn()
        rep = c.stage_report()
    finally:
        c.stage_timing(False)
    return out, rep.get("k_nussinov_batch", (0, 0, 0))[2]


def _bits(results):
    return [(np.float32(s).tobytes(), ss.tobytes()) for s, ss in results]


def test_mixed_batch_against_the_oracle_and_the_single_call(batch, ctx, oracle):
    got, launches = _launches(ctx, lambda: ctx.consensus_structures(batch.alns, TH))
    assert len(got) == len(batch.alns)
    pl = oracle.pipeline(["s%d" % k for k in range(len(LENS))], batch.seqs, oracle.params(fold_model=1), bp=batch.rows)
    assert launches == len({_size_class(m.shape[1]) for _, m in batch.alns}) == 3  # up to 256 columns; 257 and 262; 1 100
    for k, (score, ss) in enumerate(got):
        seq, mask = batch.alns[k]
        s1, ss1, p1 = ctx.consensus_structure(seq, mask, TH, want_p=True)
        assert ss.tobytes() == ss1.tobytes() and np.float32(score).tobytes() == np.float32(s1).tobytes(), k
        if k < batch.single_row:
            assert np.array_equal(p1, batch.p[k]), k  # the one row's own matrix, as supplied
            ws, wss = batch.want[k]
        else:
            assert p1.tobytes() == pl.average_basepairing(seq, mask).tobytes(), k  # the rows' average: orc_pipeline_average_basepairing
            ws, wss = oracle.nussinov(p1, None, TH)
        assert ss.tobytes() == wss.tobytes() and np.float32(score).tobytes() == np.float32(ws).tobytes(), k
        paired = int(np.sum(wss != NONE))
        if k == WEAK:
            assert paired == 0 and np.float32(ws) == 0
        elif mask.shape[1] >= 5:
            assert paired >= 1, k  # an all-unpaired answer cannot pass
        elif mask.shape[1] < 4:
            assert paired == 0
    pl.close()
    # the multi-row averages depend on the order of the rows: the same rows in index order are another alignment
    seq, mask = batch.alns[batch.single_row + 1]
    order = np.argsort(seq)
    assert not np.array_equal(order, np.arange(len(seq)))
    s_sorted, ss_sorted, _ = ctx.consensus_structure(seq[order], mask[order], TH)
    again = ctx.consensus_structures([(seq[order], mask[order])], TH)
    assert _bits(again) == _bits([(s_sorted, ss_sorted)])


def test_chunks_do_not_change_results(batch, ctx, monkeypatch):
    want = _bits(ctx.consensus_structures(batch.alns, TH))
    sizes = [int(capi._structure_bytes(m.shape[0], m.shape[1])) for _, m in batch.alns]
    for budget in (1, sizes[10] + sizes[11], sizes[11]):  # every alignment alone; the 1 100-column one closes a chunk, or runs alone
        monkeypatch.setenv("DAFS_HIP_CS_BATCH_BYTES", str(budget))
        chunks = pipeline.pack_families(sizes, budget)
        expect = sum(len({_size_class(batch.alns[k][1].shape[1]) for k in chunk}) for chunk in chunks)
        got, launches = _launches(ctx, lambda: ctx.consensus_structures(batch.alns, TH))
        assert len(chunks) >= 3 and launches == expect >= 3, (budget, launches, expect)
        assert _bits(got) == want, budget
    monkeypatch.delenv("DAFS_HIP_CS_BATCH_BYTES")
    one, launches = _launches(ctx, lambda: ctx.consensus_structures(batch.alns[9:10], TH))
    assert launches == 1 and _bits(one) == want[9:10]
    none, launches = _launches(ctx, lambda: ctx.consensus_structures([], TH))
    assert none == [] and launches == 0


def test_global_table_form_gives_the_same_bits(batch, ctx, monkeypatch):
    """DAFS_HIP_NUSS_GLOBAL: every alignment takes the span-ordered form on global tables (the form beyond ~9 900 columns),
    in a launch of its own class; two chunks"""
    alns = batch.alns[:11] + batch.alns[13:]
    want = _bits(ctx.consensus_structures(alns, TH))
    sizes = [int(capi._structure_bytes(m.shape[0], m.shape[1])) for _, m in alns]
    monkeypatch.setenv("DAFS_HIP_NUSS_GLOBAL", "1")
    monkeypatch.setenv("DAFS_HIP_CS_BATCH_BYTES", str(sum(sizes[:9])))
    got, launches = _launches(ctx, lambda: ctx.consensus_structures(alns, TH))
    assert launches == len(pipeline.pack_families(sizes, sum(sizes[:9]))) >= 2
    assert _bits(got) == want
    for k in (4, 7, 10, 13):  # and the single call in the same form
        s1, ss1, _ = ctx.consensus_structure(alns[k][0], alns[k][1], TH)
        assert _bits([got[k]]) == _bits([(s1, ss1)])
    monkeypatch.setenv("DAFS_HIP_CS_BATCH_BYTES", "many")  # no number: ignored, one chunk
    got, launches = _launches(ctx, lambda: ctx.consensus_structures(alns, TH))
    assert launches == 1 and _bits(got) == want


def _stems(rs, length):
    """rows of a long sequence, built array-wise: hairpins of 0.9 end to end and one weak entry per row"""
    col = np.full(length, -1, np.int64)
    lo = 0
    while lo + 12 < length:
        hi = min(lo + int(rs.randint(12, 60)), length - 1)
        k = np.arange(min(8, (hi - lo - 3) // 2))
        col[lo + k] = hi - k
        lo = hi + 1
    rowptr, cols, vals = [0], [], []
    for i in range(length):
        if col[i] >= 0:
            cols.append(col[i])
            vals.append(0.9)
        elif i + 5 < length:
            cols.append(min(i + 5 + int(rs.randint(0, 50)), length - 1))
            vals.append(0.05 + 0.2 * rs.rand())
        rowptr.append(len(cols))
    return np.array(rowptr, np.uint32), np.array(cols, np.uint32), np.array(vals, np.float32)


def test_forms_with_two_and_no_candidate_heads_in_lds():
    """beyond 3 328 columns the workgroup form keeps two candidates per column in LDS, beyond 4 992 none: both in one call,
    against the single call"""
    rs = np.random.RandomState(8)
    lens = [3400, 5000, 120]
    c = capi.Context(0)
    try:
        c.set_sequences(["".join(rs.choice(list("ACGU"), n)) for n in lens])
        c.set_bp([_stems(rs, n) for n in lens])
        alns = [(np.array([k], np.uint32), np.ones((1, n), np.uint8)) for k, n in enumerate(lens)]
        got, launches = _launches(c, lambda: c.consensus_structures(alns, TH))
        assert launches == 2  # 120 columns; the two wide ones together
        for (seq, mask), g in zip(alns, got):
            s1, ss1, _ = c.consensus_structure(seq, mask, TH)
            assert _bits([g]) == _bits([(s1, ss1)]) and int(np.sum(ss1 != NONE)) > mask.shape[1] // 20
    finally:
        c.close()


def test_alignments_of_two_families_in_one_call(batch):
    c = capi.Context(0)
    try:
        keep = [5, 6, 7, 12, 3, 4]  # family 0: sequences 0..2, family 1: 3..5
        c.set_sequences([batch.seqs[k] for k in keep])
        c.set_families([0, 3, 6])
        c.set_bp([batch.rows[k] for k in keep])
        rs = np.random.RandomState(5)
        alns = [(np.array([1, 0, 2], np.uint32), _gapped(rs, [64, 63, 65], 69)), (np.array([3, 5], np.uint32), _gapped(rs, [40, 5], 41)),
                (np.array([2], np.uint32), np.ones((1, 65), np.uint8)), (np.array([4], np.uint32), np.ones((1, 4), np.uint8)),
                (np.array([3], np.uint32), np.ones((1, 40), np.uint8))]
        got = c.consensus_structures(alns, TH)
        for (seq, mask), g in zip(alns, got):
            s1, ss1, _ = c.consensus_structure(seq, mask, TH)
            assert _bits([g]) == _bits([(s1, ss1)])
        assert sum(int(np.sum(ss != NONE)) for _, ss in got) > 0
    finally:
        c.close()


def _raw_call(c, alns, th, ss, score):
    n_rows = np.array([m.shape[0] for _, m in alns], np.uint32)
    lens = np.array([m.shape[1] for _, m in alns], np.uint32)
    seq = np.ascontiguousarray(np.concatenate([s for s, _ in alns]), np.uint32)
    mask = np.ascontiguousarray(np.concatenate([m.reshape(-1) for _, m in alns]), np.uint8)
    return capi._consensus_structures(c._h, len(alns), n_rows.ctypes.data, lens.ctypes.data, seq.ctypes.data, mask.ctypes.data, th,
                                      ss.ctypes.data, score.ctypes.data)


def test_refusals_leave_the_outputs_and_the_context_alone(batch, ctx):
    good = [batch.alns[4], batch.alns[batch.single_row], batch.alns[6]]
    want = _bits(ctx.consensus_structures(good, TH))
    total = sum(m.shape[1] for _, m in good)
    wrong_count = batch.alns[batch.single_row][1].copy()
    wrong_count[1, np.flatnonzero(wrong_count[1])[0]] = 0  # one residue of the second row is not placed
    bad_calls = [[good[0], (np.array([len(LENS)], np.uint32), np.ones((1, 5), np.uint8)), good[2]],  # a sequence index out of range
                 [good[0], (batch.alns[batch.single_row][0], wrong_count), good[2]]]
    for bad in bad_calls:
        ss = np.full(sum(m.shape[1] for _, m in bad), 0xABCDEF01, np.uint32)
        score = np.full(len(bad), -7.5, np.float32)
        assert _raw_call(ctx, bad, TH, ss, score) == -1  # DAFS_HIP_EINVAL
        assert np.all(ss == 0xABCDEF01) and np.all(score == -7.5)
        assert _bits(ctx.consensus_structures(good, TH)) == want
    empty = capi.Context(0)  # sequences, but no base-pairing store
    try:
        empty.set_sequences(batch.seqs)
        ss = np.full(total, 0xABCDEF01, np.uint32)
        score = np.full(len(good), -7.5, np.float32)
        assert _raw_call(empty, good, TH, ss, score) == -1
        assert np.all(ss == 0xABCDEF01) and np.all(score == -7.5)
        empty.set_bp(batch.rows)
        assert _bits(empty.consensus_structures(good, TH)) == want
    finally:
        empty.close()


# ---- the drivers ----
def _own_structures(c, relaxed, th, oracle):
    """per sequence of the context the oracle's structure of its own rows in the store"""
    return [oracle.nussinov(_dense(r), None, th)[1] for r in c.bp(relaxed)]


def test_run_with_row_structures(oracle):
    recs = synth.family_set(5, 80)
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    c = capi.Context(0)
    try:
        plain = pipeline.run(names, seqs, ctx=c, reliability=True)
        got = pipeline.run(names, seqs, ctx=c, reliability=True, row_structures=True)
        want = _own_structures(c, 1, 0.2, oracle)  # rows are printed in sequence order
        assert got.output == plain.output and got.ss.tobytes() == plain.ss.tobytes()
        assert len(got.row_ss) == 5 and all(a.tobytes() == b.tobytes() for a, b in zip(got.row_ss, want))
        assert sum(int(np.sum(x != NONE)) for x in got.row_ss) > 0
        assert got.row_ss_str == [stockholm.row_ss_str(row, x) for row, x in zip(got.rows, want)]
        lines = got.stockholm.split("\n")
        assert [ln for ln in lines if not (ln.startswith("#=GR ") and ln.split()[2] == "SS")] == plain.stockholm.split("\n")
        sto_names = stockholm.names(names)
        for nm, text in zip(sto_names, got.row_ss_str):
            at = [k for k, ln in enumerate(lines) if ln.startswith("#=GR %s SS " % nm)]
            assert len(at) == 1 and lines[at[0]].split()[-1] == text and lines[at[0] - 1].startswith("#=GR %s PP " % nm)
    finally:
        c.close()


def test_run_batch_and_pairwise_equal_single_runs():
    fams = []
    for k, (n, length) in enumerate([(3, 50), (2, 70), (4, 40), (2, 60)]):
        recs = synth.family_set(n, length, seed=900 + k)
        fams.append(([nm for nm, _ in recs], [s for _, s in recs]))
    c = capi.Context(0)
    try:
        got = pipeline.run_batch(fams, ctx=c, row_structures=True)
        for (names, seqs), g in zip(fams, got):
            want = pipeline.run(names, seqs, ctx=c, row_structures=True)
            assert g.output == want.output and g.ss.tobytes() == want.ss.tobytes()
            assert [x.tobytes() for x in g.row_ss] == [x.tobytes() for x in want.row_ss] and g.row_ss_str == want.row_ss_str
        recs = [synth.random_set(1, length, seed=950 + k, jitter=0.0)[0] for k, length in enumerate([40, 55, 70, 85, 100, 120])]
        names, seqs = ["r%d" % k for k in range(6)], [s for _, s in recs]
        pw = pipeline.pairwise(names, seqs, ctx=c, row_structures=True)
        for (x, y), g in zip(pw.pairs, pw.results):
            want = pipeline.run([names[x], names[y]], [seqs[x], seqs[y]], ctx=c, row_structures=True)
            assert g.output == want.output
            assert [v.tobytes() for v in g.row_ss] == [v.tobytes() for v in want.row_ss]
    finally:
        c.close()


def _cli(*args):
    r = subprocess.run([DAFS] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_row_structures_equal_the_python_blocks(tmp_path):
    recs = synth.family_set(4, 60, seed=77)
    names, seqs = [n for n, _ in recs], [s for _, s in recs]
    fa, sto = tmp_path / "fam.fa", tmp_path / "out.sto"
    fa.write_text(synth.to_fasta(recs))
    want = pipeline.run(names, seqs, reliability=True, row_structures=True)
    assert _cli("--stockholm", sto, "--row-structures", fa) == want.output
    assert sto.read_text() == want.stockholm and "#=GR %s SS " % stockholm.names(names)[0] in want.stockholm
    # --seed: the first three sequences' alignment as the seed, the fourth added
    seed = pipeline.run(names[:3], seqs[:3])
    seed_fa, new_fa = tmp_path / "seed.fa", tmp_path / "new.fa"
    seed_fa.write_text(seed.output)
    new_fa.write_text(synth.to_fasta(recs[3:]))
    snames, srows = stockholm.read_seed(str(seed_fa))
    want = pipeline.add(snames, srows, names[3:], seqs[3:], reliability=True, row_structures=True)
    assert _cli("--seed", seed_fa, "--stockholm", sto, "--row-structures", new_fa) == want.output
    assert sto.read_text() == want.stockholm and want.stockholm.count(" SS ") >= 4
    # --pairwise: one block per pair
    pw = pipeline.pairwise(names, seqs, reliability=True, row_structures=True)
    out = _cli("--pairwise", "--stockholm", sto, "--row-structures", fa)
    assert out == "".join("==> %d %d <==\n" % (x + 1, y + 1) + r.output for (x, y), r in zip(pw.pairs, pw.results))
    assert sto.read_text() == "".join(r.stockholm for r in pw.results)


def test_fold_each(oracle):
    recs = [synth.random_set(1, length, seed=970 + k, jitter=0.0)[0] for k, length in enumerate([30, 45, 60, 80, 100, 120])]
    names, seqs = ["f%d" % k for k in range(6)], [s for _, s in recs]
    c = capi.Context(0)
    try:
        got = pipeline.fold_each(names, seqs, th=0.2, ctx=c)
        rows = c.bp(0)  # the un-relaxed rows fold_each decoded
        assert [g.name for g in got] == names
        for g, r in zip(got, rows):
            score, ss = oracle.nussinov(_dense(r), None, 0.2)
            assert g.ss.tobytes() == ss.tobytes() and np.float32(g.score).tobytes() == np.float32(score).tobytes()
            assert g.ss_str == capi.make_brackets(ss)
        assert sum(g.ss_str.count("(") for g in got) > 0
    finally:
        c.close()
