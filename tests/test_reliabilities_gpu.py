"""GPU tests of dafs_hip_alignment_reliabilities (Context.alignment_reliabilities): many alignments
annotated in one call, the rows that are wanted only, a relaxed matching store that holds listed pairs, the chunks.  Every
comparison is bit for bit, against the single call and against the restatement of tests/reliability_ref.py."""
import numpy as np
import pytest

import reliability_ref as rr
from dafs_amd import capi, pipeline, synth

pytestmark = pytest.mark.gpu
NONE = rr.NONE
# three families of 1, 2 and 5 sequences; rows of 64, 65 and 129 residues are the edges of the blocks of 64 residues
LENS = [63, 64, 65, 129, 130, 20, 100, 64]
FIRST = [0, 1, 3, 8]


def _seqs():
    out = []
    for f in range(3):
        lens = LENS[FIRST[f]:FIRST[f + 1]]
        recs = synth.family_set(len(lens), 150, seed=900 + f)
        assert all(len(s) >= n for (_, s), n in zip(recs, lens))
        out += [s[:n] for (_, s), n in zip(recs, lens)]
    return out


def _gapped(rs, lengths, width):
    mask = np.zeros((len(lengths), width), np.uint8)
    for r, n in enumerate(lengths):
        mask[r, np.sort(rs.permutation(width)[:n])] = 1
    return mask


def _nested(rs, width):
    """a random nested structure: some of the pairs c -> width - 1 - c"""
    ss = np.full(width, NONE, np.uint32)
    for c in range(width // 2 - 2):
        if rs.rand() < 0.3:
            ss[c] = width - 1 - c
    return ss


class World:
    pass


@pytest.fixture(scope="module")
def world():
    """The context after phase 1 with the transforms, the alignments of the one call, and what the restatement gives for each:
    built once and left unchanged."""
    rs = np.random.RandomState(17)
    w = World()
    w.seqs = _seqs()
    w.ctx = capi.Context(0)
    w.ctx.set_sequences(w.seqs)
    w.ctx.set_families(FIRST)
    w.ctx.fold_posteriors(0.01)
    w.ctx.align_posteriors(fetch=False)
    w.ctx.consistency(0.25, 0.25)

    def aln(rows, width):
        return np.array(rows, np.uint32), _gapped(rs, [LENS[x] for x in rows], width)
    # widths 63, 64, 65 and 130: the edges of the steps of 64 columns (width 1: test_width_one)
    w.alns = [aln([0], 63),                # one row, no gap
              aln([1], 64),
              aln([2, 1], 65),             # descending order
              aln([7, 6, 5, 4, 3], 130),   # five rows, descending; 129 and 130 residues
              aln([3, 5, 6], 150),         # sequences 3, 5 and 6 a second time
              aln([1, 2], 70),
              aln([5], 24)]
    w.sss = [None, _nested(rs, 64), _nested(rs, 65), _nested(rs, 130), None, _nested(rs, 70), _nested(rs, 24)]
    stores = rr.context_stores(w.ctx, 1, 1)
    w.want = [rr.restate(s, m, ss, *stores) for (s, m), ss in zip(w.alns, w.sss)]
    yield w
    w.ctx.close()


def _same(a, b):
    assert a["residue"].tobytes() == b["residue"].tobytes()
    for k in ("col", "pair", "pair_rows"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.float64(a["expected_accuracy"]).tobytes() == np.float64(b["expected_accuracy"]).tobytes()


def _launches(c, fn):
    c.stage_timing(True)
    try:
        c.stage_report()
        out = fn()
        rep = c.stage_report()
    finally:
        c.stage_timing(False)
    return out, [rep.get(k, (0, 0, 0))[2] for k in ("k_rel_pos", "k_rel_residue", "k_rel_column")]


def test_one_call_equals_the_single_call_and_the_restatement(world):
    ctx = world.ctx
    got, launches = _launches(ctx, lambda: ctx.alignment_reliabilities(world.alns, world.sss))
    assert launches == [1, 1, 1]
    assert len(got) == len(world.alns)
    for a, ((seq, mask), ss) in enumerate(zip(world.alns, world.sss)):
        _same(got[a], ctx.alignment_reliability(seq, mask, ss))
        _same(got[a], world.want[a])
    assert any(g["pair_rows"].max() > 0 for g in got) and not got[0]["pair_rows"].any() and not got[4]["pair_rows"].any()
    assert got[0]["residue"].tolist() == [1.0] * 63 and got[0]["expected_accuracy"] == 1.0
    assert all(((g["residue"] >= 0) & (g["residue"] <= 1)).all() for g in got)
    # no structure anywhere: no pairs, the rest unchanged; an empty batch
    ns = ctx.alignment_reliabilities(world.alns)
    for g, n in zip(got, ns):
        assert n["residue"].tobytes() == g["residue"].tobytes() and n["col"].tobytes() == g["col"].tobytes() and not n["pair_rows"].any()
    assert ctx.alignment_reliabilities([]) == []
    # the un-relaxed stores
    raw = ctx.alignment_reliabilities(world.alns[2:4], world.sss[2:4], mp_relaxed=0, bp_relaxed=0)
    for g, ((seq, mask), ss) in zip(raw, zip(world.alns[2:4], world.sss[2:4])):
        _same(g, ctx.alignment_reliability(seq, mask, ss, mp_relaxed=0, bp_relaxed=0))
    assert raw[1]["residue"].tobytes() != got[3]["residue"].tobytes()


def test_width_one():
    """An alignment of one column: one row of one residue.  It has a context of its own, and only one-row alignments beside it,
    because a one-column alignment needs a one-residue sequence, and the three-family context runs phase 1 (folding, pair
    posteriors, transforms), which nothing in the project exercises below four residues.  A one-row alignment reads no store, so
    this context needs none; the call still takes the three kernels through len = 1 between other alignments of the chunk."""
    ctx = capi.Context(0)
    try:
        ctx.set_sequences(["A", "ACGU"])
        alns = [(np.array([0], np.uint32), np.ones((1, 1), np.uint8)), (np.array([1], np.uint32), np.ones((1, 4), np.uint8)),
                (np.array([0], np.uint32), np.ones((1, 1), np.uint8))]
        got = ctx.alignment_reliabilities(alns)
        for g, (seq, mask) in zip(got, alns):
            _same(g, ctx.alignment_reliability(seq, mask))
            _same(g, rr.restate(seq, mask, None, None, None))
        assert got[0]["residue"].tolist() == [1.0] and got[0]["col"].tolist() == [1.0]
    finally:
        ctx.close()


def test_wanted_rows(world):
    ctx = world.ctx
    full = ctx.alignment_reliabilities(world.alns, world.sss)
    off = [np.concatenate([[0], np.cumsum(m.sum(1))]).astype(np.int64) for _, m in world.alns]
    total = int(sum(o[-1] for o in off))
    # one row of the five-row alignment and one of the three-row one; everything of the others
    want = [None, None, None, np.arange(5) == 1, np.arange(3) == 2, None, None]
    pattern = np.frombuffer(np.arange(total, dtype=np.uint64).tobytes(), np.float64).copy()  # distinct bit patterns, no value repeated
    filled = pattern.copy()
    got = ctx.alignment_reliabilities(world.alns, world.sss, want=want, residue=filled)
    at = 0
    for a, g in enumerate(got):
        n = len(world.alns[a][0])
        for r in range(n):
            lo, hi = off[a][r], off[a][r + 1]
            if want[a] is None or want[a][r]:
                assert g["residue"][lo:hi].tobytes() == full[a]["residue"][lo:hi].tobytes(), (a, r)
            else:  # untouched
                assert g["residue"][lo:hi].tobytes() == pattern[at + lo:at + hi].tobytes(), (a, r)
        at += off[a][-1]
        for k in ("pair", "pair_rows"):
            assert g[k].tobytes() == full[a][k].tobytes()
        if want[a] is None:
            _same(g, full[a])
        else:
            assert np.isnan(g["col"]).all() and np.isnan(g["expected_accuracy"])
    # a single wanted row costs its own residue blocks only; no row wanted: no residue launch
    _, launches = _launches(ctx, lambda: ctx.alignment_reliabilities(world.alns[3:4], want=[np.zeros(5, bool)]))
    assert launches == [1, 0, 1]


@pytest.fixture(scope="module")
def listed():
    """A second context: three families seed + [new] over a seed of three sequences, phase 1, then the relaxed matching store
    once whole (the values to expect) and once with the (seed, new) pairs only"""
    recs = synth.family_set(6, 60, seed=930)
    seqs = [s for _, s in recs]
    m, n = 3, 4
    src = capi.Context(0)
    ctx = capi.Context(0)
    src.set_sequences(seqs)
    src.fold_posteriors(0.01)
    src.align_posteriors(capi.ALIGN_PROBCONS, 0.01, 0, m * 6 - m * (m + 1) // 2, fetch=False)
    ctx.families_from(src, [[0, 1, 2, 3 + j] for j in range(3)])
    src.close()
    ctx.consistency_bp(0.25)
    rs = np.random.RandomState(23)
    w = World()
    w.ctx = ctx
    w.alns = []
    for f in range(3):  # the new row first, as the drivers give it
        rows = [f * n + 3, f * n, f * n + 1, f * n + 2]
        w.alns.append((np.array(rows, np.uint32), _gapped(rs, [len(seqs[3 + f])] + [len(s) for s in seqs[:3]], 75)))
    w.sss = [_nested(rs, 75) for _ in range(3)]
    ctx.consistency_match(0.25)
    w.full = ctx.alignment_reliabilities(w.alns, w.sss)
    node_pairs = np.array([s * n - s * (s + 1) // 2 + m - s - 1 for s in range(m)], np.uint64)
    ctx.consistency_match_pairs(0.25, np.concatenate([node_pairs + np.uint64(f * (n * m // 2)) for f in range(3)]))
    yield w
    ctx.close()


def test_listed_store(listed):
    ctx = listed.ctx
    new_rows = [np.arange(4) == 0] * 3
    got = ctx.alignment_reliabilities(listed.alns, listed.sss, want=new_rows)
    for a, (g, f) in enumerate(zip(got, listed.full)):
        n = int(listed.alns[a][1][0].sum())
        assert g["residue"][:n].tobytes() == f["residue"][:n].tobytes() and not g["residue"][n:].any()
        assert g["pair"].tobytes() == f["pair"].tobytes() and g["pair_rows"].tobytes() == f["pair_rows"].tobytes()
        assert np.isnan(g["col"]).all() and np.isnan(g["expected_accuracy"])
    # a seed row reads the seed-seed pairs, which are not listed: refused, nothing written, and the next call works
    L = sum(m.shape[1] for _, m in listed.alns)
    for want in ([np.arange(4) < 2] * 3, [new_rows[0], new_rows[0], np.arange(4) == 3], None):
        res = np.full(sum(int(m.sum()) for _, m in listed.alns), 7.0)
        with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
            ctx.alignment_reliabilities(listed.alns, listed.sss, want=want, residue=res)
        assert (res == 7.0).all()
    with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
        ctx.alignment_reliability(*listed.alns[0])
    again = ctx.alignment_reliabilities(listed.alns, listed.sss, want=new_rows)
    assert [g["residue"].tobytes() for g in again] == [g["residue"].tobytes() for g in got] and L == 225
    # the un-relaxed store is whole
    ctx.alignment_reliabilities(listed.alns, listed.sss, mp_relaxed=0)


def test_chunks_do_not_change_results(world, monkeypatch):
    ctx = world.ctx
    want = ctx.alignment_reliabilities(world.alns, world.sss)
    sizes = [int(capi._reliability_bytes(m.shape[0], m.shape[1])) for _, m in world.alns]
    for budget in (1, sizes[0] + sizes[1] + sizes[2]):  # every alignment alone; three, then the rest one by one or in twos
        monkeypatch.setenv("DAFS_HIP_REL_BATCH_BYTES", str(budget))
        chunks = pipeline.pack_families(sizes, budget)
        got, launches = _launches(ctx, lambda: ctx.alignment_reliabilities(world.alns, world.sss))
        assert launches == [len(chunks)] * 3 and len(chunks) >= 3
        for g, f in zip(got, want):
            _same(g, f)
    assert len(pipeline.pack_families(sizes, 1)) == len(world.alns)
    monkeypatch.setenv("DAFS_HIP_REL_BATCH_BYTES", "many")  # no number: ignored, one chunk
    got, launches = _launches(ctx, lambda: ctx.alignment_reliabilities(world.alns, world.sss))
    assert launches == [1, 1, 1]
    for g, f in zip(got, want):
        _same(g, f)
    assert int(capi._reliability_batch_bytes()) > sum(sizes)


def _raw(c, alns, sss, outs, mp_relaxed=-1):
    """the library call itself, on arrays the binding would refuse to build"""
    n_rows = np.array([len(s) for s, _ in alns], np.uint32)
    lens = np.array([m.shape[1] for _, m in alns], np.uint32)
    seq = np.ascontiguousarray(np.concatenate([s for s, _ in alns] + [np.zeros(1, np.uint32)]), np.uint32)
    mask = np.ascontiguousarray(np.concatenate([m.reshape(-1) for _, m in alns] + [np.zeros(1, np.uint8)]), np.uint8)
    ss = None if sss is None else np.ascontiguousarray(np.concatenate(sss + [np.zeros(1, np.uint32)]), np.uint32)
    res, col, pair, rows, ea = outs
    return capi._alignment_reliabilities(c._h, len(alns), n_rows.ctypes.data, lens.ctypes.data, seq.ctypes.data, mask.ctypes.data,
                                         None if ss is None else ss.ctypes.data, None, mp_relaxed, -1, res.ctypes.data, col.ctypes.data,
                                         pair.ctypes.data, rows.ctypes.data, ea.ctypes.data)


def test_refusals_leave_the_outputs_and_the_context_alone(world):
    ctx = world.ctx
    good = (world.alns[5], world.sss[5])
    want = ctx.alignment_reliabilities([good[0]], [good[1]])[0]
    seq, mask = good[0]

    def refused(alns, sss, mp_relaxed=-1, c=ctx):
        outs = [np.full(4096, 3.0), np.full(1024, 3.0), np.full(1024, 3.0), np.full(1024, 3, np.uint32), np.full(8, 3.0)]
        assert _raw(c, alns, sss, outs, mp_relaxed) == -1
        assert all((o == 3).all() for o in outs)
        if c is ctx:
            _same(ctx.alignment_reliabilities([good[0]], [good[1]])[0], want)

    none70 = np.full(70, NONE, np.uint32)
    refused([good[0], (np.zeros(0, np.uint32), np.zeros((0, 70), np.uint8))], [good[1], none70])    # no rows
    refused([good[0], (np.array([1], np.uint32), np.zeros((1, 0), np.uint8))], [good[1], np.zeros(0, np.uint32)])  # no columns
    refused([good[0], (np.array([1, 8], np.uint32), mask)], [good[1], none70])                         # an unknown sequence
    refused([good[0], (np.array([1, 1], np.uint32), np.stack([mask[0], mask[0]]))], [good[1], none70])  # one sequence twice
    two = np.zeros((2, 70), np.uint8)
    two[0, :63] = 1
    two[1, :64] = 1
    refused([good[0], (np.array([0, 1], np.uint32), two)], [good[1], none70])                          # rows of two families
    short = mask.copy()
    short[1, np.nonzero(short[1])[0][0]] = 0
    refused([(seq, short), good[0]], [good[1], good[1]])                                               # a residue that is not placed
    crossed = none70.copy()
    crossed[3], crossed[5] = 10, 10
    ends_early = none70.copy()
    ends_early[69] = 0
    for bad in (crossed, ends_early):
        refused([good[0], good[0]], [good[1], bad])                                                    # a bad ss
    # an invalid store: a context with sequences and nothing else
    empty = capi.Context(0)
    try:
        empty.set_sequences(world.seqs)
        empty.set_families(FIRST)
        refused([good[0]], None, c=empty)          # two rows need a matching store
        refused([world.alns[0]], [np.full(63, NONE, np.uint32)], c=empty)  # a structure needs a base-pairing store
        one = empty.alignment_reliabilities([world.alns[0]])[0]  # one row without a structure reads none
        assert one["residue"].tolist() == [1.0] * 63
    finally:
        empty.close()
    # the relaxed store of a context that has none yet; a folding in flight
    fresh = capi.Context(0)
    try:
        fresh.set_sequences(world.seqs)
        fresh.set_families(FIRST)
        fresh.fold_posteriors(0.01)
        fresh.align_posteriors(fetch=False)
        refused([good[0]], [good[1]], mp_relaxed=1, c=fresh)
        assert _raw(fresh, [good[0]], [good[1]], [np.zeros(4096), np.zeros(1024), np.zeros(1024), np.zeros(1024, np.uint32), np.zeros(8)]) == 0
        fresh.fold_begin(0.01)
        try:
            refused([good[0]], [good[1]], c=fresh)
        finally:
            fresh.fold_end()
        assert _raw(fresh, [good[0]], [good[1]], [np.zeros(4096), np.zeros(1024), np.zeros(1024), np.zeros(1024, np.uint32), np.zeros(8)]) == 0
    finally:
        fresh.close()


def test_drivers_make_one_call_per_chunk():
    """run_batch, pairwise and add_each annotate all alignments of a chunk in one call: three launches, however many there are"""
    fams = [([n for n, _ in recs], [s for _, s in recs]) for recs in (synth.family_set(3, 40, seed=940), synth.random_set(2, 35, seed=941),
                                                                       synth.random_set(1, 30, seed=942), synth.family_set(4, 45, seed=943))]
    ctx = capi.Context(0)
    try:
        got, launches = _launches(ctx, lambda: pipeline.run_batch(fams, ctx=ctx, reliability=True))
        assert launches == [1, 1, 1]
        for (names, seqs), r in zip(fams, got):
            assert r.stockholm == pipeline.run(names, seqs, ctx=ctx, reliability=True).stockholm
        names, seqs = fams[3]
        pw, launches = _launches(ctx, lambda: pipeline.pairwise(names, seqs, ctx=ctx, reliability=True))
        assert len(pw.results) == 6 and pw.chunks == [list(range(6))] and launches == [1, 1, 1]
        pw, launches = _launches(ctx, lambda: pipeline.pairwise(names, seqs, ctx=ctx, reliability=True, max_bytes=1))
        assert len(pw.chunks) == 6 and launches == [6, 6, 6]
        rows = pipeline.run(names, seqs, ctx=ctx).rows
        new = [s for _, s in synth.family_set(7, 45, seed=943)[4:]]
        each, launches = _launches(ctx, lambda: pipeline.add_each(names, rows, ["a", "b", "c"], new, ctx=ctx, reliability=True))
        assert each.chunks == [[0, 1, 2]] and launches == [1, 1, 1] and all(r.stockholm for r in each.results)
    finally:
        ctx.close()
