"""GPU tests of the two device pieces behind pipeline.add_each: dafs_hip_families_from, families over
arbitrary subsets of one N-sequence phase 1 gathered on the device, and dafs_hip_consistency_match_pairs, the matching
transform for a list of output pairs.  Both must give, bit for bit, what the existing paths give."""
import ctypes as C

import numpy as np
import pytest

from dafs_amd import capi, synth

pytestmark = pytest.mark.gpu
u32p = capi.u32p


def _exact(recs, lens):
    """the sequences cut to exactly these lengths"""
    assert all(len(s) >= n for (_, s), n in zip(recs, lens))
    return [s[:n] for (_, s), n in zip(recs, lens)]


def _seven():
    """lengths 9, 15, 16, 17, 40, 64, 70: rows shorter than a 16-lane group, rows at and over a wavefront edge; 9, 16, 40 and 70
    are members of one family, the others unrelated"""
    fam = _exact(synth.family_set(4, 80, seed=501), [9, 16, 40, 70])
    rnd = [synth.random_set(1, n, seed=510 + n, jitter=0.0)[0][1] for n in (15, 17, 64)]
    seqs = [fam[0], rnd[0], fam[1], rnd[1], fam[2], rnd[2], fam[3]]
    assert [len(s) for s in seqs] == [9, 15, 16, 17, 40, 64, 70]
    return seqs


def _fetch(ctx):
    """dafs_hip_align_fetch: pairs, scores, counts, row pointers, columns, values as bytes"""
    npairs, nnz, nrp = C.c_uint64(), C.c_uint64(), C.c_uint64()
    capi.check(capi._align_result_size(ctx._h, C.byref(npairs), C.byref(nnz), C.byref(nrp)))
    n = npairs.value
    px = np.zeros(n, np.uint32); py = np.zeros(n, np.uint32); sim = np.zeros(n, np.float32); cnt = np.zeros(n, np.uint32)
    rowptr = np.zeros(nrp.value, np.uint32); col = np.zeros(2 * nnz.value, np.uint32); val = np.zeros(2 * nnz.value, np.float32)
    capi.check(capi._align_fetch(ctx._h, px.ctypes.data, py.ctypes.data, sim.ctypes.data, cnt.ctypes.data, rowptr.ctypes.data,
                                 col.ctypes.data, val.ctypes.data))
    return tuple(a.tobytes() for a in (px, py, sim, cnt, rowptr, col, val))


def _mp_bytes(pp):
    return (pp.pair_x.tobytes(), pp.pair_y.tobytes(), pp.nnz.tobytes(), pp._rowptr.tobytes(), pp._col.tobytes(), pp._val.tobytes())


def _bp_bytes(rows):
    return [(r.tobytes(), c.tobytes(), v.tobytes()) for r, c, v in rows]


def _state(ctx):
    return _fetch(ctx), _bp_bytes(ctx.bp(0)), [b.tobytes() for b in ctx.sim_blocks()]


def _direct(seqs, families, model):
    """a context built directly on the families' sequences"""
    ref = capi.Context(0)
    ref.set_sequences([seqs[x] for f in families for x in f])
    if len(families) > 1:
        ref.set_families(np.concatenate([[0], np.cumsum([len(f) for f in families])]))
    ref.fold_posteriors(0.01)
    ref.align_posteriors(model, 0.01, fetch=False)
    return ref


def _source(seqs, model=capi.ALIGN_PROBCONS, pair_end=0):
    src = capi.Context(0)
    src.set_sequences(seqs)
    src.fold_posteriors(0.01)
    src.align_posteriors(model, 0.01, 0, pair_end, fetch=False)
    return src


@pytest.mark.parametrize("model", [capi.ALIGN_PROBCONS, capi.ALIGN_CONTRALIGN], ids=["probcons", "contralign"])
def test_gather_equals_a_direct_build(model):
    seqs = _seven()
    families = [[0, 1, 2, 5], [0, 1, 2, 6], [3], [1, 4]]
    src = _source(seqs, model)
    before = _state(src)
    dst = capi.Context(0)
    dst.families_from(src, families)
    ref = _direct(seqs, families, model)
    got, want = _state(dst), _state(ref)
    assert got[0] == want[0]   # align_fetch: pairs, scores, nnz, row pointers, columns, values
    assert got[1] == want[1]   # bp_fetch
    assert got[2] == want[2]   # sim_blocks
    assert _mp_bytes(dst.mp(0)) == _mp_bytes(ref.mp(0))
    blocks = dst.sim_blocks()
    assert [b.shape for b in blocks] == [(4, 4), (4, 4), (1, 1), (2, 2)] and blocks[2].tolist() == [[1.0]]
    for c in (dst, ref):  # the stores are un-relaxed and the transforms run on them unchanged
        c.consistency_match(0.25)
        c.consistency_bp(0.25)
    assert _mp_bytes(dst.mp(1)) == _mp_bytes(ref.mp(1))
    assert _bp_bytes(dst.bp(1)) == _bp_bytes(ref.bp(1))
    # a second chunk cut from the same source; the source as it was
    dst.families_from(src, [[2, 3, 4, 5, 6]])
    ref.close()
    ref = _direct(seqs, [[2, 3, 4, 5, 6]], model)
    assert _state(dst) == _state(ref)
    assert _state(src) == before
    for c in (src, dst, ref):
        c.close()


def test_two_member_families_equal_pairs_from():
    seqs = _seven()
    src = _source(seqs)
    pairs = [(0, 6), (2, 4), (0, 1), (5, 6), (2, 4)]
    a, b = capi.Context(0), capi.Context(0)
    a.families_from(src, [[x, y] for x, y in pairs])
    b.pairs_from(src, [x for x, _ in pairs], [y for _, y in pairs])
    assert _state(a) == _state(b)
    for c in (src, a, b):
        c.close()


def test_prefix_stores():
    seqs = _seven()[:5]
    n, m = 5, 3
    prefix = m * n - m * (m + 1) // 2  # the pairs (x, y) with x < 3
    src = _source(seqs, pair_end=prefix)
    dst = capi.Context(0)
    families = [[0, 1, 2, 3], [0, 1, 2, 4], [2, 4], [3], [1, 3]]
    dst.families_from(src, families)
    ref = _direct(seqs, families, capi.ALIGN_PROBCONS)
    assert _state(dst) == _state(ref)
    with pytest.raises(capi.DafsHipError, match=r"code -1\b"):  # needs pair (3, 4), which the prefix does not hold
        dst.families_from(src, [[0, 1], [0, 3, 4]])
    dst.families_from(src, families)  # and the context still works
    dst.consistency_match(0.25)
    ref.consistency_match(0.25)
    assert _mp_bytes(dst.mp(1)) == _mp_bytes(ref.mp(1))
    for c in (src, dst, ref):
        c.close()


def _raw(dst, src, nfam, first, member):
    first = np.ascontiguousarray(first, np.uint32)
    member = np.ascontiguousarray(member, np.uint32)
    return capi._families_from(dst, src, nfam, first.ctypes.data_as(u32p), member.ctypes.data_as(u32p))


def test_refusals_leave_the_contexts_usable():
    seqs = _seven()[:5]
    src, dst = _source(seqs), capi.Context(0)
    EINVAL = -1

    def refused(families, s=None):
        with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
            dst.families_from(src if s is None else s, families)
    ok = ([0, 2, 2], [0, 1])
    assert _raw(None, src._h, 1, *ok) == EINVAL and _raw(dst._h, None, 1, *ok) == EINVAL   # null contexts
    assert _raw(src._h, src._h, 1, *ok) == EINVAL                                           # equal contexts
    try:
        other = capi.Context(1)
    except capi.DafsHipError:
        other = None  # one device only: no second one to refuse
    if other is not None:
        with pytest.raises(capi.DafsHipError, match=r"code -1\b"):                          # different devices
            other.families_from(src, [[0, 1]])
        other.close()
    two = capi.Context(0)                                                                   # src with two families
    two.set_sequences(seqs[:4])
    two.set_families([0, 2, 4])
    two.fold_posteriors(0.01)
    two.align_posteriors(fetch=False)
    refused([[0, 1]], two)
    two.set_sequences(seqs[:4])                                                             # no base-pairing store
    two.align_posteriors(fetch=False)
    refused([[0, 1]], two)
    two.set_sequences(seqs[:4])                                                             # no matching store
    two.fold_posteriors(0.01)
    refused([[0, 1]], two)
    two.align_posteriors(pair_begin=2, pair_end=6, fetch=False)                             # a store that does not start at pair 0
    refused([[1, 2]], two)
    two.align_posteriors(pair_begin=0, pair_end=2, fetch=False)                             # a pair behind the prefix: (1, 2) is id 3
    refused([[1, 2]], two)
    two.close()
    src.fold_begin(0.01)                                                                    # a folding in flight on src,
    refused([[0, 1]])
    src.fold_end()
    dst.set_sequences(seqs[:2])
    dst.fold_begin(0.01)                                                                    # and on dst
    refused([[0, 1]])
    dst.fold_end()
    refused([])                                                                             # nfam == 0
    assert _raw(dst._h, src._h, 1, [1, 3], [0, 1, 2]) == EINVAL                             # first[0] != 0
    assert _raw(dst._h, src._h, 2, [0, 3, 2], [0, 1, 2]) == EINVAL                          # first does not ascend
    refused([[0, 1], []])                                                                   # an empty family
    refused([[0, 5]])                                                                       # a member >= N
    refused([[1, 1]])                                                                       # members not strictly ascending
    refused([[0, 2, 1]])
    # both go on: dst takes families and runs the transforms, src is what it was
    dst.families_from(src, [[0, 2, 4], [1, 3]])
    dst.consistency_match(0.25)
    dst.consistency_bp(0.25)
    assert list(dst.mp(1).pair_x) == [0, 0, 1, 3] and list(dst.mp(1).pair_y) == [1, 2, 2, 4]
    ref = _source(seqs)
    assert _state(src) == _state(ref)
    for c in (src, dst, ref):
        c.close()


def _two_families():
    seqs = _exact(synth.family_set(4, 70, seed=520), [20, 33, 47, 60]) + _exact(synth.family_set(3, 70, seed=521), [60, 21, 40])
    ctx = capi.Context(0)
    ctx.set_sequences(seqs)
    ctx.set_families([0, 4, 7])
    ctx.fold_posteriors(0.01)
    ctx.align_posteriors(fetch=False)
    return ctx, seqs


def test_listed_transform_equals_the_full_one():
    ctx, seqs = _two_families()
    npairs = 6 + 3
    listed = [0, 2, 5, 6, 8]  # a strict subset with the first and the last pair, pairs of both families
    ctx.consistency_match(0.25)
    full = ctx.mp(1)
    full_rows = [[a.tobytes() for a in full.csr(p, t)] for p in range(npairs) for t in (False, True)]
    # an alignment of family 0 for the reliability call: every row left-justified
    lens = [len(s) for s in seqs[:4]]
    mask = np.array([[1] * n + [0] * (max(lens) - n) for n in lens], np.uint8)
    rel_full = ctx.alignment_reliability(np.arange(4, dtype=np.uint32), mask)
    ctx.consistency_match_pairs(0.25, listed)
    part = ctx.mp(1)
    assert part.pair_x.tobytes() == full.pair_x.tobytes() and part.pair_y.tobytes() == full.pair_y.tobytes()
    for p in range(npairs):
        for t in (False, True):
            rp, col, val = part.csr(p, t)
            if p in listed:
                assert [rp.tobytes(), col.tobytes(), val.tobytes()] == full_rows[2 * p + t], (p, t)
            else:
                assert part.nnz[p] == 0 and not rp.any() and len(col) == 0, (p, t)
    assert [int(part.nnz[p]) for p in listed] == [int(full.nnz[p]) for p in listed]
    # the reliability annotation would read the empty pairs as zero probabilities: refused; the un-relaxed store still serves
    with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
        ctx.alignment_reliability(np.arange(4, dtype=np.uint32), mask)
    with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
        ctx.alignment_reliability(np.arange(4, dtype=np.uint32), mask, mp_relaxed=1)
    ctx.alignment_reliability(np.arange(4, dtype=np.uint32), mask, mp_relaxed=0)
    ctx.alignment_reliability(np.array([2], np.uint32), np.ones((1, lens[2]), np.uint8))  # one row reads no matching store
    ctx.consistency_match(0.25)
    again = ctx.alignment_reliability(np.arange(4, dtype=np.uint32), mask)
    assert again["residue"].tobytes() == rel_full["residue"].tobytes() and again["col"].tobytes() == rel_full["col"].tobytes()
    assert _mp_bytes(ctx.mp(1)) == _mp_bytes(full)
    # every pair listed is the full transform
    ctx.consistency_match_pairs(0.25, list(range(npairs)))
    assert _mp_bytes(ctx.mp(1)) == _mp_bytes(full)
    ctx.close()


def test_listed_transform_refusals():
    ctx, seqs = _two_families()

    def refused(w, ids):
        with pytest.raises(capi.DafsHipError, match=r"code -1\b"):
            ctx.consistency_match_pairs(w, ids)
    refused(0.0, [0, 1])       # weight 0: nothing to compute
    refused(0.25, [])          # an empty list
    refused(0.25, [1, 1])      # not strictly ascending
    refused(0.25, [3, 2])
    refused(0.25, [0, 9])      # not a pair of the context (6 + 3 pairs)
    ctx.align_posteriors(pair_begin=0, pair_end=4, fetch=False)  # a partial un-relaxed store
    refused(0.25, [0, 1])
    ctx.set_sequences(seqs)    # no un-relaxed store
    refused(0.25, [0])
    ctx.set_families([0, 4, 7])
    ctx.fold_posteriors(0.01)
    ctx.align_posteriors(fetch=False)
    ctx.consistency_match_pairs(0.25, [0, 8])  # and the context still works
    assert [int(v) for v in np.nonzero(ctx.mp(1).nnz)[0]] == [0, 8]
    ctx.close()
