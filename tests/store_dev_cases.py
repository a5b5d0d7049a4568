"""Inputs and the numpy reference for the device store exchange (capi_dev.cpp, store_dev.hip) and the sharded phase 1
(capi_shard.cpp); DESIGN.md section 8.  Plain numpy with seeded generators, so that the CPU test (test_store_dev_cpu.py:
the reference and the cases do what they are for) and the GPU tests (test_store_dev_gpu.py, test_shard_worlds_gpu.py) see
the same bytes.

The reference of a device export is the context's own host fetch of the same store (Context.mp, Context.bp), cut here:
slice_mp gives the pairs [first, first + count) of a PairPosteriors in the layout of dafs_hip_mp_fetch, slice_bp the
base-pairing rows of the sequences in a given block order.  Nothing here does arithmetic on a probability."""
import functools

import numpy as np

import pct_cases as pc
from test_cluster_structure_cpu import csr

WORLDS = (1, 2, 3, 5)  # and npairs, npairs + 3: see splits()


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def _u32(parts):
    return np.concatenate([np.asarray(a, np.uint32) for a in parts]) if parts else np.zeros(0, np.uint32)


def _f32(parts):
    return np.concatenate([np.asarray(a, np.float32) for a in parts]) if parts else np.zeros(0, np.float32)


def slice_mp(pp, lens, first, count):
    """(nnz, rowptr, col, val) of the pairs [first, first + count) of the PairPosteriors pp, whose sequences have the
    lengths lens, in the fetch layout: per pair len_x + 1 relative row pointers of mp[x][y], then len_y + 1 of mp[y][x];
    per pair nnz entries of mp[x][y], then nnz of the transpose."""
    assert 0 <= first and 0 <= count and first + count <= len(pp)
    rps, cols, vals = [], [], []
    for p in range(first, first + count):
        x, y, k = int(pp.pair_x[p]), int(pp.pair_y[p]), int(pp.nnz[p])
        for transposed, L in ((False, int(lens[x])), (True, int(lens[y]))):
            rp, col, val = pp.csr(p, transposed)
            assert len(rp) == L + 1 and len(col) == len(val) == k
            rps.append(rp); cols.append(col); vals.append(val)
    return np.asarray(pp.nnz[first:first + count], np.uint32).copy(), _u32(rps), _u32(cols), _f32(vals)


def sim_by_pair(sim, n):
    """the upper triangle of the n x n similarity matrix in pair order"""
    ii, jj = np.triu_indices(n, k=1)
    return np.ascontiguousarray(np.asarray(sim, np.float32).reshape(n, n)[ii, jj])


def slice_bp(rows, order):
    """(rowptr, col, val): the blocks of the sequences order[0], order[1], ... one after another, every block with its own
    relative row pointers -- the layout of dafs_hip_bp_fetch for the identity, of the gathered exports otherwise"""
    return _u32([rows[x][0] for x in order]), _u32([rows[x][1] for x in order]), _f32([rows[x][2] for x in order])


def unslice_bp(lens, order, rowptr, col, val):
    """the inverse of slice_bp: the rows of every sequence from blocks in the order `order`"""
    rows = [None] * len(lens)
    r0 = e0 = 0
    for x in order:
        rp = rowptr[r0:r0 + int(lens[x]) + 1]
        k = int(rp[-1])
        rows[x] = (rp, col[e0:e0 + k], val[e0:e0 + k])
        r0 += int(lens[x]) + 1
        e0 += k
    assert r0 == len(rowptr) and e0 == len(col) == len(val)
    return rows


def same_rows(a, b):
    return len(a) == len(b) and all(u.tobytes() == v.tobytes() and u.dtype == v.dtype for s, t in zip(a, b) for u, v in zip(s, t))


def world_split(npairs, world):
    """[(first, count)] of the ranks of a world: dafs_hip_pair_range"""
    edge = [npairs * r // world for r in range(world + 1)]
    return [(edge[r], edge[r + 1] - edge[r]) for r in range(world)]


def splits(npairs):
    """The ways the pair range [0, npairs) is cut for the exports: a list of splits, each a list of (first, count) that
    cover the range in order.  The whole; the edges (0, 0), (0, 1), (npairs - 1, 1), (npairs, 0) around the middle; every
    single pair where there are at most 40; the ranks' ranges for worlds 1, 2, 3, 5, npairs and npairs + 3."""
    assert npairs >= 1
    edges = [(0, 0), (0, 1)] + ([(1, npairs - 2)] if npairs > 2 else []) + ([(npairs - 1, 1)] if npairs > 1 else []) + [(npairs, 0)]
    out = [[(0, npairs)], edges]
    if npairs <= 40:
        out.append([(p, 1) for p in range(npairs)])
    for w in WORLDS + (npairs, npairs + 3):
        out.append(world_split(npairs, w))
    return out


def ranges(npairs, extra=()):
    """every distinct range of splits(npairs), and of extra, in first-seen order"""
    seen = []
    for r in [r for s in splits(npairs) for r in s] + list(extra):
        if r not in seen:
            seen.append(r)
    return seen


def block_orders(n, seed=7):
    """{name: order} of set_bp_dev's blocks: the identity, reversed, what the ranks of a world w leave after the gather
    (rank r folds x = r mod w) for w = 2, 3 and n + 2 (more ranks than sequences: the identity again, through the empty
    ranks), and a seeded shuffle"""
    out = {"identity": list(range(n)), "reversed": list(range(n - 1, -1, -1))}
    for w in (2, 3, n + 2):
        out["world_%s" % ("n+2" if w == n + 2 else w)] = [x for r in range(w) for x in range(r, n, w)]
    out["shuffle"] = [int(x) for x in np.random.default_rng(seed + n).permutation(n)]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# hand-made matching stores
# ---------------------------------------------------------------------------------------------------------------------
def _transpose(m, ncols):
    """CSR of the transposed matrix: rows keyed by column, the original rows ascending within each (transpose_mp)"""
    rp, col, val = m
    rows = np.repeat(np.arange(len(rp) - 1, dtype=np.uint32), np.diff(rp.astype(np.int64)))
    order = np.lexsort((rows, col))
    trp = np.concatenate([[0], np.cumsum(np.bincount(col.astype(np.int64), minlength=ncols))]).astype(np.uint32)
    return trp, rows[order], val[order]


def case_pp(case):
    """the un-relaxed store Context.set_mp makes of a case, as Context.mp(0) returns it -- worked out on the host"""
    from dafs_amd import capi
    lens = np.array(case.lens, np.uint32)
    rps, cols, vals = [], [], []
    for x, y in case.pairs:
        m = case.mps[(x, y)]
        t = _transpose(m, case.lens[y])
        rps += [m[0], t[0]]; cols += [m[1], t[1]]; vals += [m[2], t[2]]
    px = np.array([p[0] for p in case.pairs], np.uint32)
    py = np.array([p[1] for p in case.pairs], np.uint32)
    nnz = np.array([len(case.mps[p][1]) for p in case.pairs], np.uint32)
    return capi.PairPosteriors(px, py, None, nnz, _u32(rps), _u32(cols), _f32(vals), lens)


MANY_EMPTY, MANY_FULL = (0, 1023, 1024, 1080), (1,)


@functools.lru_cache(maxsize=None)
def many_pairs():
    """47 sequences of 1 to 6 residues: 1081 pairs, more than the 1024 threads of k_scan_excl, so that a thread scans a
    chunk of two and the last threads none.  About three entries per pair, a fifth of the pairs empty; the pairs at the
    ends of the store and on both sides of thread 511 / 512's chunks (0, 1023, 1024, 1080) are empty, pair 1 is not."""
    rng = np.random.default_rng(4701)
    lens = [int(v) for v in rng.integers(1, 7, 47)]
    n = len(lens)
    mps, p = {}, 0
    for x in range(n):
        for y in range(x + 1, n):
            cells = lens[x] * lens[y]
            k = 0 if p in MANY_EMPTY or (p not in MANY_FULL and rng.random() < 0.2) else min(int(rng.integers(1, 6)), cells)
            pick = np.sort(rng.choice(cells, k, replace=False))
            vals = pc._vals(rng, k)
            rows = {}
            for c, v in zip(pick.tolist(), vals.tolist()):
                rows.setdefault(c // lens[y], []).append((c % lens[y], v))
            mps[(x, y)] = csr(lens[x], rows)
            p += 1
    bps = [pc.bp_rows(rng, L, {i: int(rng.integers(0, 3)) for i in range(L)}) for L in lens]
    return pc.Case("many_pairs", lens, mps, bps)


MANY_EXTRA = ((0, 1023), (0, 1024), (0, 1025), (56, 1025))  # a scan of 1024 threads over 1023, 1024 and 1025 counts


@functools.lru_cache(maxsize=None)
def two():
    """two sequences, one pair: k_sim_matrix's diagonal loop (n = 2) outruns its pair loop (np = 1)"""
    rng = np.random.default_rng(4702)
    return pc._family("two", rng, (7, 12), p_empty_pair=0.0)


HAND = {"lengths": pc.lengths, "empty": pc.empty, "chunks_17": lambda: pc.chunks(17), "many_pairs": many_pairs, "two": two}


# ---------------------------------------------------------------------------------------------------------------------
# base-pairing stores without a matching store: more sequences than k_scan_excl has threads
# ---------------------------------------------------------------------------------------------------------------------
BP_ONLY = (1023, 1024, 1025, 2049)


class BpCase:
    def __init__(self, n, lens, rows):
        self.n, self.lens, self.bps = n, tuple(lens), rows
        self.seqs = [("ACGU" * 2)[:L] for L in lens]


@functools.lru_cache(maxsize=None)
def bp_only(n):
    """n sequences of 1 to 4 residues with zero to three base pairs each (as many as i < j leaves room for); sequence 0
    and sequence n - 1 have none.  1023, 1024, 1025: one short of, exactly and one more than k_scan_excl's threads; 2049:
    chunks of three, the last threads idle."""
    rng = np.random.default_rng(4800 + n)
    lens = [int(v) for v in rng.integers(1, 5, n)]
    rows = []
    for x, L in enumerate(lens):
        cells = [(i, j) for i in range(L) for j in range(i + 1, L)]
        k = 0 if x in (0, n - 1) else min(int(rng.integers(0, 4)), len(cells))
        pick = sorted(int(c) for c in rng.choice(len(cells), k, replace=False))
        vals = pc._vals(rng, k)
        r = {}
        for c, v in zip(pick, vals.tolist()):
            r.setdefault(cells[c][0], []).append((cells[c][1], v))
        rows.append(csr(L, r))
    return BpCase(n, lens, rows)


# ---------------------------------------------------------------------------------------------------------------------
# computed inputs
# ---------------------------------------------------------------------------------------------------------------------
def _records(recs, prefix=""):
    return [prefix + r[0] for r in recs], [r[1] for r in recs]


@functools.lru_cache(maxsize=None)
def computed():
    """(names, seqs): a family of six around 40 residues and sequences of 1, 2 and 97: the pairs' costs differ by four
    orders of magnitude, so the pair kernels' bump-allocated pools are unlikely to lie in pair order"""
    from dafs_amd import synth
    names, seqs = _records(synth.family_set(6, 40, seed=3))
    for L in (1, 2, 97):
        nm, sq = _records(synth.random_set(1, L, seed=300 + L, jitter=0), "r%d_" % L)
        names += nm; seqs += sq
    return tuple(names), tuple(seqs)


@functools.lru_cache(maxsize=None)
def two_seqs():
    """lengths 1 and 30: one pair; from world 2 on a rank has no pair, from world 3 on one has no sequence to fold, and
    at world 4 rank 2 has neither"""
    from dafs_amd import synth
    return ("a", "b"), ("G", synth.random_set(1, 30, seed=31, jitter=0)[0][1])


@functools.lru_cache(maxsize=None)
def five_seqs():
    """five sequences of 1 to 80 residues: 10 pairs"""
    from dafs_amd import synth
    names, seqs = [], []
    for L in (80, 1, 33, 2, 17):
        nm, sq = _records(synth.random_set(1, L, seed=500 + L, jitter=0), "m%d_" % L)
        names += nm; seqs += sq
    return tuple(names), tuple(seqs)


# The sharded phase (test_shard_worlds_gpu.py): name -> (input, worlds, options of the phase).  align: the align model;
# the defaults are those of pipeline.run (th_a 0.01, both weights 0.25, fold_th 0.01).
def shard_runs():
    out = {}
    for w in (1, 2, 3, 4):
        out["two-world_%d" % w] = (two_seqs, w, {})
    for w in (4, 7, 10):
        for model in (0, 1):
            out["five-world_%d-model_%d" % (w, model)] = (five_seqs, w, {"align": model})
    out["computed-world_2"] = (computed, 2, {})
    out["computed-world_5"] = (computed, 5, {})
    out["computed-world_2-no_match_transform"] = (computed, 2, {"w_pct_a": 0.0})
    out["computed-world_2-no_bp_transform"] = (computed, 2, {"w_pct_s": 0.0})
    out["computed-world_3-fold_th_2"] = (computed, 3, {"fold_th": 2.0})
    out["computed-world_3-th_a_2"] = (computed, 3, {"th_a": 2.0})
    return out
