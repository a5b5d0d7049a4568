"""Hand-made matching and base-pairing stores for the consistency transforms: inputs no model
makes, at the sizes where k_pct_rows / k_pct_bp_rows / k_mp_sim and consistency_parts take another path.  Plain numpy
with seeded generators, so the CPU test (test_pct_edges_cpu.py: every case does what it is for, on the oracle alone) and
the GPU test (test_pct_edges_gpu.py: the kernels against the oracle's phase 1) see the same bytes.

A case holds lens, seqs, names, mp(x, y) for x < y and bps (one CSR triple per sequence), and the weight triples
(w_a, w_s, w_f) it is run at.  Columns ascend within a row; base-pair columns are > row; values are irregular floats in
(0, 1], so that a wrong order of additions shows in the bits.  The transforms never read residues."""
import functools

import numpy as np

from test_cluster_structure_cpu import csr

W_DEFAULT = (0.25, 0.25, 0.0)
# negative weights (1 / N each), one transform off, and the four-way transform below the ordinary ones and on its own
W_ALL = [W_DEFAULT, (-1.0, -1.0, 0.0), (0.25, 0.0, 0.0), (0.0, 0.25, 0.0), (0.25, 0.25, 0.3), (0.0, 0.0, 0.3)]
WEIGHTS = {"long_rows": W_ALL, "chunks_17": W_ALL, "empty": [W_DEFAULT, (-1.0, -1.0, 0.0)]}  # every other case: W_DEFAULT


def _vals(rng, n):
    return (0.02 + 0.98 * rng.random(n)).astype(np.float32)


def mp_rows(rng, nrows, ncols, counts, force=None, avoid=()):
    """CSR with counts[i] entries in row i: random distinct columns, those of force.get(i, ()) among them; the columns of
    avoid only where forced"""
    rows = {}
    for i in range(nrows):
        must = sorted(set((force or {}).get(i, ())))
        c = max(int(counts[i]), len(must))
        free = np.setdiff1d(np.arange(ncols), must + list(avoid))
        cols = np.sort(np.concatenate([np.array(must, np.int64), rng.choice(free, c - len(must), replace=False)]))
        rows[i] = list(zip(cols.tolist(), _vals(rng, c).tolist()))
    return csr(nrows, rows)


def bp_rows(rng, L, counts, force=None):
    """upper-triangular CSR of one sequence: counts[i] partners j > i in row i, those of force.get(i, ()) among them"""
    rows = {}
    for i in range(L):
        must = sorted(set((force or {}).get(i, ())))
        c = max(min(int(counts.get(i, 0)), L - 1 - i), len(must))
        free = np.setdiff1d(np.arange(i + 1, L), must)
        cols = np.sort(np.concatenate([np.array(must, np.int64), rng.choice(free, c - len(must), replace=False)]))
        rows[i] = list(zip(cols.tolist(), _vals(rng, c).tolist()))
    return csr(L, rows)


class Case:
    def __init__(self, name, lens, mps, bps):
        self.name, self.lens, self.mps, self.bps, self.weights = name, tuple(lens), mps, bps, WEIGHTS.get(name, [W_DEFAULT])
        self.n = len(lens)
        self.names = ["s%d" % x for x in range(self.n)]
        self.seqs = [("ACGU" * (L // 4 + 1))[:L] for L in lens]
        self.pairs = [(x, y) for x in range(self.n) for y in range(x + 1, self.n)]
        assert set(mps) == set(self.pairs) and len(bps) == self.n

    def mp(self, x, y):
        return self.mps[(x, y)]

    def set_mp_args(self):
        """(nnz, rowptr, col, val) of every pair in row-major order: the layout of Context.set_mp"""
        m = [self.mps[p] for p in self.pairs]
        return (np.array([len(t[1]) for t in m], np.uint32), np.concatenate([t[0] for t in m]),
                np.concatenate([t[1] for t in m]), np.concatenate([t[2] for t in m]))

    def row_blocks(self):
        """workgroups of k_pct_rows that have rows: the tasks pct_task_order sorts (one per pair and block of 16 rows of x)"""
        return sum((self.lens[x] + 15) // 16 for x, _ in self.pairs)


def transposed_row_lengths(m, ncols):
    """entries per row of the transposed matrix: how many rows name each column"""
    return np.bincount(m[1].astype(np.int64), minlength=ncols)


def row_lengths(m):
    return np.diff(m[0].astype(np.int64))


@functools.lru_cache(maxsize=None)
def long_rows():
    """Rows longer than a 16-lane group, forward, transposed and base-pairing, beside short and empty rows of the same
    wavefront (output rows 4q .. 4q + 3): the scalar side path of pct_step::apply and pct_round::apply (with its jlo
    filter) and the e0 loop over a long bp[y][k] row."""
    rng = np.random.default_rng(1601)
    lens = (20, 40, 24)
    c01 = [40, 0, 1, 15, 16, 17, 0, 31, 32, 1, 33, 0, 17, 16, 15, 1, 33, 0, 40, 2]
    c02 = [0, 24, 1, 17, 3, 0, 16, 2, 17, 1, 0, 15, 2, 18, 0, 1, 16, 3, 0, 24]
    c12 = [3, 0, 17, 1, 2, 24, 0, 4, 3, 3, 0, 2, 16, 1, 5, 0, 3, 2, 4, 1, 0, 3, 18, 2, 3, 2, 1, 4, 2, 3, 1, 17, 3, 1, 2, 3, 5, 3, 2, 1]
    # transposed rows beyond a group in mp[2][1]: column 3 is named by exactly 33 rows of sequence 1 (two groups and one),
    # column 20 by exactly 17 (one group and one); row 5 holds every column
    nonempty = [i for i in range(40) if c12[i]]
    force12 = {i: [3] for i in nonempty[:33]}
    for i in [5] + nonempty[-16:]:
        force12.setdefault(i, []).append(20)
    mps = {(0, 1): mp_rows(rng, 20, 40, c01), (0, 2): mp_rows(rng, 20, 24, c02),
           (1, 2): mp_rows(rng, 40, 24, c12, force12, avoid=(3, 20))}
    bps = [bp_rows(rng, 20, {0: 16, 1: 17, 2: 1, 3: 0, 5: 2, 9: 1, 12: 3}),
           bp_rows(rng, 40, {0: 33, 1: 0, 2: 17, 3: 16, 4: 1, 5: 0, 6: 33, 7: 1, 11: 2, 20: 3, 30: 1}),
           bp_rows(rng, 24, {0: 17, 1: 16, 2: 0, 3: 1, 4: 17, 8: 2, 15: 1})]
    return Case("long_rows", lens, mps, bps)


def _family(name, rng, lens, p_empty_pair=0.1, p_empty_row=0.15):
    """about three entries per row, some rows empty, a few pairs empty entirely (similarity 0, hence weight 0)"""
    n = len(lens)
    mps = {}
    for x in range(n):
        for y in range(x + 1, n):
            if rng.random() < p_empty_pair:
                mps[(x, y)] = csr(lens[x], {})
                continue
            counts = [0 if rng.random() < p_empty_row else min(int(rng.integers(1, 6)), lens[y]) for _ in range(lens[x])]
            mps[(x, y)] = mp_rows(rng, lens[x], lens[y], counts)
    bps = [bp_rows(rng, L, {i: int(rng.integers(0, 3)) for i in range(L)}) for L in lens]
    return Case(name, lens, mps, bps)


@functools.lru_cache(maxsize=None)
def chunks(n):
    """One family of n sequences: the row kernels walk it in chunks of 16 (zc / yc, zoff, zabase, h.z = min(zc + zz, N - 1)).
    16: one full chunk; 17: the last sequence alone in its chunk; 33: two full chunks and one."""
    rng = np.random.default_rng(1700 + n)
    lens = [int(v) for v in rng.integers(9, 25, n)]
    return _family("chunks_%d" % n, rng, lens)


@functools.lru_cache(maxsize=None)
def lengths():
    """Row blocks of 16 with one active row, the 8-byte row-pointer load at row 0 of a one-residue sequence, L2 < 16."""
    rng = np.random.default_rng(1801)
    return _family("lengths", rng, (1, 2, 15, 16, 17, 31, 32, 33), p_empty_pair=0.0)


@functools.lru_cache(maxsize=None)
def empty():
    """Every matching matrix empty, the base-pairing stores not: every similarity is 0, so every weight of the matching
    transform and its sum_w are 0 and nothing is kept (0 / 0 is no v > CUTOFF).  The base-pairing transform keeps the
    weight of y == x (sim[x][x] = 1), so its result is the input's own pairs."""
    rng = np.random.default_rng(1901)
    lens = (12, 17, 9, 20)
    mps = {(x, y): csr(lens[x], {}) for x in range(4) for y in range(x + 1, 4)}
    bps = [bp_rows(rng, L, {i: int(rng.integers(0, 3)) for i in range(L)}) for L in lens]
    return Case("empty", lens, mps, bps)


@functools.lru_cache(maxsize=None)
def wide(L, name=None):
    """Accumulator rows beyond 64 KiB of LDS: the long sequence comes last, so it is the column side of two pairs and its
    own base-pair tile is L wide.  Entries in columns 0, 1, L - 2 and L - 1; base pairs (0, L - 1) and (L - 3, L - 2)."""
    rng = np.random.default_rng(2000 + L)
    lens = (40, 33, L)
    three = lambda n: [int(rng.integers(2, 5)) for _ in range(n)]
    mps = {(0, 1): mp_rows(rng, 40, 33, three(40)),
           (0, 2): mp_rows(rng, 40, L, three(40), {0: [0, 1], 20: [0, L - 1], 39: [L - 2, L - 1]}),
           (1, 2): mp_rows(rng, 33, L, three(33), {0: [0, 1], 16: [1, L - 2], 32: [L - 2, L - 1]})}
    sparse = {int(i): 1 for i in rng.choice(L - 4, 300, replace=False)}
    bps = [bp_rows(rng, 40, {i: int(rng.integers(0, 3)) for i in range(40)}),
           bp_rows(rng, 33, {i: int(rng.integers(0, 3)) for i in range(33)}),
           bp_rows(rng, L, sparse, {0: [L - 1], L - 3: [L - 2]})]
    return Case(name or "wide_%d" % L, lens, mps, bps)


# Longest sequence of a family of three that the row kernels' LDS takes (pct_match_launch / pct_bp_launch in pct.hip):
#   k_pct_rows     3 * 32 + 4 * 4 + 16 * (row_cap + 16 + 68) * 4 + 64 = 5552 + 64 row_cap <= 150 KiB = 153600, so
#                  row_cap <= 2313, and row_cap is max_len rounded up to 28 (mod 32): 2300 fits, 2301 gives 2332;
#   k_pct_bp_rows  3 * 32 + 4 * 4 + 16 * (4 row_cap + 128 + 80 + 64) + 64 = 4528 + 64 row_cap, so row_cap <= 2329, and
#                  row_cap is max_len rounded up to 12 (mod 32): 2316 fits, 2317 gives 2348.
MATCH_TOP, BP_TOP = 2300, 2316


def wide_1000():
    return wide(1000)


def wide_top():
    return wide(MATCH_TOP, "wide_top")


@functools.lru_cache(maxsize=None)
def overflow():
    """A star: mp[0][y] is dense, every other pair empty.  Every output pair is dense (through z = 0) and every sequence's
    base-pairing result is its whole upper triangle, so both output pools outgrow consistency_parts' first guess and both
    transforms take the retry."""
    rng = np.random.default_rng(2101)
    n, L = 6, 40
    mps = {}
    for x in range(n):
        for y in range(x + 1, n):
            if x:
                mps[(x, y)] = csr(L, {})
                continue
            v = (0.5 + 0.1 * (rng.random((L, L)) - 0.5)).astype(np.float32)
            mps[(x, y)] = (np.arange(L + 1, dtype=np.uint32) * L, np.tile(np.arange(L, dtype=np.uint32), L), v.ravel())
    bps = [bp_rows(rng, L, {int(i): 1 for i in rng.choice(L - 1, 2, replace=False)}) for _ in range(n)]
    return Case("overflow", (L,) * n, mps, bps)


ALL = [long_rows, lambda: chunks(16), lambda: chunks(17), lambda: chunks(33), lengths, empty, wide_1000, wide_top, overflow]
IDS = ["long_rows", "chunks_16", "chunks_17", "chunks_33", "lengths", "empty", "wide_1000", "wide_top", "overflow"]
RUNS = [(name, make, w) for name, make in zip(IDS, ALL) for w in WEIGHTS.get(name, [W_DEFAULT])]  # what the GPU test runs


class Reference:
    """what the oracle's phase 1 leaves: sim, the rows of mp[a][b] for every a != b, the rows of bp[x]"""

    def __init__(self, pl, n):
        self.sim = pl.sim()
        self.mp = {(a, b): pl.mp(a, b) for a in range(n) for b in range(n) if a != b}
        self.bp = [pl.bp(x) for x in range(n)]


_REFERENCES = {}


def reference(oracle, case, w_a=0.25, w_s=0.25, w_f=0.0):
    """the oracle's phase 1 on the case's stores (align_model=2, fold_model=1), computed once per case and weights"""
    key = (case.name, case.lens, w_a, w_s, w_f)
    if key not in _REFERENCES:
        pl = oracle.pipeline(case.names, case.seqs, oracle.params(align_model=2, fold_model=1, w_pct_a=w_a, w_pct_s=w_s, w_pct_f=w_f),
                             bp=case.bps, mp=case.mp)
        pl.phase1()
        _REFERENCES[key] = Reference(pl, case.n)
        pl.close()
    return _REFERENCES[key]
