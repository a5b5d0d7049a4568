"""Cases, float32 restatements and comparison of the node set-up tests (test_node_setup_cpu.py, test_node_setup_gpu.py):
what k_node_avg, k_node_lists (or k_lists_rows / k_lists_scan / k_node_lists_tail) and k_node_cbp_fill write for a node,
fetched with Context.node_peek, against orc_pipeline_node_setup on the same hand-made stores.  Built on dd_nodes_ref.Case
and open_context; no model kernel runs.  Test infrastructure only -- nothing under dafs_amd/ imports this."""
import numpy as np

import dd_nodes_ref as R

CUT = np.float32(0.01)     # CUTOFF: cells at or below it become 0
AVG_STAGE = 1024           # dd.hip: addends a wavefront parks per round
F32 = np.float32


def _ulps(v, k):
    """the float32 k representable steps above (k > 0) or below v"""
    v = F32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, F32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return v


class PairStore(dict):
    """mp[(x, y)], x < y: the pairs that were set, and rows without entries for every other pair"""

    def __init__(self, lens):
        super().__init__()
        self.lens = lens

    def __missing__(self, key):
        return np.zeros(self.lens[key[0]] + 1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32)


def _csr(rows):
    """rows: per row a list of (column, value), any order -> (rowptr, col, val) with ascending columns"""
    return R._csr([sorted(r) for r in rows])


def _mask(rng, lens, L, lone=()):
    """rows of lens[r] residues over L columns; lone = ((column, row), ...): only that row has a residue in that column, so
    every other source of the column is a gap"""
    free = np.array([c for c in range(L) if c not in {c for c, _ in lone}])
    m = np.zeros((len(lens), L), np.uint8)
    for r, n in enumerate(lens):
        mine = [c for c, row in lone if row == r]
        m[r, mine] = 1
        m[r, rng.choice(free, n - len(mine), replace=False)] = 1
    return m


def _bp(rng, L, per_row):
    """a sequence's base-pairing rows: per_row[i] (or a number for all) partners j > i of residue i, continuous values in (0.02, 1)"""
    rows = []
    for i in range(L):
        k = min(int(per_row[i] if hasattr(per_row, "__len__") else per_row), L - 1 - i)
        js = rng.choice(np.arange(i + 1, L), k, replace=False) if k else []
        rows.append([(int(j), F32(0.02 + 0.98 * rng.random())) for j in js])
    return _csr(rows)


def _mp(rng, La, Lb, width, dense_rows=()):
    """matching rows of a pair: per residue of a, `width` columns around the scaled diagonal (all columns in dense_rows),
    continuous values in (0.02, 1)"""
    rows = []
    for i in range(La):
        c = i * Lb // La
        js = range(Lb) if i in dense_rows else range(max(0, c - width // 2), min(Lb, c - width // 2 + width))
        rows.append([(j, F32(0.02 + 0.98 * rng.random())) for j in js])
    return _csr(rows)


def _seqs(rng, lens):
    return R._sequences(rng, lens)


def rows_case(key, n1, n2, L1, L2, lone1=(), lone2=(), lens=None, bp_per_row=3, mp_width=3, dense_rows1=(), seed=0):
    """children of n1 and n2 gapped rows over L1 and L2 columns, sequences of 12 .. 30 residues (lens: given lengths); child 1
    holds sequences 0 .. n1 - 1.  dense_rows1: rows of child 1 whose matching rows against child 2 hold every column."""
    rng = np.random.default_rng(R._seed(77, n1, n2, L1, L2, seed))
    if lens is None:
        lens = [int(rng.integers(max(12, min(L, 30) - 6), min(L - len(lone), 30) + 1)) for L, n, lone in ((L1, n1, lone1), (L2, n2, lone2)) for _ in range(n)]
    bp = [_bp(rng, n, bp_per_row) for n in lens]
    mp = PairStore(lens)
    for a in range(n1):
        for b in range(n1, n1 + n2):
            mp[(a, b)] = _mp(rng, lens[a], lens[b], mp_width, range(lens[a]) if a in dense_rows1 else ())
    node = (np.arange(n1, dtype=np.uint32), _mask(rng, lens[:n1], L1, lone1), np.arange(n1, n1 + n2, dtype=np.uint32), _mask(rng, lens[n1:], L2, lone2))
    return R.Case(key, _seqs(rng, lens), bp, mp, [node], 1)


# ---- A: sources per row of p_x / p_y ----
A_ROWS = (1, 2, 63, 64, 65, 130)


def case_a(n, side):
    """one child of n gapped rows over 32 columns (side 0: the first child, averaged into p_x; 1: the second, p_y), the other a
    single row.  Columns 0 and 1 hold a residue of one row only, rows in the middle of a batch of 64 sources."""
    lone = ((0, n // 2), (1, (n * 3) // 4)) if n > 2 else ()
    if side == 0:
        return rows_case(("A", n, 0), n, 1, 32, 30, lone1=lone)
    return rows_case(("A", n, 1), 1, n, 30, 32, lone2=lone)


# ---- B: the cooperative form of k_node_avg ----
B_SHAPES = ((23, 23), (2, 256), (300, 2))


def _exact_quotient(n, want):
    """a float32 v with v / float32(n) == want in float32, or None"""
    d = F32(n)
    v0 = F32(want * d)
    for k in range(-8, 9):
        v = _ulps(v0, k)
        if F32(v / d) == want:
            return v
    return None


def case_b(n1, n2, dense=False):
    """n1 x n2 sources per row of p_z over 32 x 32 columns.  Column 0 of the second child holds a residue of one row only, and
    the first row of the first child matches it with the one value whose share is exactly the cut-off: a cell of p_z that the
    cut must clear.  dense (the staging case C): the matching rows of child 1's first three rows hold every column."""
    lone2 = ((0, n2 // 2),)
    c = rows_case(("B", n1, n2, dense), n1, n2, 32, 32, lone2=lone2, dense_rows1=(0, 1, 2) if dense else (),
                  lens=None if not dense else _dense_lens(n1, n2))
    v = _exact_quotient(n1 * n2, CUT)
    assert v is not None
    m1, lone = c.nodes[0][1], n1 + n2 // 2
    i0 = int(np.nonzero(m1[0])[0][0])                      # alignment column of residue 0 of the first row
    for r1 in range(n1):                                   # residue 0 of the lone row is the one in column 0 of the second child
        rp, col, val = c.mp[(r1, lone)]
        rows = [[(int(col[e]), val[e]) for e in range(rp[i], rp[i + 1]) if col[e] != 0] for i in range(len(rp) - 1)]
        if r1 == 0:
            rows[0].append((0, v))
        c.mp[(r1, lone)] = _csr(rows)
    c.cut_cell = (i0, 0)
    return c


def _dense_lens(n1, n2):
    rng = np.random.default_rng(R._seed(78, n1, n2))
    return [int(rng.integers(12, 31)) for _ in range(n1)] + [int(rng.integers(26, 31)) for _ in range(n2)]


# ---- C: the staging area ----
# addends per source (lane) of the four columns of case_c_split: where the running total passes AVG_STAGE
C_SPLIT_COUNTS = {
    0: [1000, 25] + [16] * 62,                   # 1000 + 25 > 1024: the batch splits after lane 0; the rest (1017) fits
    1: [16] * 63 + [17],                         # 1008, then 1025: it splits before lane 63
    2: [500] + [27] * 19 + [11] + [17] * 43,     # exactly 1024 at lane 20, which still fits
    3: [500] + [26] * 20 + [5] + [17] * 42,      # 1025 at lane 21: one entry more does not
}
C_SPLIT_PASSES = {0: [(0, 1), (1, 64)], 1: [(0, 63), (63, 64)], 2: [(0, 21), (21, 64)], 3: [(0, 21), (21, 64)]}


def passes_of(counts):
    """avg_row's rule on one batch of at most 64 sources: [first, last) of every pass -- as many lanes in order as fit
    AVG_STAGE addends together, a lane that alone exceeds it on its own"""
    out, first = [], 0
    while first < len(counts):
        last, total = first, 0
        while last < len(counts) and total + counts[last] <= AVG_STAGE:
            total += counts[last]; last += 1
        if last == first:
            last = first + 1
        out.append((first, last))
        first = last
    return out


def case_c_split():
    """64 rows in the first child; sequence 0 has 1030 residues (the only way two lanes pass 1024 addends together), the others
    30, all without gaps in columns 0 .. 29.  The base-pairing rows 0 .. 3 carry C_SPLIT_COUNTS entries."""
    rng = np.random.default_rng(R._seed(79))
    lens = [1030] + [30] * 63 + [30]
    bp = []
    for s, n in enumerate(lens):
        per_row = [3] * n
        if s < 64:
            for i in range(4):
                per_row[i] = C_SPLIT_COUNTS[i][s]
        bp.append(_bp(rng, n, per_row))
    mp = PairStore(lens)
    for a in range(64):
        mp[(a, 64)] = _mp(rng, lens[a], 30, 3)
    m1 = np.zeros((64, 1030), np.uint8)
    m1[0, :] = 1
    m1[1:, :30] = 1
    node = (np.arange(64, dtype=np.uint32), m1, np.array([64], np.uint32), np.ones((1, 30), np.uint8))
    return R.Case(("C", "split"), _seqs(rng, lens), bp, mp, [node], 1)


def case_c_rounds():
    """(23, 23): round 0 of a row of p_z does not fit its staging areas, rounds 1 and 2 do"""
    c = case_b(23, 23, True)
    c.key = ("C", "rounds")
    return c


C_LONG = 1100


def case_c_long():
    """two single rows of 1100 residues; base-pairing row 0 and matching row 0 hold about 1060 entries each: one source that
    alone exceeds the staging area, for p_x and for p_z.  Opened and peeked, never iterated."""
    rng = np.random.default_rng(R._seed(80))
    bp, mp0 = R.stores(rng, [C_LONG, C_LONG], False, 1.2, 0.6)
    mp = PairStore([C_LONG, C_LONG])
    mp[(0, 1)] = mp0[(0, 1)]

    def with_row0(store, cols):
        rp, col, val = store
        rows = [[(int(col[e]), val[e]) for e in range(rp[i], rp[i + 1])] for i in range(len(rp) - 1)]
        rows[0] = [(int(j), F32(0.02 + 0.2 * rng.random())) for j in cols]
        return _csr(rows)
    bp[0] = with_row0(bp[0], rng.choice(np.arange(1, C_LONG), 1060, replace=False))
    mp[(0, 1)] = with_row0(mp[(0, 1)], rng.choice(np.arange(0, C_LONG), 1060, replace=False))
    node = (np.array([0], np.uint32), np.ones((1, C_LONG), np.uint8), np.array([1], np.uint32), np.ones((1, C_LONG), np.uint8))
    return R.Case(("C", "long"), _seqs(rng, [C_LONG, C_LONG]), bp, mp, [node], 1)


# ---- D: the cuts ----
# name -> (stored values of the sources, the cell's value after the cuts): one source at n = 1, two at n = 2
def cut_values(n):
    two_c = F32(2) * CUT
    a = F32(0.015)
    b = F32(two_c - a)      # exact (Sterbenz): a / 2 + b / 2 == CUT without a rounding
    low = {1: {"at the cut-off": ([CUT], F32(0)), "one ulp above it": ([_ulps(CUT, 1)], _ulps(CUT, 1)), "one ulp below it": ([_ulps(CUT, -1)], F32(0))},
           2: {"at the cut-off": ([a, b], F32(0)), "one ulp above it": ([_ulps(a, 2), b], _ulps(CUT, 1)), "one ulp below it": ([_ulps(a, -2), b], F32(0))}}[n]
    one = F32(1)
    high = {1: {"above one": ([F32(1.5)], one), "one ulp above one": ([_ulps(one, 1)], one), "at one": ([one], one), "one ulp below one": ([_ulps(one, -1)], _ulps(one, -1))},
            2: {"above one": ([F32(1.5), one], one), "one ulp above one": ([_ulps(one, 2), one], one), "at one": ([one, one], one),
                "one ulp below one": ([_ulps(one, -2), one], _ulps(one, -1))}}[n]
    return low, high


def case_d(n):
    """n rows in the first child, one in the second, 16 residues each and no gap.  Residue pair (i, i + 5) of the base-pairing
    rows and cell (i, i) of the matching rows carry the values of cut_values(n), in the order of its names: the low ones in
    p_x and p_z, the high ones in p_z only (p_x has no upper cut).  c.cells: matrix -> [(name, i, j, value after the cuts)]."""
    L = 16
    lens = [L] * (n + 1)
    low, high = cut_values(n)
    bp_rows = [[[] for _ in range(L)] for _ in range(n + 1)]
    mp_rows = [[[] for _ in range(L)] for _ in range(n)]
    cells = {"p_x": [], "p_z": []}
    for i, (name, (vals, want)) in enumerate(low.items()):
        for s in range(n):
            bp_rows[s][i].append((i + 5, vals[s]))
            mp_rows[s][i].append((i, vals[s]))
        cells["p_x"].append((name, i, i + 5, want))
        cells["p_z"].append((name, i, i, want))
    for i, (name, (vals, want)) in enumerate(high.items(), start=len(low)):
        for s in range(n):
            mp_rows[s][i].append((i, vals[s]))
        cells["p_z"].append((name, i, i, want))
    for s in range(n):                              # something plain beside them
        bp_rows[s][10].append((15, F32(0.5)))
        mp_rows[s][12].append((12, F32(0.5)))
    bp_rows[n][10].append((15, F32(0.5)))
    mp = PairStore(lens)
    for s in range(n):
        mp[(s, n)] = _csr(mp_rows[s])
    rng = np.random.default_rng(R._seed(81, n))
    node = (np.arange(n, dtype=np.uint32), np.ones((n, L), np.uint8), np.array([n], np.uint32), np.ones((1, L), np.uint8))
    c = R.Case(("D", n), _seqs(rng, lens), [_csr(r) for r in bp_rows], mp, [node], 1)
    c.cells = cells
    return c


# ---- E: lists, envelope, consensus pairs ----
E_SHAPES = R.TABLE
E_HAND = (65, 257)
# name -> environment of the form; None = the default (four workgroups per node, row pointers in LDS)
E_FORMS = {"default": None, "lists1": "DAFS_HIP_DD_LISTS1=1", "wide": "DAFS_HIP_DD_WIDE=1", "lists_wide": "DAFS_HIP_DD_LISTS_WIDE=1"}
SETUP_SWITCHES = ("DAFS_HIP_AVG_COOP0", "DAFS_HIP_DD_LISTS1", "DAFS_HIP_DD_LISTS_WIDE")


def case_e_hand(L):
    """single rows of L residues with hand-made matrices: p_x / p_y supplied with the node, p_z from the matching rows.  Each has
    empty rows, a row kept whole (small values, so that it adds few consensus pairs), a kept cell in the last column, kept
    cells at j = i + 1 (p_x, p_y) and on the diagonal (p_z), and cells at the cut-off itself, which are not kept.  The strong
    pairs (i, j) sit in both foldings and on the diagonal of p_z: consensus pairs."""
    rng = np.random.default_rng(R._seed(82, L))
    ps = []
    for side in range(2):
        p = np.zeros((L, L), np.float32)
        whole = 3 + side
        p[whole, whole + 1:] = (0.02 + 0.05 * rng.random(L - whole - 1)).astype(np.float32)
        for i in range(10, L - 6, 7):
            p[i, i + 1] = F32(0.3 + 0.6 * rng.random())      # j = i + 1
            p[i, L - 1] = F32(0.3 + 0.6 * rng.random())      # the last column
            p[i + 1, i + 5] = F32(0.3 + 0.6 * rng.random())
            p[i + 2, i + 4] = CUT                            # not kept
        p[L - 2, L - 1] = F32(0.7)                           # the last cell of the upper triangle
        p[0, :] = 0                                          # empty rows: the first, the last, and one inside
        p[20, :] = 0
        ps.append(p)
    z = np.zeros((L, L), np.float32)
    z[np.arange(L), np.arange(L)] = (0.3 + 0.7 * rng.random(L)).astype(np.float32)
    z[5, :] = (0.02 + 0.05 * rng.random(L)).astype(np.float32)   # a row kept whole
    z[7, :] = 0                                                   # empty rows
    z[L - 1, :] = 0
    z[8, L - 1] = F32(0.4)                                        # the last column
    z[9, 0] = F32(0.4)
    z[30, 30] = CUT
    rows = [[(int(j), z[i, j]) for j in np.nonzero(z[i])[0]] for i in range(L)]
    mp = PairStore([L, L])
    mp[(0, 1)] = _csr(rows)
    empty = _csr([[] for _ in range(L)])
    node = (np.array([0], np.uint32), np.ones((1, L), np.uint8), np.array([1], np.uint32), np.ones((1, L), np.uint8), ps[0], ps[1])
    return R.Case(("E", "hand", L), _seqs(rng, [L, L]), [empty, empty], mp, [node], 25)


# ---- float32 restatements of the averages, source by source ----
def _sources_bp(case, side, node=0):
    """per source (row of the child) of p_x / p_y: (rows, cols, values) of its addends in alignment columns, before the division"""
    n = case.nodes[node]
    seq, mask = n[2 * side], np.asarray(n[2 * side + 1])
    out = []
    for r, s in enumerate(seq):
        idx = np.nonzero(mask[r])[0]
        rp, col, val = case.bp[int(s)]
        rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp.astype(np.int64)))
        out.append((idx[rows], idx[col], np.asarray(val, np.float32)))
    return out


def _sources_mp(case, node=0):
    """per source (pair of rows, the first child's row major) of p_z"""
    n = case.nodes[node]
    out = []
    for r1, s1 in enumerate(n[0]):
        i1 = np.nonzero(np.asarray(n[1])[r1])[0]
        for r2, s2 in enumerate(n[2]):
            i2 = np.nonzero(np.asarray(n[3])[r2])[0]
            rp, col, val = case.mp[(int(s1), int(s2))]
            rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp.astype(np.int64)))
            out.append((i1[rows], i2[col], np.asarray(val, np.float32)))
    return out


def sources(case, which, node=0):
    return _sources_mp(case, node) if which == "p_z" else _sources_bp(case, 0 if which == "p_x" else 1, node)


def average(case, which, node=0, reverse=False):
    """p_x / p_y / p_z of the node summed in float32 source by source (a source adds to a cell at most once), in the
    reference's order or in the reversed one, then cut as the reference cuts"""
    n = case.nodes[node]
    L1, L2 = np.asarray(n[1]).shape[1], np.asarray(n[3]).shape[1]
    shape = {"p_x": (L1, L1), "p_y": (L2, L2), "p_z": (L1, L2)}[which]
    src = sources(case, which, node)
    d = F32(len(src))
    p = np.zeros(shape, np.float32)
    for rows, cols, val in (src[::-1] if reverse else src):
        p[rows, cols] += val / d
    if which == "p_z":
        p[p <= CUT] = 0
        p[p > F32(1)] = 1
    else:
        up = np.triu(np.ones(shape, bool), 1)
        p[up & (p <= CUT)] = 0
    return p


def addends_per_source(case, which, node=0):
    """[row of the matrix, source] -> addends that source brings to that row"""
    src = sources(case, which, node)
    n = case.nodes[node]
    R_ = np.asarray(n[1]).shape[1] if which != "p_y" else np.asarray(n[3]).shape[1]
    out = np.zeros((R_, len(src)), np.int64)
    for k, (rows, _, _) in enumerate(src):
        out[:, k] = np.bincount(rows, minlength=R_)
    return out


def most_addends_in_a_cell(case, which, node=0):
    n = case.nodes[node]
    L1, L2 = np.asarray(n[1]).shape[1], np.asarray(n[3]).shape[1]
    cnt = np.zeros({"p_x": (L1, L1), "p_y": (L2, L2), "p_z": (L1, L2)}[which], np.int64)
    for rows, cols, _ in sources(case, which, node):
        cnt[rows, cols] += 1
    return int(cnt.max())


# ---- the oracle's side, computed once per case ----
_SETUP = {}


def reference(oracle, case):
    """orc_pipeline_node_setup of the case's nodes (read-only: shared between tests)"""
    if case.key not in _SETUP:
        pl = R.oracle_pipeline(oracle, case)
        outs = [pl.node_setup(*node) for node in case.nodes]
        pl.close()
        for o in outs:
            for a in o.values():
                a.setflags(write=False)
        _SETUP[case.key] = outs
    return _SETUP[case.key]


# ---- what the lists, maps and consensus-pair arrays must be, from the oracle's matrices and pairs ----
def lists_of(p, upper):
    """(ptr, col, map) of the cells of p above the cut-off (upper: j > i only), columns ascending row by row"""
    keep = p > CUT
    if upper:
        keep &= np.triu(np.ones(p.shape, bool), 1)
    ptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.uint32)
    col = np.nonzero(keep)[1].astype(np.uint32)
    m = np.full(p.shape, -1, np.int32)
    m[keep] = np.arange(len(col), dtype=np.int32)
    return ptr, col, m


def cz_of(cbp, L1, L2):
    """(ptr, k, map) of the sorted distinct cells (i, k) and (j, l) of the consensus pairs"""
    flag = np.zeros((L1, L2), bool)
    if len(cbp):
        flag[cbp[:, 0], cbp[:, 2]] = True
        flag[cbp[:, 1], cbp[:, 3]] = True
    ptr = np.concatenate([[0], np.cumsum(flag.sum(axis=1))]).astype(np.uint32)
    k = np.nonzero(flag)[1].astype(np.uint32)
    m = np.full((L1, L2), -1, np.int32)
    m[flag] = np.arange(len(k), dtype=np.int32)
    return ptr, k, m


def env4_of(env, L1):
    """dd.h: {max(first, 1), second} of row r at index r + 64, the empty range {1, 0} for the 64 rows before row 1 and the 65
    behind row L1"""
    e = np.asarray(env, np.uint32).reshape(-1, 2)
    out = np.tile(np.array([1, 0], np.uint32), (L1 + 130, 1))
    out[65:L1 + 65, 0] = np.maximum(e[1:, 0], 1)
    out[65:L1 + 65, 1] = e[1:, 1]
    return out.reshape(-1)


MATRICES = ("p_x", "p_y", "p_z")
SETUP_ARRAYS = ("p_x", "p_y", "p_z", "x_ptr", "x_col", "x_map", "y_ptr", "y_col", "y_map", "pz_ptr", "pz_k", "cz_ptr", "cz_k", "zmap", "env", "cbp_cnt", "cbp")


def first_matrix_difference(got, want):
    """None, or 'cell (i, j): 0x........ (value), oracle 0x........ (value); n cells differ' by the bytes of float32 matrices"""
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    if g.shape != w.shape:
        return "shape %r, oracle %r" % (g.shape, w.shape)
    bad = np.argwhere(g != w)
    if not len(bad):
        return None
    i, j = (int(v) for v in bad[0])
    return "cell (%d, %d): 0x%08x (%r), oracle 0x%08x (%r); %d cells differ" % (i, j, g[i, j], float(got[i, j]), w[i, j], float(want[i, j]), len(bad))


def _same(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return "%s has shape %r, expected %r" % (name, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        at = tuple(int(v) for v in bad[0])
        return "%s differs first at %r: %d, expected %d (%d entries differ)" % (name, at, int(got[at]), int(want[at]), len(bad))
    return None


def setup_difference(peek, want):
    """None, or a sentence naming the first array of a peeked node (dict name -> array, SETUP_ARRAYS) that is not what the
    oracle's set-up (reference()) implies"""
    for m in MATRICES:
        d = first_matrix_difference(peek[m], want[m])
        if d:
            return "%s: %s" % (m, d)
    L1, L2 = want["p_z"].shape
    for side, m in (("x", "p_x"), ("y", "p_y")):
        ptr, col, mp = lists_of(want[m], True)
        for name, w in ((side + "_ptr", ptr), (side + "_col", col), (side + "_map", mp)):
            d = _same(name, peek[name], w)
            if d:
                return d
    ptr, col, _ = lists_of(want["p_z"], False)
    for name, w in (("pz_ptr", ptr), ("pz_k", col)):
        d = _same(name, peek[name], w)
        if d:
            return d
    d = _same("env", peek["env"], want["env"])
    if d:
        return d
    cbp = np.asarray(want["cbp"], np.int64).reshape(-1, 4)
    got = np.asarray(peek["cbp"]).reshape(-1, 8)
    d = _same("cbp (i, j, k, l)", got[:, :4], cbp)
    if d:
        return d
    if len(cbp):
        xm, ym = np.asarray(peek["x_map"]), np.asarray(peek["y_map"])
        d = _same("cbp entry of p_x", got[:, 4].astype(np.int64), xm[cbp[:, 0], cbp[:, 1]]) or _same("cbp entry of p_y", got[:, 5].astype(np.int64), ym[cbp[:, 2], cbp[:, 3]])
        if d:
            return d
    nx = len(peek["x_col"])
    per_entry = np.bincount(np.asarray(peek["x_map"])[cbp[:, 0], cbp[:, 1]], minlength=nx) if len(cbp) else np.zeros(nx, np.int64)
    # k_node_cbp_fill scans the counts in place: a node with consensus pairs shows their running total
    d = _same("cbp_cnt", peek["cbp_cnt"], np.cumsum(per_entry) if len(cbp) else per_entry)
    if d:
        return d
    ptr, k, zm = cz_of(cbp, L1, L2)
    for name, w in (("cz_ptr", ptr), ("cz_k", k), ("zmap", zm)):
        d = _same(name, peek[name], w)
        if d:
            return d
    if len(cbp):
        z = np.asarray(peek["zmap"])
        d = _same("cbp cell of (i, k)", got[:, 6].astype(np.int64), z[cbp[:, 0], cbp[:, 2]]) or _same("cbp cell of (j, l)", got[:, 7].astype(np.int64), z[cbp[:, 1], cbp[:, 3]])
        if d:
            return d
    return None


# ---- the device's side ----
def peek_all(ctx, handle, arrays=SETUP_ARRAYS):
    return {a: ctx.node_peek(handle, a) for a in arrays}


def open_and_peek(cases, copies=1, **kw):
    """the nodes of the cases (each `copies` times) in ONE open call: per case and copy the peeked arrays of its first node"""
    ctx, nodes = R.open_context(cases)
    try:
        batch = [n[0] for n in nodes for _ in range(copies)]
        handles, _ = ctx.nodes_open(batch, R.device_params(cases[0], **kw))
        out = [peek_all(ctx, h) for h in handles]
        ctx.nodes_close()
    finally:
        ctx.close()
    return [out[k * copies:(k + 1) * copies] for k in range(len(cases))]
