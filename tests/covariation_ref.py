"""Plain Python / numpy restatement of the covariation statistics (dafs_hip_alignment_covariation).
The yardstick of tests/test_covariation_*.py: every number is defined here to the bit.

Scalar definitions (mix, perm, lnq, gq_pair, s_scalar) use Python ints and Python floats only.  restate() evaluates the same
definitions over whole matrices with numpy: int64 sums are exact and order-free, and every float64 array operation is the
one IEEE operation of the scalar form, in the same order (test_covariation_cpu.py checks the two forms against each other)."""
import math

import numpy as np

NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
CANONICAL = ((0, 3), (3, 0), (2, 1), (1, 2), (2, 3), (3, 2))  # AU UA GC CG GU UG

_CODE = {"A": 0, "a": 0, "C": 1, "c": 1, "G": 2, "g": 2, "U": 3, "u": 3, "T": 3, "t": 3}


def encode(rows):
    """text rows -> uint8 [n, len]: A 0, C 1, G 2, U/T 3 (either case), everything else 4"""
    rows = list(rows)
    out = np.full((len(rows), len(rows[0]) if rows else 0), 4, np.uint8)
    for r, row in enumerate(rows):
        assert len(row) == out.shape[1]
        for c, ch in enumerate(row):
            out[r, c] = _CODE.get(ch, 4)
    return out


def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def perm(seed, k, c, n):
    """the permutation of column c in shuffle k: the shuffled alignment has code[p[r]][c] at row r"""
    base = mix(seed + GOLDEN * (k + 1))
    p = list(range(n))
    for i in range(n - 1, 0, -1):
        u = mix(base + ((c << 32) | i))
        j = ((u >> 32) * (i + 1)) >> 32
        p[i], p[j] = p[j], p[i]
    return p


def lnq(n):
    """LNQ[0..n] as Python ints"""
    return [0] + [int(math.floor(math.log(float(k)) * 65536 + 0.5)) for k in range(1, n + 1)]


def counts_pair(code, c1, c2):
    """n_ab of two columns as a 4 x 4 list of Python ints"""
    nab = [[0] * 4 for _ in range(4)]
    for r in range(code.shape[0]):
        a, b = int(code[r, c1]), int(code[r, c2])
        if a < 4 and b < 4:
            nab[a][b] += 1
    return nab


def gq_pair(code, c1, c2, table=None):
    if c1 == c2:
        return 0
    table = lnq(code.shape[0]) if table is None else table
    nab = counts_pair(code, c1, c2)
    ra = [sum(nab[a]) for a in range(4)]
    sb = [sum(nab[a][b] for a in range(4)) for b in range(4)]
    m = sum(ra)
    return 2 * sum(nab[a][b] * (table[nab[a][b]] + table[m] - table[ra[a]] - table[sb[b]]) for a in range(4) for b in range(4))


def s_scalar(g, r1, r2, t, length):
    """S of one pair from Python ints, in Python floats, operations in the stated order"""
    apc = 0.0
    if t != 0:
        apc = float(r1) * float(r2) / float(t) * (float(length) / float(length - 1))
    return (float(g) - apc) / 65536.0


# ------------------------------------------------------------------------------------------------- whole matrices
def joint_counts(code):
    """n_ab for every pair of columns: int64 [4, 4, len, len]"""
    one = [(code == a).astype(np.int64) for a in range(4)]
    return np.array([[one[a].T @ one[b] for b in range(4)] for a in range(4)], np.int64)


def gq_matrix(code, table=None):
    n, length = code.shape
    t = np.array(lnq(n) if table is None else table, np.int64)
    nab = joint_counts(code)
    ra = nab.sum(1)  # [a, len, len]
    sb = nab.sum(0)  # [b, len, len]
    m = ra.sum(0)
    g = np.zeros((length, length), np.int64)
    for a in range(4):
        for b in range(4):
            g += nab[a, b] * (t[nab[a, b]] + t[m] - t[ra[a]] - t[sb[b]])
    g *= 2
    g[np.arange(length), np.arange(length)] = 0
    return g, nab


def s_matrix(g, col_sum, total, length):
    """S for every pair (the diagonal is meaningless); float64 operations in the stated order"""
    if length < 2:
        return np.zeros(g.shape, np.float64)
    rd = col_sum.astype(np.float64)
    if total != 0:
        apc = rd[:, None] * rd[None, :] / np.float64(float(total)) * np.float64(float(length) / float(length - 1))
    else:
        apc = np.zeros(g.shape, np.float64)
    return (g.astype(np.float64) - apc) / np.float64(65536.0)


def shuffled(code, seed, k):
    """the shuffled alignment of shuffle k (numpy uint64 arithmetic wraps mod 2^64 as mix does)"""
    n, length = code.shape
    out = code.copy()
    if n < 2:
        return out
    with np.errstate(over="ignore"):
        base = np.uint64(mix(seed + GOLDEN * (k + 1)))
        cols = np.arange(length, dtype=np.uint64) << np.uint64(32)
        ar = np.arange(length)
        for i in range(n - 1, 0, -1):
            z = base + (cols | np.uint64(i))
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            u = z ^ (z >> np.uint64(31))
            j = (((u >> np.uint64(32)) * np.uint64(i + 1)) >> np.uint64(32)).astype(np.int64)
            vi = out[i, ar].copy()
            out[i, ar] = out[j, ar]
            out[j, ar] = vi
    return out


def check_ss(ss, length):
    used = [False] * length
    for c in range(length):
        p = int(ss[c])
        if p == NONE:
            continue
        assert c < p < length and not used[c] and not used[p], "bad ss"
        used[c] = used[p] = True


def restate(code, ss=None, shuffles=100, seed=1, matrix=True):
    """Every output of dafs_hip_alignment_covariation as a dict of numpy arrays (total: a Python int; g with matrix)."""
    code = np.ascontiguousarray(code, np.uint8)
    n, length = code.shape
    nan = float("nan")
    out = dict(col_sum=np.zeros(length, np.int64), best=np.full(length, NONE, np.uint32), best_score=np.zeros(length, np.float64),
               best_e=np.full(length, nan if shuffles == 0 else 0.0), pair_score=np.zeros(length, np.float64),
               pair_e=np.zeros(length, np.float64), pair_rows=np.zeros(length, np.uint32), pair_canonical=np.zeros(length, np.uint32),
               pair_types=np.zeros(length, np.uint32), total=0)
    if matrix:
        out["g"] = np.zeros((length, length), np.int64)
    lefts = []
    if ss is not None:
        check_ss(ss, length)
        lefts = [c for c in range(length) if int(ss[c]) != NONE]
    if shuffles == 0:
        out["pair_e"][lefts] = nan
    if n < 2 or length < 2:
        return out
    table = lnq(n)
    g, nab = gq_matrix(code, table)
    col_sum = g.sum(1)
    total = int(col_sum.sum())
    s = s_matrix(g, col_sum, total, length)
    out["col_sum"], out["total"] = col_sum, total
    if matrix:
        out["g"] = g
    masked = s.copy()
    masked[np.arange(length), np.arange(length)] = -np.inf
    best = masked.argmax(1)  # the first maximum: the smallest c'
    out["best"] = best.astype(np.uint32)
    out["best_score"] = s[np.arange(length), best]
    for c1 in lefts:
        c2 = int(ss[c1])
        out["pair_score"][c1] = s[c1, c2]
        out["pair_rows"][c1] = nab[:, :, c1, c2].sum()
        out["pair_canonical"][c1] = sum(int(nab[a, b, c1, c2]) for a, b in CANONICAL)
        out["pair_types"][c1] = sum(1 for a, b in CANONICAL if nab[a, b, c1, c2] > 0)
    if shuffles > 0:
        iu = np.triu_indices(length, 1)
        tail_best = np.zeros(length, np.int64)
        tail_pair = np.zeros(len(lefts), np.int64)
        ps = out["pair_score"][lefts]
        for k in range(shuffles):
            gk, _ = gq_matrix(shuffled(code, seed, k), table)
            rk = gk.sum(1)
            sk = np.sort(s_matrix(gk, rk, int(rk.sum()), length)[iu])
            tail_best += len(sk) - np.searchsorted(sk, out["best_score"], side="left")
            tail_pair += len(sk) - np.searchsorted(sk, ps, side="left")
        out["best_e"] = np.array([int(t) / float(shuffles) for t in tail_best], np.float64)
        out["pair_e"][lefts] = [int(t) / float(shuffles) for t in tail_pair]
    return out


# ------------------------------------------------------------------------------------- the planted-covariation case
def planted_alignment():
    """48 rows x 100 columns: a random ancestor, each cell redrawn with probability 0.35, eight complementary planted pairs
    (5 + i, 60 - i) with 10 % noise, 5 % non-nucleotides; the consensus is the planted pairs"""
    rng = np.random.default_rng(1)
    n, length = 48, 100
    code = np.tile(rng.integers(0, 4, length), (n, 1))
    redraw = rng.random((n, length)) < 0.35
    code[redraw] = rng.integers(0, 4, int(redraw.sum()))
    ss = np.full(length, NONE, np.uint32)
    for i in range(8):
        c1, c2 = 5 + i, 60 - i
        left = rng.integers(0, 4, n)
        right = 3 - left
        noise = rng.random(n) < 0.10
        right[noise] = rng.integers(0, 4, int(noise.sum()))
        code[:, c1], code[:, c2] = left, right
        ss[c1] = c2
    code[rng.random((n, length)) < 0.05] = 4
    return code.astype(np.uint8), ss


def check_planted(out, ss):
    """exactly the planted pairs have E <= 0.05, and they are the largest best scores"""
    lefts = [c for c in range(len(ss)) if ss[c] != NONE]
    planted = sorted(lefts + [int(ss[c]) for c in lefts])
    assert (out["pair_e"][lefts] <= 0.05).all()
    assert sorted(np.nonzero(out["best_e"] <= 0.05)[0].tolist()) == planted
    for c in lefts:
        assert out["best"][c] == ss[c] and out["best"][ss[c]] == c
        assert out["best_score"][c] == out["pair_score"][c]
    assert sorted(np.argsort(-out["best_score"], kind="stable")[:len(planted)].tolist()) == planted
