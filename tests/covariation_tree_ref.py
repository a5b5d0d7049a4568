"""Plain Python / numpy restatement of the tree-aware null of the covariation statistics ("Null by
evolution along a tree"; dafs_hip_alignment_covariation_null, dafs_hip_covariation_null_alignment).  The yardstick of
tests/test_covariation_tree_*.py: every number is defined here to the bit.  Nothing here calls the library or a device.

Scalar forms (pi, fitch_column) use Python ints only.  pi_all evaluates the same permutation for every column at once with
numpy uint64 (wrapping mod 2^64 as mix does); test_covariation_tree_cpu.py checks the two forms against each other."""
import numpy as np

import covariation_ref as cr
import linkage_ref

NONE = cr.NONE
M64 = cr.M64
GOLDEN = cr.GOLDEN
NULLS = ("shuffle", "tree")


# ------------------------------------------------------------------------------------------------ the column permutation
def halfbits(length):
    """the smallest h >= 1 with 4^h >= length"""
    h = 1
    while (1 << (2 * h)) < length:
        h += 1
    return h


def feistel(key, h, x):
    """F: a bijection of [0, 4^h); four rounds on the two h-bit halves of x"""
    mask = (1 << h) - 1
    L, R = x >> h, x & mask
    for r in range(4):
        L, R = R, L ^ (cr.mix(key + GOLDEN * (r + 1) + R) & mask)
    return (L << h) | R


def pi(key, length, c):
    """the stateless bijection of [0, length): walk F's cycle from c until it returns below length"""
    h = halfbits(length)
    x = feistel(key, h, c)
    while x >= length:
        x = feistel(key, h, x)
    return x


def _mix_vec(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def _feistel_vec(key, h, x):
    mask = np.uint64((1 << h) - 1)
    hh = np.uint64(h)
    L, R = x >> hh, x & mask
    for r in range(4):
        L, R = R, L ^ (_mix_vec(np.uint64((key + GOLDEN * (r + 1)) & M64) + R) & mask)
    return (L << hh) | R


def pi_all(key, length):
    """pi(key, length, c) for every c: int64 [length]"""
    h = halfbits(length)
    with np.errstate(over="ignore"):
        x = _feistel_vec(key, h, np.arange(length, dtype=np.uint64))
        while True:
            out = x >= np.uint64(length)
            if not out.any():
                break
            x[out] = _feistel_vec(key, h, x[out])
    return x.astype(np.int64)


# ------------------------------------------------------------------------------------------------------------- the tree
def check_tree(n, left, right):
    """the checks of dafs_host_cluster_cut; returns parent[2n-1] (the root's is -1)"""
    left, right = np.asarray(left, np.int64), np.asarray(right, np.int64)
    T = 2 * n - 1
    assert left.shape == (T,) and right.shape == (T,), "bad tree"
    parent = np.full(T, -1, np.int64)
    for i in range(T):
        if i < n:
            assert left[i] == -1 and right[i] == -1, "a leaf with a child"
            continue
        assert left[i] != right[i], "a join of a node with itself"
        for ch in (int(left[i]), int(right[i])):
            assert 0 <= ch < i, "a child that is not an earlier node"
            assert parent[ch] == -1, "a node that is a child twice"
            parent[ch] = i
    return parent


def similarity(code):
    """sim(r, s) of item 5: float32 [n, n] (the diagonal is not read by the linkage)"""
    code = np.asarray(code, np.uint8)
    base = code <= 3
    assert base.any(1).all(), "a row without a base"
    both = base.astype(np.int64) @ base.astype(np.int64).T
    ident = sum(((code == a).astype(np.int64) @ (code == a).astype(np.int64).T) for a in range(4))
    sim = np.zeros(both.shape, np.float32)
    nz = both > 0
    sim[nz] = (ident[nz].astype(np.float64) / both[nz].astype(np.float64)).astype(np.float32)
    return sim


def default_tree(code):
    """(left, right) of average linkage on similarity(code)"""
    _, left, right = linkage_ref.linkage_ref(similarity(code), "average")
    return left, right


def comb_tree(n):
    """the left comb: join t takes the previous join (leaf 0 first) and leaf t + 1"""
    left = np.array([-1] * n + [0] + list(range(n, 2 * n - 2)), np.int64)[:2 * n - 1]
    right = np.array([-1] * n + list(range(1, n)), np.int64)
    return left, right


def balanced_tree(n):
    """joins of neighbours, level by level (an odd one out waits for the next level)"""
    left, right = [-1] * n, [-1] * n
    level = list(range(n))
    while len(level) > 1:
        nxt = []
        for i in range(0, len(level) - 1, 2):
            nxt.append(len(left))
            left.append(level[i])
            right.append(level[i + 1])
        if len(level) % 2:
            nxt.append(level[-1])
        level = nxt
    return np.array(left, np.int64), np.array(right, np.int64)


def random_tree(n, rs):
    """joins of two clusters drawn at random (rs: a numpy RandomState)"""
    left, right = [-1] * n, [-1] * n
    active = list(range(n))
    while len(active) > 1:
        a = active.pop(int(rs.randint(len(active))))
        b = active.pop(int(rs.randint(len(active))))
        active.append(len(left))
        left.append(a)
        right.append(b)
    return np.array(left, np.int64), np.array(right, np.int64)


def relabel_tree(left, right, perm):
    """the tree of the alignment code[perm]: row i of it is old row perm[i], so old leaf perm[i] becomes leaf i"""
    n = len(perm)
    new = np.arange(2 * n - 1, dtype=np.int64)
    new[np.asarray(perm)] = np.arange(n)
    f = lambda a: np.array([-1 if v < 0 else new[v] for v in a], np.int64)
    return f(left), f(right)


# ------------------------------------------------------------------------------------------ Fitch sets, states, changes
def low(s):
    return (s & -s).bit_length() - 1


def fitch_column(col, left, right, parent):
    """one column in Python ints: (sets, states, chg) as lists over the 2n-1 nodes"""
    n = len(col)
    T = 2 * n - 1
    sets = [0] * T
    for r in range(n):
        sets[r] = (1 << int(col[r])) if col[r] < 4 else 15
    for v in range(n, T):
        i = sets[left[v]] & sets[right[v]]
        sets[v] = i if i != 0 else sets[left[v]] | sets[right[v]]
    state, chg = [0] * T, [0] * T
    state[T - 1] = low(sets[T - 1])
    for v in range(T - 2, -1, -1):
        p = state[parent[v]]
        state[v] = p if (sets[v] >> p) & 1 else low(sets[v])
        chg[v] = 0 if state[v] == p else 1 + 4 * p + state[v]
    return sets, state, chg


_LOW = np.array([0] + [low(s) for s in range(1, 16)], np.uint8)


def fitch(code, left, right):
    """every column at once: (sets, state, chg), uint8 [2n-1, len]"""
    code = np.asarray(code, np.uint8)
    n, length = code.shape
    parent = check_tree(n, left, right)
    T = 2 * n - 1
    sets = np.zeros((T, length), np.uint8)
    sets[:n] = np.where(code < 4, np.uint8(1) << np.minimum(code, 3), np.uint8(15))
    for v in range(n, T):
        i = sets[left[v]] & sets[right[v]]
        sets[v] = np.where(i != 0, i, sets[left[v]] | sets[right[v]])
    state = np.zeros((T, length), np.uint8)
    chg = np.zeros((T, length), np.uint8)
    state[T - 1] = _LOW[sets[T - 1]]
    for v in range(T - 2, -1, -1):
        p = state[parent[v]]
        state[v] = np.where((sets[v] >> p) & 1 != 0, p, _LOW[sets[v]])
        chg[v] = np.where(state[v] == p, 0, 1 + 4 * p + state[v])
    return sets, state, chg


def parsimony(code, left, right):
    """Fitch's score per column: the joins whose children's sets do not meet"""
    sets, _, _ = fitch(code, left, right)
    n = code.shape[0]
    return sum(((sets[left[v]] & sets[right[v]]) == 0).astype(np.int64) for v in range(n, 2 * n - 1)) if n > 1 else 0


# ---------------------------------------------------------------------------------------------------- the null alignment
def node_key(seed, k, v):
    base = cr.mix(seed + GOLDEN * (k + 1))
    return cr.mix(base ^ (((v + 1) << 32) & M64))


def evolve(code, left, right, seed, k, fit=None, nodes=False):
    """null alignment k: uint8 [n, len]; with nodes, the states ns of every node before the gaps go back in"""
    code = np.asarray(code, np.uint8)
    n, length = code.shape
    parent = check_tree(n, left, right)
    _, state, chg = fitch(code, left, right) if fit is None else fit
    T = 2 * n - 1
    ns = np.zeros((T, length), np.uint8)
    ns[T - 1] = state[T - 1]
    for v in range(T - 2, -1, -1):
        rec = chg[v][pi_all(node_key(seed, k, v), length)].astype(np.int64)
        p = ns[parent[v]]
        a, b = ((rec - 1) >> 2) & 3, (rec - 1) & 3
        ns[v] = np.where(rec == 0, p, np.where(b != p, b, a))
    if nodes:
        return ns
    return np.where(code == 4, np.uint8(4), ns[:n]).astype(np.uint8)


def null_alignment(code, null, tree, seed, k):
    """what dafs_hip_covariation_null_alignment returns"""
    code = np.ascontiguousarray(code, np.uint8)
    if null == "shuffle":
        assert tree is None
        return cr.shuffled(code, seed, k)
    assert null == "tree"
    left, right = default_tree(code) if tree is None else tree
    return evolve(code, left, right, seed, k)


def restate(code, ss=None, shuffles=100, seed=1, null="tree", tree=None, matrix=True):
    """every output of dafs_hip_alignment_covariation_null: covariation_ref.restate with the null alignments of `null`"""
    code = np.ascontiguousarray(code, np.uint8)
    if null == "shuffle":
        assert tree is None
        return cr.restate(code, ss, shuffles, seed, matrix)
    assert null == "tree"
    out = cr.restate(code, ss, 0, seed, matrix)  # the alignment's own numbers do not depend on the null
    n, length = code.shape
    if shuffles == 0 or n < 2 or length < 2:
        if shuffles:
            out["best_e"] = np.zeros(length, np.float64)
            out["pair_e"] = np.zeros(length, np.float64)
        return out
    left, right = default_tree(code) if tree is None else tree
    fit = fitch(code, left, right)
    lefts = [c for c in range(length) if ss is not None and int(ss[c]) != NONE]
    table = cr.lnq(n)
    iu = np.triu_indices(length, 1)
    tail_best = np.zeros(length, np.int64)
    tail_pair = np.zeros(len(lefts), np.int64)
    ps = out["pair_score"][lefts]
    for k in range(shuffles):
        gk, _ = cr.gq_matrix(evolve(code, left, right, seed, k, fit), table)
        rk = gk.sum(1)
        sk = np.sort(cr.s_matrix(gk, rk, int(rk.sum()), length)[iu])
        tail_best += len(sk) - np.searchsorted(sk, out["best_score"], side="left")
        tail_pair += len(sk) - np.searchsorted(sk, ps, side="left")
    out["best_e"] = np.array([int(t) / float(shuffles) for t in tail_best], np.float64)
    out["pair_e"] = np.zeros(length, np.float64)
    out["pair_e"][lefts] = [int(t) / float(shuffles) for t in tail_pair]
    return out


# ------------------------------------------------------------------------------------------- the case the null exists for
def phylo(seed, planted, n=48, length=100):
    """rows evolved on a two-level tree (4 clades x 3 subclades x n/12 members), every column independent but for `planted`
    complementary pairs (5 + i, 60 - i); 5 % non-bases.  The draws keep this order."""
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 4, length)
    pairs = [(5 + i, 60 - i) for i in range(planted)]
    rows = []

    def mutate(x, rate):
        y = x.copy()
        hit = rng.random(length) < rate
        y[hit] = rng.integers(0, 4, int(hit.sum()))
        for c1, c2 in pairs:
            if rng.random() < rate * 2:
                y[c1] = rng.integers(0, 4)
            y[c2] = 3 - y[c1]
        return y

    for clade in range(4):
        f = mutate(anc, 0.5)
        for sub in range(3):
            g = mutate(f, 0.2)
            for m in range(n // 12):
                rows.append(mutate(g, 0.08))
    code = np.array(rows, np.uint8)
    code[rng.random(code.shape) < 0.05] = 4
    ss = np.full(length, NONE, np.uint32)
    for c1, c2 in pairs:
        ss[c1] = c2
    return code, ss
