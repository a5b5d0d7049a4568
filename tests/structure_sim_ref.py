"""Plain numpy / Python restatement of the structural pair score, to the bit: float64 products in the
contract's bracketing, Python integers for every sum, and the two host formulas.  Nothing here calls the library or a device:
the tests compare it with dafs_host_structure_score / dafs_host_mix_score (test_cluster_structure_cpu.py) and with the kernels
(test_cluster_structure_gpu.py).

Rows are CSR triples (rowptr, col, val): `mp` the rows of mp[x][y] (len[x] rows, columns k ascending), `bp` the rows of a
sequence's base-pairing store (columns j > i ascending)."""
import numpy as np

SCALE = float(1 << 40)
MAX_TERMS = 1 << 24


def c(v):
    """a stored float as a double clamped into [0, 1]; NaN becomes 0"""
    v = np.float64(np.float32(v))
    if not v > 0.0:
        return np.float64(0.0)
    return v if v < 1.0 else np.float64(1.0)


def row(csr, i):
    rp, col, val = csr
    return [(int(col[e]), val[e]) for e in range(int(rp[i]), int(rp[i + 1]))]


def pair_terms(mp, bp_x, bp_y):
    """(T, terms) of one pair: Python integers"""
    lx, ly = len(bp_x[0]) - 1, len(bp_y[0]) - 1
    q_of = {}
    for k in range(ly):
        for l, q in row(bp_y, k):
            q_of[(k, l)] = q
    T = terms = 0
    for i in range(lx):
        for j, p in row(bp_x, i):
            if j >= lx:
                continue
            for k, a in row(mp, i):
                for l, b in row(mp, j):
                    if l <= k or (k, l) not in q_of:  # bp[y] holds l > k only
                        continue
                    T += int(np.floor(((c(p) * c(q_of[(k, l)])) * (c(a) * c(b))) * SCALE))
                    terms += 1
    return T, terms


def weight(bp_x):
    """W of one sequence"""
    return sum(int(np.floor(c(p) * SCALE)) for p in bp_x[2])


def structure_score(T, wx, wy):
    w = min(int(wx), int(wy))
    if w == 0:
        return np.float32(0.0)
    return np.float32(min(1.0, float(int(T)) / float(w)))  # both conversions round to nearest, then one division


def mix_score(sim, st, w):
    return np.float32(np.float64(np.float32(sim)) + np.float64(np.float32(w)) * (np.float64(np.float32(st)) - np.float64(np.float32(sim))))


def transpose(mp, ly):
    """the rows of mp[y][x] from those of mp[x][y], columns ascending"""
    rp, col, val = mp
    lx = len(rp) - 1
    rows = [[] for _ in range(ly)]
    for i in range(lx):
        for k, a in row(mp, i):
            rows[k].append((i, a))
    trp = np.zeros(ly + 1, np.uint32)
    trp[1:] = np.cumsum([len(r) for r in rows])
    tcol = np.array([i for r in rows for i, _ in r], np.uint32)
    tval = np.array([a for r in rows for _, a in r], np.float32)
    return trp, tcol, tval


def matrices(n, mps, bps, sim=None, kind="structure", w=0.5):
    """(T, terms, W, struct, chosen) of n sequences: mps[(x, y)] the rows of mp[x][y] for x < y, bps[x] the rows of bp[x].
    T and terms are dicts over the pairs, W a list, struct and chosen n x n float32 matrices with unit diagonals (chosen is
    struct, or with kind "mix" the mix with the n x n float32 matrix sim at weight w)."""
    W = [weight(bps[x]) for x in range(n)]
    T, terms = {}, {}
    st = np.eye(n, dtype=np.float32)
    for x in range(n):
        for y in range(x + 1, n):
            T[(x, y)], terms[(x, y)] = pair_terms(mps[(x, y)], bps[x], bps[y])
            st[x, y] = st[y, x] = structure_score(T[(x, y)], W[x], W[y])
    chosen = st
    if kind == "mix":
        chosen = np.eye(n, dtype=np.float32)
        for x in range(n):
            for y in range(n):
                if x != y:
                    chosen[x, y] = mix_score(sim[x, y], st[x, y], w)
    return T, terms, W, st, chosen


def test_set():
    """(names, seqs, family): 15 sequences -- three synth.structured_family_set families of four at about 40, 60 and 90 nt,
    interleaved (ranges cut from them fall into different launch plans of the pair kernels), and three unrelated sequences of
    130, 9 and 3 nt, the last too short to hold a base pair.  family[i]: 0, 1, 2 or None."""
    from dafs_amd import synth
    a = synth.structured_family_set(4, 40, stems=1, seed=91)
    b = synth.structured_family_set(4, 60, stems=2, seed=92)
    c = synth.structured_family_set(4, 90, stems=3, seed=93)
    long_, short = synth.random_set(1, 130, seed=94, jitter=0.0)[0], synth.random_set(1, 9, seed=95, jitter=0.0)[0]
    recs = [("a%d" % k, a[k][1], 0) for k in range(4)] + [("b%d" % k, b[k][1], 1) for k in range(4)] + [("c%d" % k, c[k][1], 2) for k in range(4)]
    order = [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11]
    recs = ([recs[k] for k in order[:5]] + [("r9", short[1], None)] + [recs[k] for k in order[5:9]] + [("r3", "GAC", None)]
            + [recs[k] for k in order[9:]] + [("r130", long_[1], None)])
    return [r[0] for r in recs], [r[1] for r in recs], [r[2] for r in recs]


test_set.__test__ = False  # a helper of the test modules, not a test
