"""Shapes, inputs and comparison of the node-level solver tests (test_dd_nodes_cpu.py, test_dd_nodes_gpu.py): one node of
the progressive phase on supplied stores, device (Context.solve_nodes) against oracle (orc_pipeline_solve_node).
Test infrastructure only -- nothing under dafs_amd/ imports this."""
import numpy as np

TH_A, TH_S = 0.01, 0.2   # the defaults of both sides (dafs.cpp:1612-1640)

# (L1, L2) = columns of the two child alignments.  Per (lds_flags, fold_fast) class that dafs_hipk_dd_node_plan gives the
# default-switch rows of tests/golden/dd_node_plan.npz with both sides <= 1025, the smallest shape (by cells L1 * L2, then L1)
# whose short side is at least 30; and its mirror wherever the mirror's class differs.  test_dd_nodes_cpu.py checks all of it
# against the fixture and the planner.
SHAPES = [(63, 63), (63, 65), (63, 255), (63, 256), (63, 511), (511, 63), (63, 767), (767, 63), (63, 769), (769, 63),
          (63, 1024), (1024, 63), (63, 1025), (1025, 63), (255, 255), (255, 256), (257, 257), (511, 511), (511, 769), (769, 511),
          (511, 1024), (1024, 511), (511, 1025), (1025, 511), (769, 769), (767, 1023), (1023, 767), (767, 1025), (1025, 767),
          (769, 1023), (769, 1025), (1025, 769), (1025, 1025)]
DEGENERATE = [(1, 1), (1, 2), (2, 1), (1, 65), (1, 769), (769, 1), (1025, 1)]
TABLE = SHAPES + DEGENERATE

# one shape per form family of the folding DPs, for the quantised inputs
FAMILIES = {"span side by side": (63, 63), "register side by side": (257, 257), "shared region": (255, 256), "codes in HBM": (511, 511),
            "48 lanes": (63, 767), "workgroup form": (1025, 63), "span folders in split mode": (63, 65)}
SWITCHES = [None, "DAFS_HIP_DD_SPAN=0", "DAFS_HIP_DD_SPLIT=0", "DAFS_HIP_DD_NWG=1", "DAFS_HIP_DD_WG=2"]
ALL_SWITCHES = ("WIDE", "SPAN", "NWG", "WG", "SPAN_MW", "SPLIT")

# multi-row children: both span-sized, one register-sized beside one on 48 lanes, one beyond 1024 columns
MULTIROW_SHAPES = [(100, 120), (300, 600), (1030, 200)]
SUPPLIED_SHAPES = [(90, 130), (300, 70)]


def t_max_of(L1, L2):
    """Iteration cap of a case: the default for the shapes of at most 65 columns (sparse enough to converge, see densities),
    else 25, or 12 beyond 600 columns, where an iteration of the oracle's dense tables takes ~0.1 s"""
    return 600 if max(L1, L2) <= 65 else 25 if max(L1, L2) <= 600 else 12


def densities(L1, L2):
    """(base pairs per column, share of them common to both sides): sparser and more alike where the cap is the default, so
    that the multipliers can settle; elsewhere dense and different enough that the cap ends the run"""
    return (0.8, 0.8) if max(L1, L2) <= 65 else (1.2, 0.6)


def plan_class(L1, L2):
    """(lds_flags, fold_fast) of the planner under the switches of the environment as it is now"""
    from dafs_amd import capi
    p = capi.DdNodePlan()
    assert capi.dd_node_plan(L1, L2, p) == 0
    return p.lds_flags, p.fold_fast


def _csr(rows):
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    col = np.array([c for r in rows for c, _ in r], np.uint32)
    val = np.array([v for r in rows for _, v in r], np.float32)
    return rp, col, val


def _band(rng, La, Lb, quant):
    """rows of mp[a][b]: a band of +-2 around the scaled diagonal j = i * Lb // La, values in (th_a, 1], largest on the diagonal"""
    rows = []
    for i in range(La):
        c = i * Lb // La
        r = []
        for j in range(max(0, c - 2), min(Lb, c + 3)):
            d = abs(j - c)
            if quant:
                v = int(rng.integers(*((3, 9), (1, 7), (1, 5))[d])) / 8.0
            else:
                lo, hi = ((0.5, 1.0), (0.1, 0.5), (0.02, 0.2))[d]
                v = lo + (hi - lo) * rng.random()
            r.append((j, np.float32(v)))
        rows.append(r)
    return _csr(rows)


def _pairs(rng, L, count):
    """count random pairs (i, j) of 0 .. L-1 with j - i >= 4, as a set"""
    if L < 5 or count <= 0:
        return set()
    i = rng.integers(0, L, count); j = rng.integers(0, L, count)
    return {(int(min(a, b)), int(max(a, b))) for a, b in zip(i, j) if abs(int(a) - int(b)) >= 4}


def _bp_rows(rng, L, strong, extra, quant):
    """base-pairing rows of one sequence: the pairs of `strong` above th_s, those of `extra` anywhere above the cut-off"""
    rows = [[] for _ in range(L)]
    for (i, j) in sorted(strong | extra):
        if quant:
            v = int(rng.integers(2 if (i, j) in strong else 1, 5)) / 4.0
        else:
            v = 0.3 + 0.7 * rng.random() if (i, j) in strong else 0.02 + 0.98 * rng.random()
        rows[i].append((j, np.float32(v)))
    return _csr(rows)


def stores(rng, lens, quant=False, per_row=1.2, share=0.6):
    """Supplied stores of sequences of the given lengths: bp[x] and mp[(x, y)], x < y, as (rowptr, col, val).  The shortest
    sequence m carries per_row * len random pairs; sequence a carries the images of a share of them under k -> ceil(k *
    len[a] / len[m]) -- a column whose band in mp[a][m] is centred on k, so the two pairs and the two matches form a consensus
    base pair -- and random pairs of its own for the rest.  quant: bp from {0.25, 0.5, 0.75, 1}, mp from multiples of 1/8."""
    m = int(np.argmin(lens))
    Lm = lens[m]
    master = _pairs(rng, Lm, int(per_row * Lm))
    bp = []
    for a, La in enumerate(lens):
        if a == m:
            strong, extra = master, set()
        else:
            strong = {(-(-k * La // Lm), -(-l * La // Lm)) for (k, l) in sorted(master) if rng.random() < share}
            extra = _pairs(rng, La, int(per_row * La) - len(strong)) - strong
        bp.append(_bp_rows(rng, La, strong, extra, quant))
    mp = {(x, y): _band(rng, lens[x], lens[y], quant) for x in range(len(lens)) for y in range(x + 1, len(lens))}
    return bp, mp


def _sequences(rng, lens):
    return ["".join("ACGU"[int(c)] for c in rng.integers(0, 4, L)) for L in lens]


class Case:
    """sequences + supplied stores + the nodes to solve on them: (idx1, mask1, idx2, mask2[, p_x, p_y]) with idx into seqs"""

    def __init__(self, key, seqs, bp, mp, nodes, t_max, w_pct=0.0):
        self.key, self.seqs, self.bp, self.mp, self.nodes, self.t_max, self.w_pct = key, seqs, bp, mp, nodes, t_max, w_pct


def _seed(*key):
    return [1009] + [int(k) for k in key]


def shape_case(L1, L2, quant=False, t_max=None):
    """two sequences of L1 and L2 residues, single-row children; t_max: another iteration cap on the same inputs"""
    rng = np.random.default_rng(_seed(L1, L2, quant))
    bp, mp = stores(rng, [L1, L2], quant, *densities(L1, L2))
    node = (np.array([0], np.uint32), np.ones((1, L1), np.uint8), np.array([1], np.uint32), np.ones((1, L2), np.uint8))
    return Case(("shape", L1, L2, quant) + ((t_max,) if t_max else ()), _sequences(rng, [L1, L2]), bp, mp, [node], t_max or t_max_of(L1, L2))


def supplied_case(L1, L2):
    """a shape_case whose node brings its own base-pairing matrices (the --bp-update input): dense-ish, quantised"""
    rng = np.random.default_rng(_seed(L1, L2, 7))
    c = shape_case(L1, L2, True)
    ps = []
    for L in (L1, L2):
        p = (rng.integers(1, 5, (L, L)) / 4.0 * (rng.random((L, L)) < 0.1)).astype(np.float32)
        ps.append(np.triu(p, 4))
    # the consensus pairs need the same pairs on both sides of the diagonal map: carry a part of the short side's over
    s, l = (0, 1) if L1 <= L2 else (1, 0)
    Ls, Ll = (L1, L2)[s], (L1, L2)[l]
    for i, j in zip(*np.nonzero(ps[s])):
        if rng.random() < 0.5:
            ps[l][-(-int(i) * Ll // Ls), -(-int(j) * Ll // Ls)] = ps[s][i, j]
    c.key = ("supplied", L1, L2)
    c.nodes = [c.nodes[0] + (ps[0], ps[1])]
    return c


def _gapped_mask(rng, lens, L):
    """rows of lens[r] residues over L columns, gaps at random columns, no all-gap column"""
    while True:
        m = np.zeros((len(lens), L), np.uint8)
        for r, n in enumerate(lens):
            m[r, rng.choice(L, n, replace=False)] = 1
        if m.any(axis=0).all():
            return m


def multirow_case(nseq, L1, L2):
    """nseq sequences in two children of nseq // 2 and nseq - nseq // 2 rows over L1 and L2 columns, every row with up to 8 gaps;
    stores relaxed by the consistency transforms at weights 0.25 / 0.25 on both sides"""
    rng = np.random.default_rng(_seed(nseq, L1, L2, 3))
    n1 = nseq // 2
    lens = [int((L1 if r < n1 else L2) - rng.integers(0, 9)) for r in range(nseq)]
    lens[0], lens[n1] = L1 - 1, L2     # a row with one gap, and a row without
    bp, mp = stores(rng, lens, False, share=0.8)
    i1 = rng.permutation(n1).astype(np.uint32)                 # the rows of a child in no particular order
    i2 = (n1 + rng.permutation(nseq - n1)).astype(np.uint32)
    node = (i1, _gapped_mask(rng, [lens[i] for i in i1], L1), i2, _gapped_mask(rng, [lens[i] for i in i2], L2))
    return Case(("multirow", nseq, L1, L2), _sequences(rng, lens), bp, mp, [node], min(t_max_of(L1, L2), 12), w_pct=0.25)


# ---- the oracle's side: computed once per case and shared ----
_REFERENCE = {}


def oracle_params(oracle, case, **kw):
    return oracle.params(fold_model=1, align_model=2, w_pct_a=case.w_pct, w_pct_s=case.w_pct, t_max=case.t_max, **kw)


def oracle_pipeline(oracle, case, **kw):
    pl = oracle.pipeline(["s%d" % k for k in range(len(case.seqs))], case.seqs, oracle_params(oracle, case, **kw), bp=case.bp,
                         mp=lambda x, y: case.mp[(x, y)])
    pl.phase1()
    return pl


def reference(oracle, case):
    """the oracle's results of the case's nodes (read-only: shared between tests)"""
    if case.key not in _REFERENCE:
        pl = oracle_pipeline(oracle, case)
        outs = [pl.solve_node(*node) for node in case.nodes]
        pl.close()
        for o in outs:
            for k in ("x", "y", "z"):
                o[k].setflags(write=False)
        _REFERENCE[case.key] = outs
    return _REFERENCE[case.key]


_CASES = {}


def cached(make, *args):
    """the case make(*args), built once"""
    k = (make.__name__,) + args
    if k not in _CASES:
        _CASES[k] = make(*args)
    return _CASES[k]


# ---- the device's side ----
def open_context(cases):
    """A context that holds the sequences of all cases one after another with their stores (pairs across cases are empty),
    and per case its nodes with the sequence indices moved to the context's numbering."""
    from dafs_amd import capi
    seqs, bp, first = [], [], []
    for c in cases:
        first.append(len(seqs))
        seqs += c.seqs
        bp += c.bp
    owner = [k for k, c in enumerate(cases) for _ in c.seqs]
    nnz, rps, cols, vals = [], [], [], []
    for x in range(len(seqs)):
        for y in range(x + 1, len(seqs)):
            if owner[x] == owner[y]:
                f = first[owner[x]]
                rp, col, val = cases[owner[x]].mp[(x - f, y - f)]
            else:
                rp, col, val = np.zeros(len(seqs[x]) + 1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.float32)
            nnz.append(len(col)); rps.append(rp); cols.append(col); vals.append(val)
    ctx = capi.Context(0)
    ctx.set_sequences(seqs)
    ctx.set_bp(bp)
    ctx.set_mp(np.array(nnz, np.uint32), np.concatenate(rps), np.concatenate(cols), np.concatenate(vals))
    w = {c.w_pct for c in cases}
    assert len(w) == 1
    if w != {0.0}:
        ctx.consistency(w.pop(), cases[0].w_pct)
    nodes = [[(n[0] + np.uint32(f), n[1], n[2] + np.uint32(f)) + tuple(n[3:]) for n in c.nodes] for c, f in zip(cases, first)]
    return ctx, nodes


def device_params(case, **kw):
    from dafs_amd import capi
    return capi.dd_params(th_a=TH_A, th_s=TH_S, t_max=case.t_max, **kw)


def solve_on_device(case, **kw):
    ctx, nodes = open_context([case])
    try:
        return ctx.solve_nodes(nodes[0], device_params(case, **kw))
    finally:
        ctx.close()


OUTPUTS = ("x", "y", "z", "score", "ncbp", "iterations", "violated")


def first_difference(got, want, outputs=OUTPUTS):
    """None, or a sentence naming the first output in which two results of one node differ (score by its bytes)"""
    for k in outputs:
        g, w = got[k], want[k]
        if k in ("x", "y", "z"):
            if not np.array_equal(g, w):
                at = int(np.nonzero(np.asarray(g) != np.asarray(w))[0][0])
                return "%s differs first at column %d: %d, oracle %d (%d columns differ)" % (k, at, int(g[at]) - (1 << 32) * (g[at] == 0xFFFFFFFF),
                                                                                             int(w[at]) - (1 << 32) * (w[at] == 0xFFFFFFFF), int((np.asarray(g) != np.asarray(w)).sum()))
        elif k == "score":
            if np.float32(g).tobytes() != np.float32(w).tobytes():
                return "score differs: %r (0x%08x), oracle %r (0x%08x)" % (float(g), int(np.float32(g).view(np.uint32)), float(w), int(np.float32(w).view(np.uint32)))
        elif int(g) != int(w):
            return "%s differs: %d, oracle %d" % (k, int(g), int(w))
    return None


def assert_node(got, want, case, what="", outputs=OUTPUTS):
    d = first_difference(got, want, outputs)
    if d is not None:
        L1, L2 = len(want["x"]), len(want["y"])
        raise AssertionError("node %r%s (%d x %d columns, plan class (lds_flags, fold_fast) = %r, t_max %d): %s"
                             % (case.key, ", " + what if what else "", L1, L2, plan_class(L1, L2), case.t_max, d))


# ---- ties: do the DPs of the first iteration (multipliers all zero) meet equal candidates? ----
def averaged(oracle, case, node=0):
    """(p_x, p_y, p_z) as the node's solver sees them, from the oracle's stores: single-row children only"""
    n = case.nodes[node]
    assert len(n[0]) == 1 and len(n[2]) == 1 and case.w_pct == 0.0
    out = []
    for s in (int(n[0][0]), int(n[2][0])):
        rp, col, val = case.bp[s]
        L = len(rp) - 1
        p = np.zeros((L, L), np.float32)
        for i in range(L):
            p[i, col[rp[i]:rp[i + 1]]] = val[rp[i]:rp[i + 1]]
        out.append(p)
    if len(n) > 4:
        out = [np.asarray(n[4], np.float32), np.asarray(n[5], np.float32)]
    rp, col, val = case.mp[(int(n[0][0]), int(n[2][0]))]
    pz = np.zeros((len(rp) - 1, out[1].shape[0]), np.float32)
    for i in range(len(rp) - 1):
        pz[i, col[rp[i]:rp[i + 1]]] = val[rp[i]:rp[i + 1]]
    pz[pz <= np.float32(0.01)] = 0
    return out[0], out[1], pz


def alignment_ties(oracle, pz):
    """Cells of SparseNeedlemanWunsch::decode's table (multipliers zero, oracle/decoders.c) at which two of the three
    predecessors give the same float sum and that sum is the cell's value: the order of the comparisons decides the code."""
    L1, L2 = pz.shape
    env = oracle.nw_envelope(pz, TH_A).reshape(-1, 2)
    th = np.float32(TH_A)
    prev = np.zeros(L2 + 1, np.float32)
    low = np.float32(-np.finfo(np.float32).max)
    ties = 0
    for i in range(1, L1 + 1):
        cur = np.full(L2 + 1, low, np.float32)
        cur[0] = 0
        for k in range(max(int(env[i, 0]), 1), int(env[i, 1]) + 1):
            c = (np.float32(np.float32(prev[k - 1] + pz[i - 1, k - 1]) - th), prev[k], cur[k - 1])
            v = max(c)
            ties += v > 0 and sum(1 for a in c if a == v) > 1
            cur[k] = v
        prev = cur
    return ties


def folding_ties(p, w):
    """Cells of SparseNussinov::decode's table (multipliers zero, oracle/decoders.c) at which two candidates give the same
    float sum, that sum is the cell's (positive) value and one of the two closes or joins a pair (traceback code 3 or
    above): the order of the comparisons decides the structure."""
    L = p.shape[0]
    dp = np.zeros((L, L), np.float32)
    cand = [[] for _ in range(L)]
    th, w = np.float32(TH_S), np.float32(w)
    ties = 0
    for span in range(1, L):
        for i in range(L - span):
            j = i + span
            plain, pairing = [], []
            if i + 1 < j:
                plain.append(dp[i + 1, j])
            if i < j - 1:
                plain.append(dp[i, j - 1])
            if i + 1 < j - 1:
                s = np.float32(w * np.float32(p[i, j] - th))
                if s > 0:
                    cand[j].append((i, np.float32(dp[i + 1, j - 1] + s)))
                    pairing.append(cand[j][-1][1])
            pairing += [np.float32(dp[i, k - 1] + s) for k, s in cand[j] if i < k]
            if plain or pairing:
                v = max(plain + pairing)
                ties += v > 0 and v in pairing and (plain + pairing).count(v) > 1
                dp[i, j] = max(v, np.float32(0))
    return ties
