"""Cases and float32 restatements of the --bp-update tests (test_bp_update_cpu.py, test_bp_update_gpu.py): hand-made gapped
alignments with a hand-made nested structure, for Context.update_basepairing / the multi-row average of
Context.consensus_structure against orc_pipeline_update_basepairing / orc_pipeline_average_basepairing.  Deterministic, plain
numpy, no device.  Test infrastructure only -- nothing under dafs_amd/ imports this."""
import ctypes as C
import os

import numpy as np

NONE = 0xFFFFFFFF
F32 = np.float32
CUTOFF = 0.01  # a double in the reference: `p[i][j] <= CUTOFF` compares in double (dafs.cpp:602, :706)
PAIRS = ("AU", "UA", "GC", "CG", "GU", "UG")  # what CONTRAfold can pair
# stems mostly of G-C pairs between loops poor in G, so that the rows' free folds agree on them and the plain average of
# mid and wide decodes to pairs at TH
PAIR_P = (0.05, 0.05, 0.4, 0.4, 0.05, 0.05)
LOOP_P = (0.5, 0.2, 0.05, 0.25)
TH = 0.2  # the threshold of the two decodes around an update
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Case:
    """seqs: the context's sequences; idx [n]: the sequence of each row; mask [n, L]; ss [L]: ss[i] = j at the left column of
    a pair only, NONE elsewhere (the decoders' convention); pairs: the same as (i, j) tuples"""

    def __init__(self, key, seqs, idx, mask, pairs):
        self.key = key
        self.seqs = seqs
        self.idx = np.array(idx, np.uint32)
        self.mask = np.ascontiguousarray(mask, np.uint8)
        self.n, self.L = self.mask.shape
        self.pairs = sorted(pairs)
        self.ss = np.full(self.L, NONE, np.uint32)
        for i, j in self.pairs:
            self.ss[i] = j

    def __repr__(self):
        return "Case(%s)" % self.key


def _stems(*stems):
    """(first left column, last right column, pairs) per stem -> the pairs (i, j), outermost first"""
    return [(i + t, j - t) for i, j, k in stems for t in range(k)]


def _nested(pairs):
    cols = [c for p in pairs for c in p]
    return len(set(cols)) == len(cols) and not any(a < c < b < d for a, b in pairs for c, d in pairs)


def _row(rng, L, gaps, pairs, complementary=True):
    """(mask row, residues): a residue in every column but gaps; random residues, the right partner of every pair whose two
    columns the row holds made complementary to the left one (complementary=False: left as drawn)"""
    m = np.ones(L, np.uint8)
    m[list(gaps)] = 0
    res = [str(c) for c in rng.choice(list("ACGU"), L, p=LOOP_P if complementary else None)]
    for i, j in pairs:
        if complementary and m[i] and m[j]:
            res[i], res[j] = PAIRS[int(rng.choice(len(PAIRS), p=PAIR_P))]
    return m, "".join(res[c] for c in range(L) if m[c])


def _case(key, seed, L, idx, rows, pairs, ss_pairs=None):
    """rows: per row (gap columns, complementary); the context holds two sequences of no row in front of the rows' own, which
    stand in it in the order of their sequence index"""
    assert _nested(pairs) and all(0 <= i < j < L for i, j in pairs)
    rng = np.random.default_rng(seed)
    n = len(rows)
    assert sorted(idx) == list(range(2, n + 2)) and all(idx[r] != r for r in range(n)) and list(idx) != sorted(idx)
    seqs = ["".join(rng.choice(list("ACGU"), k)) for k in (23, 31)] + [None] * n
    mask = np.zeros((n, L), np.uint8)
    for r, (gaps, comp) in enumerate(rows):
        mask[r], seqs[idx[r]] = _row(rng, L, gaps, pairs, comp)
    return Case(key, seqs, idx, mask, pairs if ss_pairs is None else ss_pairs)


def _but(L, keep):
    return [c for c in range(L) if c not in set(keep)]


def build_cases():
    cases = {}
    # small: three stems side by side, the first and the last column paired.  Row 1 lacks column 11 (the pair (1, 11)), row 2
    # columns 16 and 38 (two pairs); the last row holds two residues, column 0 (whose partner it lacks) and a loop column.
    p = _stems((0, 12, 4), (14, 25, 4), (27, 39, 4))
    rows = [((), True), ((11, 20, 33), True), ((4, 5, 6, 16, 19, 20, 38), True), ((), True), (_but(40, (0, 33)), True)]
    cases["small"] = _case("small", 11, 40, [4, 6, 5, 2, 3], rows, p)
    cases["none"] = _case("none", 11, 40, [4, 6, 5, 2, 3], rows, p, ss_pairs=[])
    # mid: rows of 64, 65 and 63 residues; the outer stem closes at columns 0 and 70.  Row 1 has its gaps in loops only.
    p = _stems((0, 70, 5), (8, 30, 6), (34, 62, 7))
    rows = [((5, 6, 12, 18, 19, 45, 64), True), ((16, 17, 20, 47, 48, 65), True), ((7, 31, 32, 33, 36, 50, 63, 70), True)]
    cases["mid"] = _case("mid", 12, 71, [4, 2, 3], rows, p)
    # wide: four stems over 400 columns.  Row 1 lacks every column strictly inside the second stem's span (101 .. 229), so
    # that its pair (100, 230) joins neighbours; row 2 keeps random residues; rows 3 and 4 are short.
    p = _stems((5, 95, 8), (100, 230, 6), (240, 330, 8), (335, 398, 7))
    gaps1 = list(range(101, 230)) + [0, 1, 40, 41, 42, 50, 280, 281, 282, 283, 290, 360, 361, 399]
    gaps2 = [242] + list(range(20, 80)) + list(range(110, 130)) + list(range(140, 160)) + list(range(255, 299))  # 242: the pair (242, 328)
    keep3 = list(range(335, 342)) + list(range(392, 399)) + list(range(350, 380)) + list(range(5, 13)) + list(range(200, 211))
    rows = [((), True), (gaps1, True), (gaps2, False), (_but(400, keep3), True), (_but(400, (3, 100, 150, 231, 399)), True)]
    cases["wide"] = _case("wide", 13, 400, [4, 6, 5, 2, 3], rows, p)
    want = {"small": [40, 37, 33, 40, 2], "none": [40, 37, 33, 40, 2], "mid": [64, 65, 63], "wide": [400, 257, 255, 63, 5]}
    for k, c in cases.items():
        assert [int(v) for v in c.mask.sum(1)] == want[k] == [len(c.seqs[s]) for s in c.idx], k
    return cases


CASES = build_cases()
KEYS = ["small", "mid", "wide", "none"]


# ---- the folds, shared between the tests of a run ----
_folds = {}


def fold(orc, seq, con=None):
    """orc_fold_calculate(seq, con, 0.01): (rowptr, col, val) of the pairs with p > 0.01 (read-only: cached)"""
    key = (seq, con)
    if key not in _folds:
        L = len(seq)
        cap = L * (L + 1) // 2 + 1
        rp = np.zeros(L + 1, np.uint32); col = np.zeros(cap, np.uint32); val = np.zeros(cap, np.float32)
        n = orc.lib.orc_fold_calculate(seq.encode(), L, None if con is None else con.encode(), C.c_float(0.01), rp.ctypes.data, col.ctypes.data,
                                       val.ctypes.data)
        assert n >= 0, (seq, con)
        out = (rp, col[:n].copy(), val[:n].copy())
        for a in out:
            a.flags.writeable = False
        _folds[key] = out
    return _folds[key]


def free_rows(orc, case):
    """the unconstrained rows of every sequence of the context: what both sides of the plain average are supplied with"""
    return [fold(orc, s) for s in case.seqs]


def oracle_pipeline(orc, case, with_rows=True):
    names = ["s%d" % k for k in range(len(case.seqs))]
    return orc.pipeline(names, case.seqs, orc.params(fold_model=1), bp=free_rows(orc, case) if with_rows else None)


# ---- the restatement: DAFS::average_basepairing_probability (dafs.cpp:561-607) and DAFS::update_basepairing_probability
# (:609-712), use_alifold == false, one level of brackets ----
def brackets(ss):
    """Fold::Decoder::make_brackets for one level: '(' at i and ')' at ss[i]"""
    s = ["."] * len(ss)
    for i, j in enumerate(ss):
        if j != NONE:
            s[i], s[int(j)] = "(", ")"
    return "".join(s)


def constraint(mask_row, ss, text, rule=None):
    """the string of one row, :637-653; rule "free": all '?', "dot": the '.' branch taken for '('"""
    rev = np.full(len(mask_row), -1, np.int64)
    rev[np.flatnonzero(mask_row)] = np.arange(int(mask_row.sum()))
    con = ["?"] * int(mask_row.sum())
    for i in range(len(mask_row)):
        if rule != "free" and ss[i] != NONE and rev[i] >= 0 and rev[int(ss[i])] >= 0:
            if text[i] == "(" and rule != "dot":
                con[rev[i]], con[rev[int(ss[i])]] = "(", ")"
            else:
                con[rev[i]] = con[rev[int(ss[i])]] = "."
    return "".join(con)


def _average(case, rows, rule=None):
    """p[idx[i]][idx[j]] += val / N over the rows in order, float32 throughout; then the cut-off on the upper triangle"""
    L, n = case.L, case.n
    p = np.zeros((L, L), F32)
    div = F32(n + 1 if rule == "n+1" else n)
    order = range(n - 1, -1, -1) if rule == "reverse" else range(n)
    for r in order:
        rp, col, val = rows[r]
        at = np.flatnonzero(case.mask[r])
        assert len(rp) == len(at) + 1
        i = at[np.repeat(np.arange(len(at)), np.diff(rp.astype(np.int64)))]
        j = at[col]
        assert len(set(zip(i.tolist(), j.tolist()))) == len(i)  # one addend per cell and row
        p[i, j] = p[i, j] + (val / div).astype(F32)
    up = np.triu(np.ones((L, L), bool), 1)
    p[up & (p.astype(np.float64) <= CUTOFF)] = 0
    return p


def restated_average(orc, case, rule=None):
    return _average(case, [fold(orc, case.seqs[s]) for s in case.idx], rule)


def row_sequence(case, r, rule=None):
    """the residues row r is folded as; rule "row": sequence r of the context instead of idx[r], cut or filled up with A to
    the row's residues"""
    if rule != "row":
        return case.seqs[case.idx[r]]
    k = int(case.mask[r].sum())
    return (case.seqs[r] + "A" * k)[:k]


def restated_update(orc, case, ss=None, rule=None):
    ss = case.ss if ss is None else ss
    text = brackets(ss)
    rows = [fold(orc, row_sequence(case, r, rule), constraint(case.mask[r], ss, text, rule)) for r in range(case.n)]
    return _average(case, rows, rule)


RULES = ["free", "row", "reverse", "dot", "n+1"]


# ---- whole runs on which both flags change the oracle's output ----
def whole_run_inputs():
    """(key, FASTA text) of the inputs the command-line test adds to its family"""
    from dafs_amd import synth
    with open(os.path.join(GOLDEN, "RF00005_0.fa")) as f:
        trna = f.read()
    return [("RF00005_0", trna), ("structured", synth.to_fasta(synth.structured_family_set(5, 60, stems=2, seed=7, indel=0.1)))]
