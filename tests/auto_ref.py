"""numpy and Python-integer restatement of the choice of thresholds by pseudo-expected accuracy, for
the tests.  Every cell counts as the integer q(p) = floor(clip(p, 0, 1) * 2^30) (the product is exact in float32); S is the
sum of q over the cells i < j of the unmasked matrix, T of a structure the sum of q over its pairs, n their number, and
(Ta, na) beats (Tb, nb) exactly when Ta (nb 2^30 + S) > Tb (na 2^30 + S) in Python's unbounded integers.  The masks are the
literal rule of levels_ref.py and the decodes the oracle's SparseNussinov.  Also the hand-made cases both test files use."""
import numpy as np

import levels_ref as lref

NONE, FREE = lref.NONE, lref.FREE
GAMMAS = (1, 2, 4, 8, 16, 32)
ONE = 2 ** 30


def candidates(gammas=GAMMAS):
    """the thresholds of the weights, as the command line converts -G"""
    return np.array([np.float32(1.0 / (1.0 + g)) for g in gammas], np.float32)


def q(p):
    return np.floor(np.clip(p, 0, 1).astype(np.float32) * np.float32(2 ** 30)).astype(np.uint64)


def total(p):
    """S: over the cells right of the diagonal"""
    p = np.asarray(p, np.float32)
    return int(np.triu(q(p), 1).sum(dtype=np.uint64)) if p.shape[0] else 0


def value(pk, ss):
    """(T, n) of the structure ss on the matrix pk it was decoded from"""
    prs = lref.pairs_of(ss)
    return sum(int(q(pk[i, j])) for i, j in prs), len(prs)


def beats(a, b, S):
    return a[0] * (b[1] * ONE + S) > b[0] * (a[1] * ONE + S)


def f_of(t, n, S):
    den = n * ONE + S
    return 2 * t / den if den else 0.0


class Result:
    pass


def decode(oracle, p, cand, nlevels):
    """The contract on the dense matrix p.  Returns a Result: scores[K] float32, ss, level, chosen[K], sum_p, tp[K], npairs[K],
    cand_tp / cand_pairs [K][C] (Python integers; 0 for levels that are not decoded), launched (the levels decoded),
    per_level (the kept structure of every decoded level) and cand_ss (per decoded level the C structures)."""
    p = np.ascontiguousarray(p, np.float32)
    cand = [np.float32(c) for c in cand]
    L, K, C = p.shape[0], nlevels, len(cand)
    r = Result()
    r.scores = np.zeros(K, np.float32)
    r.ss = np.full(L, NONE, np.uint32)
    r.level = np.full(L, FREE, np.uint8)
    r.chosen = [NONE] * K
    r.sum_p = total(p)
    r.tp, r.npairs = [0] * K, [0] * K
    r.cand_tp = [[0] * C for _ in range(K)]
    r.cand_pairs = [[0] * C for _ in range(K)]
    r.per_level, r.cand_ss, r.launched = [], [], 0
    base = (0, 0)
    for k in range(K if L else 0):
        pk = p if k == 0 else lref.masked(p, r.per_level)
        decs = [oracle.nussinov(pk, None, float(c)) for c in cand]
        vals = [value(pk, ss) for _, ss in decs]
        r.launched += 1
        r.cand_ss.append([ss for _, ss in decs])
        r.cand_tp[k] = [v[0] for v in vals]
        r.cand_pairs[k] = [v[1] for v in vals]
        with_base = [(base[0] + t, base[1] + n) for t, n in vals]
        best = 0
        for c in range(1, C):  # the first that no earlier one equals or beats
            if beats(with_base[c], with_base[best], r.sum_p):
                best = c
        if not beats(with_base[best], base, r.sum_p):
            r.per_level.append(np.full(L, NONE, np.uint32))
            break  # an empty level: the higher ones are empty too, and are not decoded
        r.chosen[k] = best
        r.tp[k], r.npairs[k] = vals[best]
        r.scores[k] = np.float32(decs[best][0])
        r.per_level.append(decs[best][1])
        base = with_base[best]
        for i, j in lref.pairs_of(decs[best][1]):
            r.ss[i] = j
            r.level[i] = r.level[j] = k
    r.kept = [c for c in r.chosen if c != NONE]
    r.f = f_of(sum(r.tp), sum(r.npairs), r.sum_p)
    return r


def same(got, want):
    """(scores, ss, level, choice) of the library against a Result, everything to the bit"""
    scores, ss, level, a = got
    K = len(want.chosen)
    return (np.asarray(scores, np.float32).tobytes() == want.scores.tobytes() and ss.tobytes() == want.ss.tobytes()
            and level.tobytes() == want.level.tobytes() and [int(c) for c in a.chosen] == want.chosen and a.sum_p == want.sum_p
            and [int(t) for t in a.tp] == want.tp and [int(n) for n in a.npairs] == want.npairs
            and [[int(t) for t in row] for row in a.cand_tp] == want.cand_tp
            and [[int(n) for n in row] for row in a.cand_pairs] == want.cand_pairs and len(a.chosen) == K)


def _matrix(L, cells):
    p = np.zeros((L, L), np.float32)
    for (i, j), v in cells.items():
        p[i, j] = v
    return p


class Case:
    def __init__(self, name, p, gammas, nlevels, chosen, text):
        self.name, self.p, self.gammas, self.nlevels, self.chosen, self.text = name, p, gammas, nlevels, chosen, text
        self.cand = candidates(gammas)


def hand_cases():
    """The expected choice (the candidate's index per level) and the bracket string written out."""
    by_name = {c.name: c for c in lref.hand_cases()}
    c = []
    # a strong helix of five pairs at 0.9 and scattered cells at 0.15 that nest around and beside it.  At the thresholds 1/2,
    # 1/3 and 1/5 the decode is the helix, T = 5 q(0.9), n = 5; from 1/9 on the weak cells (0, 29), (1, 28), (20, 26) and
    # (21, 25) come in: T grows by 4 q(0.15) = 0.6 while n grows by 4, which lowers F.  The three first are equal; the first wins.
    helix = {(4 + k, 18 - k): 0.9 for k in range(5)}
    weak = {(0, 29): 0.15, (1, 28): 0.15, (20, 26): 0.15, (21, 25): 0.15}
    c.append(Case("helix-and-scatter", _matrix(30, {**helix, **weak}), GAMMAS, 1, [0], "....(((((.....)))))..........."))
    # nothing reaches the lowest threshold 1/33: every candidate decodes nothing, and nothing is kept
    c.append(Case("nothing", _matrix(12, {(0, 8): 0.02, (2, 7): 0.03}), GAMMAS, 2, [NONE, NONE], "............"))
    # both candidates decode the one pair: equal values, the higher threshold (the earlier in the list) wins
    c.append(Case("equal-values", _matrix(8, {(1, 6): 0.8}), (1, 4), 1, [0], ".(....)."))
    # lowering the threshold is worth it: at 1/2 only (0, 9) at 0.6 pairs, F = 2 * 0.6 / (1 + 1.5) = 0.48; at 1/3 (1, 8) at
    # 0.45 and (2, 7) at 0.45 join it, F = 2 * 1.5 / (3 + 1.5) = 0.667
    c.append(Case("lower-is-better", _matrix(10, {(0, 9): 0.6, (1, 8): 0.45, (2, 7): 0.45}), (1, 2), 1, [1], "(((....)))"))
    # the 12-column H-type of test_levels_cpu.py: stem B at 0.8 crosses stem A at 0.9, and level 1 raises F from
    # 2 * 1.8 / (2 + 3.4) to 2 * 3.4 / (4 + 3.4): it is kept, each level at the highest threshold
    c.append(Case("h-type-12", by_name["h-type-12"].p, GAMMAS, 2, [0, 0], "((.[[))...]]"))
    # the strong cell that crosses nothing: cells (0, 6) = 0.9, (8, 12) = 0.45, (3, 10) = 0.3, so S = 1.65.
    # Level 0 at threshold 1/2: only (0, 6) pairs; T = 0.9, n = 1, F = 2 * 0.9 / (1 + 1.65) = 0.679.
    # Level 0 at 1/3 and at every lower threshold: (0, 6) and (8, 12); T = 1.35, n = 2, F = 2 * 1.35 / (2 + 1.65) = 0.740.
    # (3, 10) crosses (0, 6) and is worth less, so no threshold pairs it at level 0.  0.740 > 0.679: level 0 takes candidate 1
    # (1/3), the first of the equal ones.
    # Level 1: (3, 10) is the only cell left (it crosses (0, 6)); it pairs from threshold 1/5 on.  With it T = 1.65, n = 3,
    # F = 2 * 1.65 / (3 + 1.65) = 0.710 < 0.740: level 1 is decoded and comes out empty
    c.append(Case("crosses-nothing", by_name["crosses-nothing"].p, GAMMAS, 2, [1, NONE], "(.....).(...)."))
    return c
