"""numpy restatement of the level-by-level decode, for the tests: the literal definitions, by brute
force.  Level 0 is the oracle's SparseNussinov on P at th[0]; level k >= 1 the same decoder at th[k] on P_k, where
P_k(i, j) = P(i, j) when (a) i and j are unpaired in every lower level and (b) every lower level has a pair that crosses
(i, j), and 0 otherwise.  Also the hand-made cases both test files use."""
import numpy as np

NONE = 0xFFFFFFFF
FREE = 0xFF


def pairs_of(ss):
    return [(i, int(j)) for i, j in enumerate(ss) if j != NONE]


def crosses(a, b, i, j):
    """definition (b): the pair (a, b) crosses the cell (i, j)"""
    return a < i < b < j or i < a < j < b


def masked(p, lower):
    """P_k from P and the structures of the levels below k: definitions (a) and (b) on every cell (numpy over the cells, a
    loop over the pairs)"""
    L = p.shape[0]
    i, j = np.meshgrid(np.arange(L), np.arange(L), indexing="ij")
    keep = i < j
    for ss in lower:
        crossed = np.zeros((L, L), bool)
        for a, b in pairs_of(ss):
            keep &= (i != a) & (i != b) & (j != a) & (j != b)                      # (a)
            crossed |= ((a < i) & (i < b) & (b < j)) | ((i < a) & (a < j) & (j < b))  # (b), as crosses() states it
        keep &= crossed
    return np.where(keep, p, np.float32(0)).astype(np.float32)


def decode(oracle, p, ths):
    """(scores[K] float32, merged ss, level, per-level ss list) of the dense matrix p"""
    p = np.ascontiguousarray(p, np.float32)
    L, K = p.shape[0], len(ths)
    scores = np.zeros(K, np.float32)
    merged = np.full(L, NONE, np.uint32)
    level = np.full(L, FREE, np.uint8)
    per_level = []
    for k in range(K):
        if L == 0:
            per_level.append(np.zeros(0, np.uint32))
            continue
        pk = p if k == 0 else masked(p, per_level)
        s, ss = oracle.nussinov(pk, None, float(np.float32(ths[k])))
        scores[k] = s
        per_level.append(ss)
        for i, j in pairs_of(ss):
            assert merged[i] == NONE and level[i] == FREE and level[j] == FREE  # constraint 1, or the restatement is wrong
            merged[i] = j
            level[i] = level[j] = k
    return scores, merged, level, per_level


def enclosers(ss):
    """enc[c]: the left column of the innermost pair of the nested structure ss that strictly encloses c, or NONE"""
    L = len(ss)
    enc = np.full(L, NONE, np.uint32)
    for c in range(L):
        best = None
        for a, b in pairs_of(ss):
            if a < c < b and (best is None or a > best):
                best = a
        if best is not None:
            enc[c] = best
    return enc


def brackets(ss, level):
    out = ["."] * len(ss)
    for i, j in pairs_of(ss):
        out[i], out[j] = "([{<"[level[i]], ")]}>"[level[i]]
    return "".join(out)


def tree_score(p, ss, th):
    """the decoder's score of the nested structure ss in float32, summed in the decoder's own order: a pair closing an
    interval adds its p - th to the inside; otherwise the interval's last column closes a pair (k, j), and the value is
    [i, k - 1] + ([k + 1, j - 1] + s_kj)"""
    th = np.float32(th)
    left = {j: i for i, j in pairs_of(ss)}

    def f(i, j):
        while i <= j and ss[i] == NONE and i not in left:
            i += 1
        while i <= j and ss[j] == NONE and j not in left:
            j -= 1
        if i >= j:
            return np.float32(0)
        k = left[j]
        s = np.float32(np.float32(p[k, j]) - th)
        inner = np.float32(f(k + 1, j - 1) + s)
        return inner if k == i else np.float32(f(i, k - 1) + inner)

    return f(0, len(ss) - 1)


def _matrix(L, cells):
    p = np.zeros((L, L), np.float32)
    for (i, j), v in cells.items():
        p[i, j] = v
    return p


def _ss(L, pairs):
    ss = np.full(L, NONE, np.uint32)
    for i, j in pairs:
        ss[i] = j
    return ss


def _level(L, by_level):
    lv = np.full(L, FREE, np.uint8)
    for k, prs in enumerate(by_level):
        for i, j in prs:
            lv[i] = lv[j] = k
    return lv


class Case:
    def __init__(self, name, L, cells, ths, by_level, text):
        self.name, self.p, self.ths = name, _matrix(L, cells), ths
        self.ss = _ss(L, [pr for prs in by_level for pr in prs])
        self.level = _level(L, by_level)
        self.by_level, self.text = by_level, text


def hand_cases():
    """Structure and levels written out.  The decoder pairs (i, j) only when j - i >= 3, so the smallest knot with that rule
    spans seven columns; at four columns, (0, 2) and (1, 3) are too short to pair at all."""
    c = []
    # L = 4, cells (0,2) and (1,3): the smallest crossing there is, but both spans are under three and the decoder pairs
    # neither (nussinov.cpp:327) -- nothing at either level
    c.append(Case("smallest-4", 4, {(0, 2): 0.9, (1, 3): 0.8}, (0.2, 0.2), [[], []], "...."))
    # the smallest knot the decoder does return: two crossing cells of span four
    c.append(Case("smallest-knot", 7, {(0, 4): 0.9, (2, 6): 0.8}, (0.2, 0.2), [[(0, 4)], [(2, 6)]], "(.[.).]"))
    # a 12-column H-type: stem A (0,6) (1,5), stem B (3,11) (4,10)
    c.append(Case("h-type-12", 12, {(0, 6): 0.9, (1, 5): 0.9, (3, 11): 0.8, (4, 10): 0.8}, (0.2, 0.2),
                  [[(0, 6), (1, 5)], [(3, 11), (4, 10)]], "((.[[))...]]"))
    # a kissing hairpin: two hairpins (0,7) (1,6) and (10,17) (11,16) at level 0, their loops paired (3,14) (4,13) at level 1
    c.append(Case("kissing", 18, {(0, 7): 0.9, (1, 6): 0.9, (10, 17): 0.9, (11, 16): 0.9, (3, 14): 0.7, (4, 13): 0.7}, (0.2, 0.2),
                  [[(0, 7), (1, 6), (10, 17), (11, 16)], [(3, 14), (4, 13)]], "((.[[.))..((.]].))"))
    # a strong cell that crosses nothing: (8,12) is under th[0] and well over th[1], but lies beside level 0's (0,6); it
    # must be absent from level 1, which unmasked would prefer it to (3,10), the cell that crosses it and (0,6)
    c.append(Case("crosses-nothing", 14, {(0, 6): 0.9, (8, 12): 0.45, (3, 10): 0.3}, (0.5, 0.1),
                  [[(0, 6)], [(3, 10)]], "(..[..)...]..."))
    # K = 3: (2,15) crosses level 0's (0,5) but encloses level 1's (3,12): absent from level 2, which takes (4,14), the cell
    # that crosses both (unmasked, level 2 would take both cells: they nest)
    c.append(Case("k3", 16, {(0, 5): 0.9, (3, 12): 0.6, (2, 15): 0.4, (4, 14): 0.3}, (0.7, 0.5, 0.1),
                  [[(0, 5)], [(3, 12)], [(4, 14)]], "(..[{)......].}."))
    # a cell whose column is taken by a lower level: (5,11) is stronger than (2,9), but column 5 is level 0's
    c.append(Case("column-taken", 12, {(0, 5): 0.9, (5, 11): 0.85, (2, 9): 0.6}, (0.2, 0.2),
                  [[(0, 5)], [(2, 9)]], "(.[..)...].."))
    return c
