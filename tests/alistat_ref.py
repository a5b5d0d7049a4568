"""Plain-Python restatement of DESIGN.md section 18 "Alignment statistics": the yardstick of test_alistat_cpu.py and
test_alistat_gpu.py.  Integer counts, the cross-multiplied order, the walk of the non-redundant subset and the weights in the
stated order of operations; Python's float is the IEEE double of the definitions and every operation below is a single one."""
import math

NONE = 0xFFFFFFFF


def code(ch):
    """the cell code of one character; ValueError for anything that is neither a letter nor a gap"""
    if ch in "Aa":
        return 0
    if ch in "Cc":
        return 1
    if ch in "Gg":
        return 2
    if ch in "UuTt":
        return 3
    if ("A" <= ch <= "Z") or ("a" <= ch <= "z"):
        return 4
    if ch in "-.":
        return 5
    raise ValueError("not a cell: %r" % ch)


def cells(rows):
    return [[code(ch) for ch in row] for row in rows]


def _used(length, use):
    return [c for c in range(length) if use is None or use[c]]


def counts(cell, use=None):
    """(res[n], ident[n][n], aligned[n][n]) over the used columns; ValueError for a row without residues"""
    n = len(cell)
    cols = _used(len(cell[0]), use)
    res = [sum(1 for c in cols if row[c] <= 4) for row in cell]
    if any(x == 0 for x in res):
        raise ValueError("a row without residues")
    ident = [[0] * n for _ in range(n)]
    aligned = [[0] * n for _ in range(n)]
    used = [[row[c] for c in cols] for row in cell]
    for r in range(n):
        for s in range(r, n):  # both counts are symmetric
            a = i = 0
            for x, y in zip(used[r], used[s]):
                if x <= 4 and y <= 4:
                    a += 1
                    if x == y and x <= 3:
                        i += 1
            aligned[r][s] = aligned[s][r] = a
            ident[r][s] = ident[s][r] = i
    return res, ident, aligned


def more_identical(i1, d1, i2, d2):
    return i1 * d2 > i2 * d1  # Python integers: exact


def nearest(res, ident, cand=None):
    """(nearest[n], nearest_ident[n], nearest_den[n]); NONE, 0, 0 without a candidate"""
    n = len(res)
    out = []
    for r in range(n):
        best = None
        for s in range(n):
            if s == r or (cand is not None and not cand[s]):
                continue
            i, d = ident[r][s], min(res[r], res[s])
            if best is None or more_identical(i, d, best[1], best[2]):  # a tie keeps the smaller s
                best = (s, i, d)
        out.append(best if best is not None else (NONE, 0, 0))
    return [b[0] for b in out], [b[1] for b in out], [b[2] for b in out]


def redundant(i, d, t):
    return float(i) >= t * float(d)


def red_matrix(res, ident, t):
    n = len(res)
    return [[r != s and redundant(ident[r][s], min(res[r], res[s]), t) for s in range(n)] for r in range(n)]


def red_bits(red):
    """the bit matrix as rows of 32-bit words"""
    n = len(red)
    words = (n + 31) // 32
    out = [[0] * words for _ in range(n)]
    for r in range(n):
        for s in range(n):
            if red[r][s]:
                out[r][s // 32] |= 1 << (s % 32)
    return out


def nr_select(red, rank, forced=None):
    """(kept[n], by[n]) of the walk in rank order"""
    n = len(red)
    if sorted(rank) != list(range(n)):
        raise ValueError("not a permutation")
    kept = [False] * n
    by = [NONE] * n
    keepers = []
    for r in rank:
        remover = NONE
        if forced is None or not forced[r]:
            for q in keepers:
                if red[r][q]:
                    remover = q
                    break
        kept[r] = remover == NONE
        by[r] = remover
        if kept[r]:
            keepers.append(r)
    return kept, by


def weights(cell, use=None):
    n = len(cell)
    length = len(cell[0])
    if n == 1:
        return [1.0]
    k = [[sum(1 for row in cell if row[c] == a) for a in range(5)] for c in range(length)]
    t = [sum(1 for a in range(5) if k[c][a] > 0) for c in range(length)]
    u = []
    for row in cell:
        v = 0.0
        res = 0
        for c in _used(length, use):
            if row[c] <= 4:
                v += 1.0 / float(t[c] * k[c][row[c]])
                res += 1
        u.append(v / float(res))
    total = 0.0
    for x in u:
        total += x
    return [(x * float(n)) / total for x in u]


def v_sums(cell, use=None):
    """the v_r of the weights alone (the known answer of the issue)"""
    length = len(cell[0])
    k = [[sum(1 for row in cell if row[c] == a) for a in range(5)] for c in range(length)]
    t = [sum(1 for a in range(5) if k[c][a] > 0) for c in range(length)]
    out = []
    for row in cell:
        v = 0.0
        for c in _used(length, use):
            if row[c] <= 4:
                v += 1.0 / float(t[c] * k[c][row[c]])
        out.append(v)
    return out


def summary(res, ident):
    """(average, minimum, maximum) pid over r < s; NaN for one row"""
    n = len(res)
    if n == 1:
        return (math.nan, math.nan, math.nan)
    total = 0.0
    lo = hi = None
    for r in range(n):
        for s in range(r + 1, n):
            i, d = ident[r][s], min(res[r], res[s])
            total += float(i) / float(d)
            if lo is None or more_identical(lo[0], lo[1], i, d):
                lo = (i, d)
            if hi is None or more_identical(i, d, hi[0], hi[1]):
                hi = (i, d)
    return (total / float(n * (n - 1) // 2), float(lo[0]) / float(lo[1]), float(hi[0]) / float(hi[1]))
