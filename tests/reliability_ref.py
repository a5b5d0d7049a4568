"""The alignment-reliability definitions of DESIGN.md ("Alignment reliability") restated in plain Python from host arrays:
the yardstick for dafs_hip_alignment_reliability.  Every sum is a Python float (IEEE double) loop in the stated order;
probabilities are widened from float32."""
import numpy as np

NONE = 0xFFFFFFFF


def _lookup(cols, vals, j):
    v = np.float32(0.0)
    for c, p in zip(cols, vals):
        if int(c) == j:
            v = p
    return float(v)


def _mass(vals):
    s = 0.0
    for p in vals:
        s += float(np.float32(p))
    return s


def restate(seq, mask, ss, mp_row, bp_row):
    """seq[n], mask[n, L] (1 = residue), ss[L] or None.  mp_row(x, y, i) -> (cols, vals) of row i of mp[x][y];
    bp_row(x, i) -> (cols, vals) of row i of bp[x].  Returns the dict Context.alignment_reliability returns."""
    seq = [int(s) for s in seq]
    mask = np.asarray(mask, bool)
    n, L = mask.shape
    order = sorted(range(n), key=lambda r: seq[r])
    pos = []  # per row: column -> residue index or None
    for r in range(n):
        p, k = [None] * L, 0
        for c in range(L):
            if mask[r, c]:
                p[c] = k
                k += 1
        pos.append(p)
    rel = {}
    for r in order:
        x = seq[r]
        vals = []
        for c in range(L):
            i = pos[r][c]
            if i is None:
                continue
            acc = 0.0
            for q in order:
                if q == r:
                    continue
                cols, vv = mp_row(x, seq[q], i)
                j = pos[q][c]
                if j is not None:
                    term = _lookup(cols, vv, j)
                else:
                    term = max(0.0, 1.0 - _mass(vv))
                acc += term
            vals.append(acc / float(n - 1) if n > 1 else 1.0)
        rel[r] = np.array(vals, np.float64)
    col = np.zeros(L, np.float64)
    pair = np.zeros(L, np.float64)
    rows = np.zeros(L, np.uint32)
    for c in range(L):
        s, K = 0.0, 0
        for r in order:
            i = pos[r][c]
            if i is not None:
                s += float(rel[r][i])
                K += 1
        col[c] = s / float(K) if K else 0.0
        if ss is not None and int(ss[c]) != NONE:
            c2 = int(ss[c])
            ps, pc = 0.0, 0
            for r in order:
                i, j = pos[r][c], pos[r][c2]
                if i is None or j is None:
                    continue
                cols, vv = bp_row(seq[r], i)
                ps += _lookup(cols, vv, j)
                pc += 1
            pair[c] = ps / float(pc) if pc else 0.0
            rows[c] = pc
    total, cnt = 0.0, 0
    for r in order:
        for v in rel[r]:
            total += float(v)
            cnt += 1
    return dict(residue=np.concatenate([rel[r] for r in range(n)]), col=col, pair=pair, pair_rows=rows,
                expected_accuracy=total / float(cnt))


def dict_stores(mp, bp=None):
    """Accessors over hand-built stores: mp[(x, y)] = list of rows (cols, vals) of mp[x][y] (missing pair: no entries),
    bp[x] = list of rows of bp[x]"""
    def mp_row(x, y, i):
        rows = mp.get((x, y))
        return rows[i] if rows is not None else ((), ())

    def bp_row(x, i):
        return bp[x][i]
    return mp_row, bp_row


def context_stores(ctx, mp_relaxed, bp_relaxed):
    """Accessors over a context's stores, fetched once (Context.mp / Context.bp); mp[x][y] with x > y is the transposed
    half of the pair (y, x)"""
    st = ctx.mp(mp_relaxed)
    at = {(int(st.pair_x[p]), int(st.pair_y[p])): p for p in range(len(st))}
    bps = ctx.bp(bp_relaxed)

    def mp_row(x, y, i):
        if x < y:
            rp, col, val = st.csr(at[(x, y)])
        else:
            rp, col, val = st.csr(at[(y, x)], transposed=True)
        return col[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]]

    def bp_row(x, i):
        rp, col, val = bps[x]
        return col[rp[i]:rp[i + 1]], val[rp[i]:rp[i + 1]]
    return mp_row, bp_row
