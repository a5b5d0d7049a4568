"""Plain numpy restatement of the linkage contract: single, complete and average linkage of a
similarity matrix, to the bit.  Nothing here calls the library or a device: the tests compare it with dafs_hip_linkage_tree,
dafs_hipk_linkage and the drivers (test_linkage_gpu.py) and check its own properties (test_linkage_cpu.py).

Clusters live in slots 0 .. n-1.  Join t takes the first maximum, in row-major order, of the upper triangle of the current
matrix (so: the highest similarity, then the smallest a, then the smallest b; -0 equals 0), writes node n + t, rewrites slot a
and retires slot b: its row and column become -inf."""
import numpy as np

RULES = ("single", "complete", "average")


def linkage_ref(sim, rule):
    """(score float32 [2n-1], left int64, right int64) in capi.build_tree's layout; only the entries x < y of sim are read"""
    if rule not in RULES:
        raise ValueError("linkage_ref: unknown rule %r" % (rule,))
    sim = np.asarray(sim, np.float32)
    n = sim.shape[0]
    assert sim.shape == (n, n) and n >= 1
    score = np.zeros(2 * n - 1, np.float32)
    left = np.full(2 * n - 1, -1, np.int64)
    right = np.full(2 * n - 1, -1, np.int64)
    U = np.full((n, n), -np.inf, np.float32)  # the upper triangle alone; everything else never wins
    iu = np.triu_indices(n, 1)
    U[iu] = sim[iu]
    assert np.isfinite(U[iu]).all(), "linkage_ref: a non-finite entry above the diagonal"
    size = np.ones(n, np.int64)
    node = np.arange(n, dtype=np.int64)
    idx = np.arange(n)
    with np.errstate(invalid="ignore"):
        for t in range(n - 1):
            a, b = divmod(int(np.argmax(U)), n)
            assert a < b
            score[n + t], left[n + t], right[n + t] = U[a, b], node[a], node[b]
            p = np.where(idx > a, U[a, :], U[:, a])  # S(a, k) for every k; -inf for k = a and for retired k
            q = np.where(idx > b, U[b, :], U[:, b])
            if rule == "single":
                v = np.where(p >= q, p, q)
            elif rule == "complete":
                v = np.where(p <= q, p, q)
            else:
                s = np.float64(size[a]) * p.astype(np.float64) + np.float64(size[b]) * q.astype(np.float64)
                v = (s / np.float64(size[a] + size[b])).astype(np.float32)
            v[a] = v[b] = -np.inf
            v[~np.isfinite(p)] = -np.inf  # retired slots stay retired (and k = a, b)
            U[a, a + 1:] = v[a + 1:]
            U[:a, a] = v[:a]
            U[b, :] = -np.inf
            U[:, b] = -np.inf
            size[a] += size[b]
            node[a] = n + t
    return score, left, right


def leaves(tree, node):
    """the leaves below `node`, ascending (no recursion: a comb is as deep as the set)"""
    score, left, right = tree
    n = (len(score) + 1) // 2
    out, todo = [], [int(node)]
    while todo:
        x = todo.pop()
        if x < n:
            out.append(x)
        else:
            todo += [int(left[x]), int(right[x])]
    return sorted(out)


def canon(tree, node, relabel):
    """a subtree as nested (score bits, left, right) tuples with the leaves renamed by `relabel`"""
    score, left, right = tree
    n = (len(score) + 1) // 2
    if node < n:
        return relabel[int(node)]
    return (np.float32(score[node]).tobytes(), canon(tree, left[node], relabel), canon(tree, right[node], relabel))


def chain_case(n):
    """A matrix whose tree is known in closed form under every rule, for sizes the restatement is too slow for: S(i, j) =
    float32(1 - j / n) for i < j.  Every entry of column k is the same value, so whichever rule joins it keeps it (the double
    mean of equal floats narrows to that float); slot 0 takes slots 1, 2, ... in turn: a left comb with falling scores.
    Returns (sim, (score, left, right)); only the upper triangle of sim is meaningful."""
    col = (1.0 - np.arange(n, dtype=np.float64) / n).astype(np.float32)
    sim = np.empty((n, n), np.float32)
    sim[:] = col[None, :]
    score = np.concatenate([np.zeros(n, np.float32), col[1:]])
    left = np.concatenate([np.full(n, -1, np.int64), [0] if n > 1 else [], np.arange(n, 2 * n - 2)]).astype(np.int64)
    right = np.concatenate([np.full(n, -1, np.int64), np.arange(1, n)]).astype(np.int64)
    return sim, (score, left, right)
