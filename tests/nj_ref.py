"""Plain numpy restatement of the neighbour-joining contract, to the bit.  Nothing here calls the
library or a device: the tests compare it with dafs_hip_nj_tree, dafs_hipk_nj, dafs_host_nj_distances and the drivers
(test_phylogeny_gpu.py) and check its own properties (test_phylogeny_cpu.py).

Clusters live in slots 0 .. n-1.  Join t takes the first minimum, in row-major order over the active slots, of
Q(i, j) = ((m - 2) * D(i, j) - R[i]) - R[j] (so: the smallest Q, then the smallest a, then the smallest b), writes node n + t
and the two branch lengths, rewrites slot a and retires slot b.  Every step is vectorised over a row with the same
elementwise order of operations as the contract; the running sums are running sums."""
import math

import numpy as np

CAP = 3.0
Q20 = 1048576.0


def _running_sum(values):
    s = 0.0
    for v in values:
        s = s + float(v)
    return s


def nj_ref(dist):
    """(left int64 [2n-1], right int64, length float64) in capi.build_tree's layout; only the entries x < y of dist are read.
    ValueError on the contract's refusals: a non-finite entry above the diagonal, and any non-finite value written into D, R
    or the lengths."""
    dist = np.asarray(dist, np.float64)
    n = dist.shape[0]
    if dist.ndim != 2 or dist.shape != (n, n) or n == 0:
        raise ValueError("nj_ref: the distance matrix must be n x n with n >= 1")
    left = np.full(2 * n - 1, -1, np.int64)
    right = np.full(2 * n - 1, -1, np.int64)
    length = np.zeros(2 * n - 1, np.float64)
    iu = np.triu_indices(n, 1)
    if not np.isfinite(dist[iu]).all():
        raise ValueError("nj_ref: a non-finite entry above the diagonal")
    if n == 1:
        return left, right, length
    D = np.zeros((n, n), np.float64)
    D[iu] = dist[iu]
    D.T[iu] = dist[iu]  # copied, not added: a -0.0 stays -0.0
    with np.errstate(over="ignore", invalid="ignore"):
        R = np.zeros(n, np.float64)
        for j in range(n):  # ascending j for every k at once; the diagonal's +0 changes no bit of a sum that started at +0
            R = R + D[:, j]
        written_ok = bool(np.isfinite(R).all())
        node = np.arange(n, dtype=np.int64)
        active = np.ones(n, bool)
        upper = np.triu(np.ones((n, n), bool), 1)
        for t in range(n - 1):
            act = np.flatnonzero(active)
            m = len(act)
            sub = D[np.ix_(act, act)]
            Q = (np.float64(m - 2) * sub - R[act][:, None]) - R[act][None, :]
            first_is_nan = bool(np.isnan(Q[0, 1]))
            Q = np.where(upper[:m, :m], Q, np.inf)  # act ascends: the pairs i < j are the upper triangle
            if np.isnan(Q.min()):
                Q[np.isnan(Q)] = np.inf  # a NaN is below nothing
            ia, ib = divmod(int(np.argmin(Q)), m)  # the first of equals in row-major order
            if first_is_nan or Q[ia, ib] == np.inf:  # nothing compares below the candidate the scan starts from
                ia, ib = 0, 1
            a, b = int(act[ia]), int(act[ib])
            assert a < b
            dab = D[a, b]
            la = 0.5 * dab
            if m > 2:
                la = la + (R[a] - R[b]) / (2.0 * np.float64(m - 2))
            lb = dab - la
            length[node[a]], length[node[b]] = la, lb
            left[n + t], right[n + t] = node[a], node[b]
            others = act[(act != a) & (act != b)]
            p, q = D[a, others], D[b, others]
            u = 0.5 * ((p + q) - dab)
            R[others] = ((R[others] - p) - q) + u
            D[a, others] = u
            D[others, a] = u
            R[a] = _running_sum(u)
            written_ok = written_ok and bool(np.isfinite(u).all() and np.isfinite(R[act[act != b]]).all() and np.isfinite(la) and np.isfinite(lb))
            active[b] = False
            node[a] = n + t
    if not written_ok:
        raise ValueError("nj_ref: a non-finite value was written into the distances, the row sums or the lengths")
    return left, right, length


def distances_ref(ident, aligned, model):
    """the distances of DESIGN.md section 22 from the integer matrices of alignment_identity, in Python floats and math.log"""
    ident = np.asarray(ident)
    aligned = np.asarray(aligned)
    n = ident.shape[0]
    out = np.zeros((n, n), np.float64)
    for r in range(n):
        for s in range(n):
            if r == s:
                continue
            comp = int(aligned[r, s])
            mism = comp - int(ident[r, s])
            if model == "p":
                out[r, s] = float(mism) / float(comp) if comp else 1.0
            elif model == "jc":
                if comp == 0 or 4 * mism >= 3 * comp:
                    out[r, s] = CAP
                else:
                    x = 1.0 - (4.0 * float(mism)) / (3.0 * float(comp))
                    k = math.floor(-0.75 * math.log(x) * Q20 + 0.5)
                    out[r, s] = min(float(k), CAP * Q20) / Q20
            else:
                raise ValueError("distances_ref: unknown model %r" % (model,))
    return out


def random_tree(rng, n, denominator=1024, longest=64):
    """A random binary tree over n >= 2 leaves in build_tree's layout with positive branch lengths that are multiples of
    1 / denominator (a power of two: every path sum is exact in double).  Returns (left, right, length); the two branches
    below the root are the two halves of one edge of the unrooted tree."""
    left = np.full(2 * n - 1, -1, np.int64)
    right = np.full(2 * n - 1, -1, np.int64)
    tops = list(range(n))
    for t in range(n - 1):
        i, j = sorted(rng.choice(len(tops), 2, replace=False))
        left[n + t], right[n + t] = tops[i], tops[j]
        tops[i] = n + t
        del tops[j]
    length = rng.integers(1, longest + 1, 2 * n - 1).astype(np.float64) / denominator
    length[2 * n - 2] = 0.0
    return left, right, length


def leaf_sets(left, right):
    """per node the frozenset of the leaves below it (children precede their join: one ascending pass)"""
    n = (len(left) + 1) // 2
    below = [frozenset([k]) for k in range(n)]
    for k in range(n, 2 * n - 1):
        below.append(below[int(left[k])] | below[int(right[k])])
    return below


def tree_distances(left, right, length):
    """the n x n path lengths between the leaves of a tree"""
    n = (len(left) + 1) // 2
    T = 2 * n - 1
    parent = np.full(T, -1, np.int64)
    for k in range(n, T):
        parent[left[k]] = parent[right[k]] = k
    depth = np.zeros(T, np.float64)
    for k in range(T - 2, -1, -1):  # a parent has a higher index: it is done first
        depth[k] = depth[parent[k]] + length[k]
    below = leaf_sets(left, right)
    dist = np.zeros((n, n), np.float64)
    for k in range(n, T):  # node k is the lowest common ancestor of the pairs across its children
        for x in below[int(left[k])]:
            for y in below[int(right[k])]:
                dist[x, y] = dist[y, x] = (depth[x] - depth[k]) + (depth[y] - depth[k])
    return dist


def unrooted_edges(left, right, length):
    """{split: length} of the unrooted tree: a split is the frozenset of the leaves on the side without leaf 0; the two
    branches below the root are one edge and their lengths add up"""
    n = (len(left) + 1) // 2
    everything = frozenset(range(n))
    below = leaf_sets(left, right)
    out = {}
    for k in range(2 * n - 2):
        side = below[k] if 0 not in below[k] else everything - below[k]
        out[side] = out.get(side, 0.0) + float(length[k])
    return out
