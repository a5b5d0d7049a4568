"""Plain numpy restatement of the transfer bootstrap, by brute force and in integers, on top of
bootstrap_ref.py and nj_ref.py.  Nothing here calls the library or a device: the tests compare it with dafs_hip_tree_transfer,
dafs_hip_alignment_bootstrap_transfer, dafs_host_newick_transfer, dafs_host_transfer_table and the drivers
(test_transfer_gpu.py) and check its own properties (test_transfer_cpu.py)."""
import numpy as np

import bootstrap_ref as br
import nj_ref


def side_matrix(left, right):
    """bool [2n-2, n]: row v is side(v) of bootstrap_ref.sides, for every node below the root, leaves included"""
    n = (len(left) + 1) // 2
    out = np.zeros((2 * n - 2, n), bool)
    for v, side in enumerate(br.sides(left, right)):
        out[v, sorted(side)] = True
    return out


def depths(left, right):
    """per node min(|side|, n - |side|); -1 for the root and for a split with fewer than two leaves on a side"""
    n = (len(left) + 1) // 2
    out = np.full(2 * n - 1, -1, np.int64)
    if n >= 2:
        size = side_matrix(left, right).sum(1)
        d = np.minimum(size, n - size)
        out[:2 * n - 2] = np.where(d >= 2, d, -1)
    return out


def transfer_each_ref(left, right, rep_left, rep_right):
    """phi [B, 2n-1]: per replicate tree and node v of the main tree the smallest min(H, n - H) over all nodes u of the
    replicate below its root, H the Hamming distance of side(v) and side(u); -1 for the root and trivial splits"""
    n = (len(left) + 1) // 2
    B = len(rep_left)
    out = np.full((B, 2 * n - 1), -1, np.int64)
    shown = np.flatnonzero(depths(left, right) >= 0)
    if len(shown) == 0:
        return out
    mine = side_matrix(left, right)[shown].astype(np.int64)  # [S, n]
    for k in range(B):
        theirs = side_matrix(rep_left[k], rep_right[k]).astype(np.int64)  # [2n-2, n]
        hamming = mine.sum(1)[:, None] + theirs.sum(1)[None, :] - 2 * (mine @ theirs.T)
        out[k, shown] = np.minimum(hamming, n - hamming).min(1)
    return out


def transfer_ref(left, right, rep_left, rep_right):
    """(transfer [2n-1], phi [B, 2n-1]): the sums over the replicates, -1 where phi is"""
    phi = transfer_each_ref(left, right, rep_left, rep_right)
    n = (len(left) + 1) // 2
    total = phi.sum(0) if len(phi) else np.zeros(2 * n - 1, np.int64)
    return np.where(depths(left, right) >= 0, total, -1), phi


def percent(transfer, depth, B):
    """the transfer bootstrap expectation in percent, halves rounded up"""
    most = B * (int(depth) - 1)
    return (200 * (most - int(transfer)) + most) // (2 * most)


def newick_ref(names, left, right, length, transfer, B):
    """dafs_host_newick_transfer's text for plain names: bootstrap_ref.newick_ref with tbe as the labels"""
    n = len(names)
    depth = depths(left, right)
    root, silent = 2 * n - 2, br.silent_root_child(left, right)
    text = {}
    for v in range(2 * n - 1):
        if v < n:
            t = names[v]
        else:
            t = "(" + text.pop(int(left[v])) + "," + text.pop(int(right[v])) + ")"
            if v != root and v != silent and transfer[v] >= 0:
                t += str(percent(transfer[v], depth[v], B))
        if v != root and length is not None:
            t += ":" + br._fmt(length[v])
        text[v] = t
    return text[root] + ";\n"


def table_ref(names, left, right, support, transfer, B, seed, model):
    """dafs_host_transfer_table's text: bootstrap_ref.table_ref's lines with depth, transfer and tbe behind them"""
    plain = br.table_ref(names, left, right, support, B, seed, model).splitlines()
    depth = depths(left, right)
    out = [plain[0] + " measure transfer\n"]
    for line in plain[1:]:
        v = int(line.split("\t")[0]) - 1
        out.append("%s\t%d\t%d\t%d\n" % (line, depth[v], transfer[v], percent(transfer[v], depth[v], B)))
    return "".join(out)


def caterpillar(n, order=None):
    """((((o0,o1),o2),o3),...) over the leaves in `order` (default 0 .. n-1) in build_tree's layout"""
    order = list(range(n)) if order is None else list(order)
    left = np.full(2 * n - 1, -1, np.int64)
    right = np.full(2 * n - 1, -1, np.int64)
    left[n], right[n] = order[0], order[1]
    for t in range(1, n - 1):
        left[n + t], right[n + t] = n + t - 1, order[t + 1]
    return left, right
