"""Plain numpy restatement of the bootstrap contract, to the bit, on top of nj_ref.py.  Nothing here calls
the library or a device: the tests compare it with dafs_hip_alignment_bootstrap, dafs_hip_bootstrap_alignment,
dafs_host_tree_support, dafs_host_newick_support, dafs_host_support_table and the drivers (test_bootstrap_gpu.py) and check
its own properties (test_bootstrap_cpu.py)."""
import numpy as np

import nj_ref

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(z):
    """mix of DESIGN.md section 13 on Python integers, mod 2^64"""
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draws(seed, k, U):
    """the U draws of replicate k, each below U: indices into the ascending list of the used columns"""
    base = mix(seed + GOLDEN * (k + 1))
    return [((mix(base + i) >> 32) * U) >> 32 for i in range(U)]


def used_columns(length, use=None):
    return [c for c in range(length) if use is None or use[c]]


def replicate_cells(cell, use, seed, k):
    """replicate k of the alignment cell (codes, [n, len]) as cells [n, U]"""
    cell = np.asarray(cell, np.uint8)
    cols = used_columns(cell.shape[1], use)
    if not cols:
        raise ValueError("bootstrap_ref: no used column")
    return cell[:, [cols[j] for j in draws(seed, k, len(cols))]]


def counts(cell):
    """(ident, aligned) of DESIGN.md section 18 over all columns of cell, as exact integer matrices"""
    cell = np.asarray(cell)
    res = (cell <= 4).astype(np.int64)
    aligned = res @ res.T
    ident = np.zeros_like(aligned)
    for a in range(4):
        one = (cell == a).astype(np.int64)
        ident += one @ one.T
    return ident, aligned


def replicate_tree(cell, use, model, seed, k):
    """(left, right, length) of replicate k: its counts, nj_ref.distances_ref, nj_ref.nj_ref"""
    ident, aligned = counts(replicate_cells(cell, use, seed, k))
    return nj_ref.nj_ref(nj_ref.distances_ref(ident, aligned, model))


def sides(left, right):
    """per node below the root its side: the leaves below it if leaf 0 is not among them, otherwise the rest"""
    n = (len(left) + 1) // 2
    everything = frozenset(range(n))
    below = nj_ref.leaf_sets(left, right)
    return [below[v] if 0 not in below[v] else everything - below[v] for v in range(2 * n - 2)]


def support_ref(left, right, rep_left, rep_right):
    """per node of the main tree the number of replicate trees with a node of the same side; -1 for the root and for a split
    with fewer than two leaves on a side"""
    n = (len(left) + 1) // 2
    out = np.full(2 * n - 1, -1, np.int64)
    mine = sides(left, right)
    theirs = [set(sides(rl, rr)) for rl, rr in zip(rep_left, rep_right)]
    for v, side in enumerate(mine):
        if len(side) >= 2 and n - len(side) >= 2:
            out[v] = sum(1 for s in theirs if side in s)
    return out


def bootstrap_ref(cell, use, model, B, seed, tree):
    """(support, rep_left [B, 2n-1], rep_right) of the main tree (left, right, ...) from B replicates"""
    n = np.asarray(cell).shape[0]
    if n <= 3:
        return np.full(2 * n - 1, -1, np.int64), np.full((B, 2 * n - 1), -1, np.int64), np.full((B, 2 * n - 1), -1, np.int64)
    reps = [replicate_tree(cell, use, model, seed, k) for k in range(B)]
    rep_left = np.array([r[0] for r in reps], np.int64)
    rep_right = np.array([r[1] for r in reps], np.int64)
    return support_ref(tree[0], tree[1], rep_left, rep_right), rep_left, rep_right


def percent(support, B):
    return (200 * int(support) + B) // (2 * B)


def silent_root_child(left, right):
    """the child of the root that does not show the root split: the right one if the left one is a join"""
    n = (len(left) + 1) // 2
    if n < 2:
        return None
    return int(right[-1]) if int(left[-1]) >= n else None


def _fmt(v):
    return "%.9g" % v


def newick_ref(names, left, right, length, support, B):
    """dafs_host_newick_support's text for plain names (no quoting here)"""
    n = len(names)
    root, silent = 2 * n - 2, silent_root_child(left, right)
    text = {}
    for v in range(2 * n - 1):  # children precede their join
        if v < n:
            t = names[v]
        else:
            t = "(" + text.pop(int(left[v])) + "," + text.pop(int(right[v])) + ")"
            if v != root and v != silent and support[v] >= 0:
                t += str(percent(support[v], B))
        if v != root and length is not None:
            t += ":" + _fmt(length[v])
        text[v] = t
    return text[root] + ";\n"


def table_ref(names, left, right, support, B, seed, model):
    """dafs_host_support_table's text"""
    n = len(names)
    silent = silent_root_child(left, right)
    out = ["# rows %d replicates %d seed %d model %s\n" % (n, B, seed, model)]
    for v, side in enumerate(sides(left, right)):
        if v == silent or support[v] < 0:
            continue
        out.append("%d\t%d\t%d\t%d\t%d\t%s\n" % (v + 1, support[v], B, percent(support[v], B), len(side), ",".join(names[x] for x in sorted(side))))
    return "".join(out)
