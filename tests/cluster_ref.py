"""Plain-Python restatement of what the clustering adds to the library's host code: the cut of a guide
tree into clusters (dafs_host_cluster_cut, host_tree.cpp), the cluster table (dafs_host_cluster_table, host_text.cpp) and the
ranges of the similarity pass (dafs_host_similarity_ranges).  Nothing here calls the library: the tests compare it with the
library (test_cluster_cpu.py) and with the drivers (test_cluster_gpu.py)."""
import numpy as np

import text_ref


def members(n, left, right, node):
    """the leaves below `node`, in the order the tree holds them"""
    if node < n:
        return [int(node)]
    return members(n, left, right, left[node]) + members(n, left, right, right[node])


def kept_joins(tree, threshold=None, count=None):
    """per node of the tree True when the join is kept (leaves: True).  threshold: its score is >= threshold and every join
    below it is kept; count: every join but the count - 1 with the highest node indices."""
    score, left, right = tree
    T = len(score)
    n = (T + 1) // 2
    kept = [True] * T
    for i in range(n, T):
        own = i < T - (count - 1) if count is not None else bool(np.float32(score[i]) >= np.float32(threshold))
        kept[i] = own and kept[left[i]] and kept[right[i]]
    return kept


def cut(tree, threshold=None, count=None):
    """(labels, roots): the cluster of every leaf, and per cluster the node whose leaves it is.  A cluster is the leaf set of a
    maximal kept join, or a single leaf; clusters are numbered by their smallest member."""
    score, left, right = tree
    T = len(score)
    n = (T + 1) // 2
    kept = kept_joins(tree, threshold, count)
    parent = {}
    for i in range(n, T):
        parent[int(left[i])] = parent[int(right[i])] = i
    # a kept node (leaves count as kept) under an undone parent, or the kept root
    maximal = [i for i in range(T) if kept[i] and not (i in parent and kept[parent[i]])]
    groups = sorted((sorted(members(n, left, right, i)), i) for i in maximal)
    labels = np.zeros(n, np.uint32)
    for c, (leaves, _) in enumerate(groups):
        labels[leaves] = c
    assert sorted(x for g, _ in groups for x in g) == list(range(n))
    return labels, [i for _, i in groups]


def subtree_canon(tree, node, relabel):
    """a subtree as nested (score bits, left, right) tuples with the leaves renamed by `relabel`"""
    score, left, right = tree
    n = (len(score) + 1) // 2
    if node < n:
        return relabel[int(node)]
    return (np.float32(score[node]).tobytes(), subtree_canon(tree, left[node], relabel), subtree_canon(tree, right[node], relabel))


def table(headers, lengths, labels, tree, sim):
    """the text of --cluster-table: per sequence i name length cluster size join nearest_in sim_in nearest_out sim_out"""
    names = text_ref.names(headers)
    n = len(names)
    labels = [int(x) for x in labels]
    score, left, right = tree
    size = {c: labels.count(c) for c in set(labels)}
    join = {}
    for c in size:
        want = sorted(i for i in range(n) if labels[i] == c)
        node = [i for i in range(len(score)) if sorted(members(n, left, right, i)) == want]
        assert len(node) == 1
        join[c] = float("nan") if node[0] < n else float(score[node[0]])
    out = []
    for i in range(n):
        fields = [str(i + 1), names[i], str(int(lengths[i])), str(labels[i] + 1), str(size[labels[i]]), text_ref._fmt9(join[labels[i]])]
        for inside in (True, False):
            cand = [j for j in range(n) if j != i and (labels[j] == labels[i]) == inside]
            if not cand:
                fields += ["0", "nan"]
                continue
            best = max(float(sim[i][j]) for j in cand)
            j = min(j for j in cand if float(sim[i][j]) == best)  # ties go to the smallest index
            fields += [str(j + 1), text_ref._fmt9(sim[i][j])]
        out.append("\t".join(fields) + "\n")
    return "".join(out)


def pair_bytes(lx, ly):
    """what a pair takes before its launch: 2 * min(len) * 24 entries of 8 bytes and its row pointers in both directions"""
    return 2 * min(lx, ly) * 24 * 8 + 4 * (lx + ly + 2)


def ranges(lens, max_bytes):
    """the ranges [begin, end) of the row-major pairs, greedy in pair order under max_bytes, a pair over the budget alone"""
    out, begin, used, p = [], 0, 0, 0
    n = len(lens)
    for x in range(n):
        for y in range(x + 1, n):
            b = pair_bytes(lens[x], lens[y])
            if p > begin and used + b > max_bytes:
                out.append((begin, p))
                begin, used = p, 0
            used += b
            p += 1
    if p > begin:
        out.append((begin, p))
    return out
