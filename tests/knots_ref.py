"""Plain-Python restatements of the definitions of a seed structure whose pairs may cross, the
yardsticks of test_seed_knots_cpu.py and test_seed_knots_gpu.py: the group matching, the cleaning, the level assignment, the
per-level constraints, the carried levels and the merge of a sequence's folds.  Nothing here calls the library."""
import numpy as np

from structure_ref import NONE, Refused, complementary, residue_at

FREE = 0xFF
MAX_LEVELS = 4
UNPAIRED = ".,:_-~"
# the groups in their order: the four bracket kinds, then the letters (upper case opens, lower case closes)
GROUPS = [("(", ")"), ("[", "]"), ("{", "}"), ("<", ">")] + [(chr(ord("A") + k), chr(ord("a") + k)) for k in range(26)]


def crosses(a, b, i, j):
    """the literal definition: the pairs (a, b) and (i, j) cross"""
    return a < i < b < j or i < a < j < b


def group_pairs(structure):
    """per group the list of its pairs (left, right), each group matched last-in-first-out with itself"""
    opens = {o: g for g, (o, _) in enumerate(GROUPS)}
    closes = {c: g for g, (_, c) in enumerate(GROUPS)}
    stacks = [[] for _ in GROUPS]
    pairs = [[] for _ in GROUPS]
    for c, ch in enumerate(structure):
        if ch in opens:
            stacks[opens[ch]].append(c)
        elif ch in closes:
            if not stacks[closes[ch]]:
                raise Refused("unbalanced")
            pairs[closes[ch]].append((stacks[closes[ch]].pop(), c))
        elif ch not in UNPAIRED:
            raise Refused("character")
    if any(stacks):
        raise Refused("unbalanced")
    return pairs


def clean(rows, structure):
    """(rows without their all-gap columns and '-' for gaps, ss, level) over the kept columns: ss the right column at a pair's
    left column and NONE elsewhere, level the pair's level at both of its columns and FREE elsewhere.  A pair that loses a
    column is dropped first; then, group after group, a non-empty group goes to the lowest level at which none of its pairs
    crosses a pair already placed there; a fifth level is refused."""
    if len(structure) != len(rows[0]):
        raise Refused("length")
    pairs = group_pairs(structure)
    keep = [c for c in range(len(rows[0])) if any(r[c] not in ".-" for r in rows)]
    now = {c: k for k, c in enumerate(keep)}
    ss, level = [NONE] * len(keep), [FREE] * len(keep)
    placed = [[] for _ in range(MAX_LEVELS)]
    for prs in pairs:
        mine = [(now[a], now[b]) for a, b in prs if a in now and b in now]
        if not mine:
            continue
        for lv in range(MAX_LEVELS):
            if not any(crosses(a, b, i, j) for a, b in placed[lv] for i, j in mine):
                break
        else:
            raise Refused("levels")
        placed[lv] += mine
        for i, j in mine:
            ss[i] = j
            level[i] = level[j] = lv
    return ["".join("-" if r[c] in ".-" else r[c] for c in keep) for r in rows], ss, level


def row_constraints(mask_row, ss, level, nlevels, residues):
    """the nlevels constraint strings of one row: string k has '?' everywhere, '(' ')' at a pair of level k the row holds both
    residues of when they are complementary and at least 4 apart, '.' at both residues of a pair of another level the row holds
    both residues of; a string k >= 1 without '(' is empty"""
    pos = residue_at(mask_row)
    out = []
    for k in range(nlevels):
        s = ["?"] * len(residues)
        for c, p in enumerate(ss):
            if p == NONE:
                continue
            i, j = pos[c], pos[p]
            if i is None or j is None:
                continue
            if level[c] != k:
                s[i] = s[j] = "."
            elif j - i >= 4 and complementary(residues[i], residues[j]):
                s[i], s[j] = "(", ")"
        s = "".join(s)
        out.append(s if k == 0 or "(" in s else "")
    return out


def carry_levels(seed_level, seed_col, width):
    """the levels in merged columns: insert columns FREE"""
    out = [FREE] * width
    for c, lv in enumerate(seed_level):
        out[seed_col[c]] = lv
    return out


def nested(ss, level, k):
    """True when the pairs of level k do not cross one another"""
    prs = [(i, p) for i, p in enumerate(ss) if p != NONE and level[i] == k]
    return not any(crosses(a, b, i, j) for a, b in prs for i, j in prs)


def merge_rows(denses, L, th):
    """The store rows of one sequence of length L from the dense triangular posteriors of its folds (the oracle's layout: cell
    (i, j), 1-based, i <= j, at i (2 (L + 1) - i - 1) / 2 + j): per cell the maximum over the folds, kept where it exceeds th, rows
    in order, columns ascending.  Returns (rowptr[L + 1] uint32, col uint32 0-based, val float32)."""
    best = np.max(np.stack([np.asarray(d, np.float32) for d in denses]), axis=0)
    rowptr, col, val = [0], [], []
    for i in range(1, L + 1):
        off = i * (2 * (L + 1) - i - 1) // 2
        for j in range(i, L + 1):
            if best[off + j] > np.float32(th):
                col.append(j - 1)
                val.append(best[off + j])
        rowptr.append(len(col))
    return np.array(rowptr, np.uint32), np.array(col, np.uint32), np.array(val, np.float32)
