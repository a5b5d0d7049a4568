"""Plain-Python restatements of the seed-structure definitions, the yardsticks of
test_seed_structure_cpu.py and test_seed_structure_gpu.py.  Nothing here calls the library."""
NONE = 0xFFFFFFFF
OPEN, CLOSE, UNPAIRED = "(<[{", ")>]}", ".,:_-~"


class Refused(ValueError):
    pass


def partners(structure):
    """partner column per column of a structure line (None: unpaired); each bracket kind is matched with its own kind"""
    out = [None] * len(structure)
    stacks = {k: [] for k in OPEN}
    for c, ch in enumerate(structure):
        if ch in OPEN:
            stacks[ch].append(c)
        elif ch in CLOSE:
            st = stacks[OPEN[CLOSE.index(ch)]]
            if not st:
                raise Refused("unbalanced")
            o = st.pop()
            out[c], out[o] = o, c
        elif not (ch.isascii() and ch.isalpha()) and ch not in UNPAIRED:
            raise Refused("character")
    if any(stacks.values()):
        raise Refused("unbalanced")
    pairs = [(c, p) for c, p in enumerate(out) if p is not None and p > c]
    for a, b in pairs:
        for c, d in pairs:
            if a < c < b < d:
                raise Refused("crossing")
    return out


def clean(rows, structure):
    """(rows without their all-gap columns and '-' for gaps, ss over the kept columns: the right column at a pair's left
    column, NONE elsewhere); a pair that loses a column is dropped"""
    if len(structure) != len(rows[0]):
        raise Refused("length")
    part = partners(structure)
    keep = [c for c in range(len(rows[0])) if any(r[c] not in ".-" for r in rows)]
    now = {c: k for k, c in enumerate(keep)}
    ss = [now[part[c]] if part[c] is not None and part[c] > c and part[c] in now else NONE for c in keep]
    return ["".join("-" if r[c] in ".-" else r[c] for c in keep) for r in rows], ss


def complementary(a, b):
    """CONTRAfold's pairs over its alphabet ACGU (either case): T is not U there"""
    return (a.upper(), b.upper()) in {("A", "U"), ("U", "A"), ("G", "C"), ("C", "G"), ("G", "U"), ("U", "G")}


def residue_at(mask_row):
    """per column the residue index of the row, None at a gap"""
    out, k = [], 0
    for m in mask_row:
        out.append(k if m else None)
        k += 1 if m else 0
    return out


def row_constraint(mask_row, ss, residues):
    """'?' everywhere; '(' / ')' at the residues of a pair the row holds both ends of, when they are complementary and at
    least 4 apart in the row"""
    pos = residue_at(mask_row)
    out = ["?"] * len(residues)
    for c, p in enumerate(ss):
        if p == NONE:
            continue
        i, j = pos[c], pos[p]
        if i is None or j is None or j - i < 4 or not complementary(residues[i], residues[j]):
            continue
        out[i], out[j] = "(", ")"
    return "".join(out)


def carry(seed_ss, seed_col, width):
    """the seed's structure in merged columns: insert columns unpaired"""
    out = [NONE] * width
    for c, p in enumerate(seed_ss):
        if p != NONE:
            out[seed_col[c]] = seed_col[p]
    return out


def support(mask_row, ss, residues, bp_row):
    """(both, canonical, half, expected) of one row; bp_row = (rowptr, col, val) of its sequence; expected adds the float32
    values widened to double in ascending left column"""
    pos = residue_at(mask_row)
    rowptr, col, val = bp_row
    both = canonical = half = 0
    expected = 0.0
    for c, p in enumerate(ss):
        if p == NONE:
            continue
        i, j = pos[c], pos[p]
        if (i is None) != (j is None):
            half += 1
        if i is None or j is None:
            continue
        both += 1
        canonical += 1 if complementary(residues[i], residues[j]) else 0
        v = 0.0
        for k in range(int(rowptr[i]), int(rowptr[i + 1])):
            if int(col[k]) == j:
                v = float(val[k])
        expected += v
    return both, canonical, half, expected
