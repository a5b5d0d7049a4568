"""Plain-Python restatement of the merged alignment of pipeline.add_each(merged=True) and `dafs --seed-merged` (DESIGN.md
section 17): the merge rule of section 11 over k independent column maps, the rows, the RF line, the carried structure, the PP
lines of the placed rows, PP_cons, and the block's bytes.  Nothing here calls the library."""
import text_ref

NONE = 0xFFFFFFFF


def merge(columns, zs):
    """k maps (per residue its seed column or NONE) into a seed of `columns` columns: seed column c, then an insert block as wide
    as the widest run of unmatched residues any sequence has behind c (anchor -1: before column 0), new residues left-justified
    in it.  Returns (seed_col, res_col per sequence, width)."""
    widest = [0] * (columns + 1)  # slot a + 1 for anchor a
    for z in zs:
        anchor, run = -1, 0
        for v in list(z) + [None]:
            if v is None or v != NONE:
                widest[anchor + 1] = max(widest[anchor + 1], run)
                anchor, run = v, 0
            else:
                run += 1
    seed_col, start, pos = [], [0], widest[0]
    for c in range(columns):
        seed_col.append(pos)
        pos += 1
        start.append(pos)
        pos += widest[c + 1]
    res_col = []
    for z in zs:
        anchor, run, cols = -1, 0, []
        for v in z:
            if v != NONE:
                cols.append(seed_col[v])
                anchor, run = v, 0
            else:
                cols.append(start[anchor + 1] + run)
                run += 1
        res_col.append(cols)
    return seed_col, res_col, pos


def carry(seed_ss, seed_col, width):
    ss = [NONE] * width
    for c, p in enumerate(seed_ss):
        if p != NONE:
            ss[seed_col[c]] = seed_col[p]
    return ss


def brackets(ss):
    """one level of round brackets: what dafs_hip_make_brackets writes for a nested structure"""
    out = ["."] * len(ss)
    for c, p in enumerate(ss):
        if p != NONE:
            out[c], out[p] = "(", ")"
    return "".join(out)


class Merged:
    pass


def merged(seed_headers, seed_rows, seed_ss, headers, seqs, zs, pps):
    """The merged alignment from the seed's cleaned rows and structure, the new sequences, their maps and their residue values"""
    m, k, columns = len(seed_rows), len(seqs), len(seed_rows[0])
    mg = Merged()
    seed_col, res_col, width = merge(columns, zs)
    mg.names = text_ref.names(list(seed_headers) + list(headers))
    rows = [["-"] * width for _ in range(m + k)]
    for r in range(m):
        for c in range(columns):
            rows[r][seed_col[c]] = seed_rows[r][c]
    for j in range(k):
        for i, c in enumerate(res_col[j]):
            rows[m + j][c] = seqs[j][i]
    mg.rows = ["".join(r) for r in rows]
    mg.rf = [c in set(seed_col) for c in range(width)]
    mg.ss = carry(seed_ss, seed_col, width)
    mg.ss_str = brackets(mg.ss)
    mg.pp_lines = [text_ref.row_pp(mg.rows[m + j], pps[j]) for j in range(k)]
    mg.col = []
    for c in range(width):
        s, cnt = 0.0, 0
        for j in range(k):  # a running double sum in input order
            if c in res_col[j]:
                s += float(pps[j][res_col[j].index(c)])
                cnt += 1
        mg.col.append(s / float(cnt) if cnt else float("nan"))
    mg.pp_cons = "".join("." if v != v else text_ref.pp_char(v) for v in mg.col)
    labels = mg.names + ["#=GR %s PP" % nm for nm in mg.names[m:]] + ["#=GC SS_cons", "#=GC PP_cons", "#=GC RF"]
    w = max(len(s) for s in labels) + 1
    lines = ["# STOCKHOLM 1.0"] + [nm.ljust(w) + row for nm, row in zip(mg.names, mg.rows)]
    lines += [("#=GR %s PP" % nm).ljust(w) + pp for nm, pp in zip(mg.names[m:], mg.pp_lines)]
    lines += ["#=GC SS_cons".ljust(w) + mg.ss_str, "#=GC PP_cons".ljust(w) + mg.pp_cons,
              "#=GC RF".ljust(w) + "".join("x" if f else "." for f in mg.rf), "//"]
    mg.stockholm = "\n".join(lines) + "\n"
    mg.output = "".join([">SS_cons\n", mg.ss_str, "\n"] + ["> %s\n%s\n" % (h, row) for h, row in zip(list(seed_headers) + list(headers), mg.rows)])
    return mg
