"""Stockholm output with posterior-probability lines (the Python twin of the `dafs --stockholm` writer in
dafs_amd/csrc/host/cli_main.cpp; both produce the same bytes).  One block per alignment:

    # STOCKHOLM 1.0
    #=GF CC <the tree line>
    <name>           <row, '-' for gaps>
    #=GR <name> PP   <PP characters>
    ...
    #=GC SS_cons     <bracket string>
    #=GC PP_cons     <PP characters of the column reliabilities>
    //

The reliabilities come from Context.alignment_reliability (DESIGN.md "Alignment reliability")."""
import math

_SPACE = " \t\n\v\f\r"  # C isspace() in the "C" locale


def pp_char(p):
    """Infernal's PP character: '*' for p >= 0.95, else the digit floor(p * 10 + 0.5), in double"""
    p = float(p)
    if p >= 0.95:
        return "*"
    return chr(ord("0") + int(math.floor(p * 10.0 + 0.5)))


def names(headers):
    """Stockholm names of FASTA headers in input order: the first whitespace-separated word, "seq<k>" (k 1-based) for an
    empty one, ".2", ".3", ... appended to the second, third, ... occurrence of a name"""
    out, seen = [], {}
    for k, h in enumerate(headers):
        b = 0
        while b < len(h) and h[b] in _SPACE:
            b += 1
        e = b
        while e < len(h) and h[e] not in _SPACE:
            e += 1
        nm = h[b:e] or "seq%d" % (k + 1)
        seen[nm] = seen.get(nm, 0) + 1
        out.append(nm if seen[nm] == 1 else "%s.%d" % (nm, seen[nm]))
    return out


def row_pp(row, rel):
    """PP line of one printed row: the residues' reliabilities (in sequence order) at their columns, '.' at gaps"""
    out, k = [], 0
    for ch in row:
        if ch == "-":
            out.append(".")
        else:
            out.append(pp_char(rel[k]))
            k += 1
    return "".join(out)


def block(tree_line, row_names, rows, residue_rel, col_rel, ss_str):
    """One alignment.  row_names / rows / residue_rel: per printed row (stdout order) its Stockholm name, its text and its
    residues' reliabilities; col_rel: per column; a column without residues gets '.' in PP_cons."""
    labels = list(row_names) + ["#=GR %s PP" % nm for nm in row_names] + ["#=GC SS_cons", "#=GC PP_cons"]
    width = max(len(s) for s in labels) + 1
    lines = ["# STOCKHOLM 1.0", "#=GF CC " + tree_line]
    for nm, row, rel in zip(row_names, rows, residue_rel):
        lines.append(nm.ljust(width) + row)
        lines.append(("#=GR %s PP" % nm).ljust(width) + row_pp(row, rel))
    cons = "".join("." if all(r[c] == "-" for r in rows) else pp_char(col_rel[c]) for c in range(len(col_rel)))
    lines.append("#=GC SS_cons".ljust(width) + ss_str)
    lines.append("#=GC PP_cons".ljust(width) + cons)
    lines.append("//")
    return "\n".join(lines) + "\n"
