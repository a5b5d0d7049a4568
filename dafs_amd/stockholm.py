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

With covariation statistics (Context.alignment_covariation) a `#=GC cov_SS_cons` line follows PP_cons:
'2' at both columns of every consensus pair whose E-value is at most e_max, '.' elsewhere.

The reliabilities come from Context.alignment_reliability (DESIGN.md "Alignment reliability").  An alignment with new
sequences added to a seed (pipeline.add, `dafs --seed`) has no tree line, so no CC line, and a `#=GC RF` line after
PP_cons.

read_seed reads a seed alignment for pipeline.add: Stockholm or aligned FASTA; the C++ reader in
cli_main.cpp accepts and refuses the same files with the same messages."""
import math
import re

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


def cov_ss_cons(ss, pair_e, e_max=0.05):
    """The `#=GC cov_SS_cons` characters: '2' at both columns of every pair of ss (left column -> right column, 0xFFFFFFFF
    otherwise) with pair_e <= e_max (compared in double; a NaN never is), '.' elsewhere"""
    out = ["."] * len(ss)
    for c in range(len(ss)):
        if int(ss[c]) != 0xFFFFFFFF and float(pair_e[c]) <= float(e_max):
            out[c] = out[int(ss[c])] = "2"
    return "".join(out)


def block(tree_line, row_names, rows, residue_rel, col_rel, ss_str, rf=None, cov=None):
    """One alignment.  row_names / rows / residue_rel: per printed row (stdout order) its Stockholm name, its text and its
    residues' reliabilities; col_rel: per column; a column without residues gets '.' in PP_cons.  tree_line None: no
    `#=GF CC` line.  rf: per column True for a seed column ('x'), False for an insert column ('.'), written as `#=GC RF`
    after PP_cons; None: no RF line.  cov: the cov_SS_cons characters (cov_ss_cons), written as `#=GC cov_SS_cons` directly after
    PP_cons; None: no such line, and the labels are as wide as without it."""
    labels = list(row_names) + ["#=GR %s PP" % nm for nm in row_names] + ["#=GC SS_cons", "#=GC PP_cons"]
    if cov is not None:
        labels.append("#=GC cov_SS_cons")
    width = max(len(s) for s in labels) + 1
    lines = ["# STOCKHOLM 1.0"]
    if tree_line is not None:
        lines.append("#=GF CC " + tree_line)
    for nm, row, rel in zip(row_names, rows, residue_rel):
        lines.append(nm.ljust(width) + row)
        lines.append(("#=GR %s PP" % nm).ljust(width) + row_pp(row, rel))
    cons = "".join("." if all(r[c] == "-" for r in rows) else pp_char(col_rel[c]) for c in range(len(col_rel)))
    lines.append("#=GC SS_cons".ljust(width) + ss_str)
    lines.append("#=GC PP_cons".ljust(width) + cons)
    if cov is not None:
        lines.append("#=GC cov_SS_cons".ljust(width) + cov)
    if rf is not None:
        lines.append("#=GC RF".ljust(width) + "".join("x" if f else "." for f in rf))
    lines.append("//")
    return "\n".join(lines) + "\n"


class SeedError(ValueError):
    pass


_LETTERS = frozenset("ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz")  # C isalpha() in the "C" locale
_GAPS = frozenset(".-")


def _fields(line):
    return [f for f in re.split("[" + re.escape(_SPACE) + "]+", line) if f]


def parse_seed(text):
    """(names, rows) of a seed as its file holds them, before clean_seed.  Stockholm when the first line is
    `# STOCKHOLM 1.0`: the first alignment up to `//`, interleaved blocks concatenated by name (names in order of first
    appearance), `#` lines (GF, GS, GR, GC) ignored, every other non-blank line `name row`.  Otherwise aligned FASTA as
    `dafs` prints it: lines before the first `>` ignored (the tree line), leading blanks of a name stripped, a record named
    SS_cons skipped, a row may span several lines."""
    lines = [ln.rstrip(_SPACE) for ln in text.split("\n")]
    names, rows = [], []
    if lines and lines[0] == "# STOCKHOLM 1.0":
        at = {}
        for k, ln in enumerate(lines[1:], 2):
            if ln == "//":
                break
            if not ln.strip(_SPACE) or ln.startswith("#"):
                continue
            f = _fields(ln)
            if len(f) != 2:
                raise SeedError("seed: line %d is neither a #= annotation nor 'name row'" % k)
            if f[0] not in at:
                at[f[0]] = len(names)
                names.append(f[0])
                rows.append("")
            rows[at[f[0]]] += f[1]
        return names, rows
    keep = False
    for ln in lines:
        if ln.startswith(">"):
            nm = ln[1:].lstrip(_SPACE)
            keep = nm != "SS_cons"
            if keep:
                names.append(nm)
                rows.append("")
        elif keep:
            rows[-1] += "".join(_fields(ln))
    return names, rows


def clean_seed(names, rows):
    """Checks a seed and drops its all-gap columns.  Refuses (SeedError) an empty seed, rows of unequal length, a
    character that is neither a letter nor a gap ('.' or '-'), a row without residues.  Returns (names, rows) with '-'
    for every gap."""
    names, rows = list(names), list(rows)
    if not rows:
        raise SeedError("seed: no rows")
    if len(names) != len(rows):
        raise SeedError("seed: one name per row")
    for nm, row in zip(names, rows):
        if len(row) != len(rows[0]):
            raise SeedError("seed: rows of unequal length (%s: %d columns, %s: %d)" % (names[0], len(rows[0]), nm, len(row)))
        for ch in row:
            if ch not in _LETTERS and ch not in _GAPS:
                raise SeedError("seed: row %s holds '%s', which is neither a letter nor a gap" % (nm, ch))
        if all(ch in _GAPS for ch in row):
            raise SeedError("seed: row %s has no residues" % nm)
    keep = [c for c in range(len(rows[0])) if any(row[c] not in _GAPS for row in rows)]  # not empty: every row has a residue
    return names, ["".join("-" if row[c] in _GAPS else row[c] for c in keep) for row in rows]


def read_seed(path):
    """A seed alignment file (Stockholm or aligned FASTA, parse_seed) checked and without its all-gap columns
    (clean_seed): (names, rows), '-' for gaps"""
    with open(path, "rb") as fh:
        text = fh.read().decode("latin-1")
    return clean_seed(*parse_seed(text))
