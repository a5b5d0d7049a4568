"""Stockholm output with posterior-probability lines, and the seed reader.  Every function here is a call of the library's
host text code (dafs_amd/csrc/host_text.cpp), which the `dafs` command line calls too.  One block per alignment:

    # STOCKHOLM 1.0
    #=GF CC <the tree line>
    <name>           <row, '-' for gaps>
    #=GR <name> PP   <PP characters>
    #=GR <name> SS   <the row's own structure, with row structures>
    ...
    #=GC SS_cons     <bracket string>
    #=GC PP_cons     <PP characters of the column reliabilities>
    //

With covariation statistics (Context.alignment_covariation) a `#=GC cov_SS_cons` line follows PP_cons:
'2' at both columns of every consensus pair whose E-value is at most e_max, '.' elsewhere.

The reliabilities come from Context.alignment_reliability (DESIGN.md "Alignment reliability").  An alignment with new
sequences added to a seed (pipeline.add, `dafs --seed`) has no tree line, so no CC line, and a `#=GC RF` line after
PP_cons.

read_seed reads a seed alignment for pipeline.add: Stockholm or aligned FASTA; a file the library
refuses raises SeedError with the message `dafs --seed` prints.  read_seed_structure also returns the seed's consensus
structure; read_seed_knots reads one whose pairs may cross, with the pairs' levels.

block_merged writes the merged alignment of all placements of pipeline.add_each: the rows, then PP
lines for the placed rows only, SS_cons, PP_cons over the placed rows, RF."""
import ctypes as C

import numpy as np

from . import capi


def pp_char(p):
    """Infernal's PP character: '*' for p >= 0.95, else the digit floor(p * 10 + 0.5), in double"""
    return capi._pp_char(float(p)).decode()


def names(headers):
    """Stockholm names of FASTA headers in input order: the first whitespace-separated word, "seq<k>" (k 1-based) for an
    empty one, ".2", ".3", ... appended to the second, third, ... occurrence of a name"""
    headers = list(headers)
    return capi.split_lines(capi.host_text(capi._stockholm_names, len(headers), capi.c_strings(headers)), len(headers))


def cov_ss_cons(ss, pair_e, e_max=0.05):
    """The `#=GC cov_SS_cons` characters: '2' at both columns of every pair of ss (left column -> right column, 0xFFFFFFFF
    otherwise) with pair_e <= e_max (compared in double; a NaN never is), '.' elsewhere"""
    ss, e = np.ascontiguousarray(ss, np.uint32), np.ascontiguousarray(pair_e, np.float64)
    if ss.ndim != 1 or e.shape != ss.shape:
        raise ValueError("cov_ss_cons: one E-value per column")
    return capi.host_text(capi._cov_ss_cons, len(ss), ss.ctypes.data, e.ctypes.data, float(e_max))


def row_ss_str(row, ss, level=None):
    """A row's own structure (ss over its residues: partner index at the left one, 0xFFFFFFFF otherwise) laid into the row's
    columns: the bracket characters of capi.make_brackets at the residues' columns, '.' at gaps.  level: the pairs' levels
    (a structure decoded level by level): the characters of capi.make_brackets_levels."""
    chars = iter(capi.make_brackets(ss) if level is None else capi.make_brackets_levels(ss, level))
    return "".join("." if ch == "-" else next(chars) for ch in row)


def with_weights(text, row_names, weights):
    """A block with one `#=GS <name> WT <%.6f>` line per row directly after its `#=GF` lines (dafs_host_stockholm_weights;
    DESIGN.md section 18): the sequence weights of Context.alignment_weights.  Every other byte stays."""
    row_names = list(row_names)
    w = np.ascontiguousarray(weights, np.float64)
    if w.shape != (len(row_names),):
        raise ValueError("stockholm.with_weights: one weight per row")
    return capi.host_text(capi._stockholm_weights, text.encode("latin-1"), len(row_names), capi.c_strings(row_names), w.ctypes.data)


def block(tree_line, row_names, rows, residue_rel, col_rel, ss_str, rf=None, cov=None, row_ss=None, weights=None):
    """One alignment.  row_names / rows / residue_rel: per printed row (stdout order) its Stockholm name, its text and its
    residues' reliabilities; col_rel: per column; a column without residues gets '.' in PP_cons.  tree_line None: no
    `#=GF CC` line.  rf: per column True for a seed column ('x'), False for an insert column ('.'), written as `#=GC RF`
    after PP_cons; None: no RF line.  cov: the cov_SS_cons characters (cov_ss_cons), written as `#=GC cov_SS_cons` directly after
    PP_cons; None: no such line, and the labels are as wide as without it.  row_ss: per row its own structure in the row's
    columns (row_ss_str), written as `#=GR <name> SS` after the row's PP line; None: no such lines.  weights: per row its
    sequence weight, written as `#=GS <name> WT` lines (with_weights); None: the block byte for byte as without them."""
    row_names, rows = list(row_names), list(rows)
    col = np.ascontiguousarray(col_rel, np.float64)
    rel = [np.ascontiguousarray(r, np.float64) for r in residue_rel]
    if not len(row_names) == len(rel) == len(rows):
        raise ValueError("stockholm.block: one name and one reliability array per row")
    if any(len(r) < len(row) - row.count("-") for r, row in zip(rel, rows)):
        raise ValueError("stockholm.block: one reliability per residue")
    rf8 = None if rf is None else np.ascontiguousarray(np.asarray(rf, bool), np.uint8)
    if rf8 is not None and rf8.shape != col.shape:
        raise ValueError("stockholm.block: rf needs one entry per column")
    text = [None if t is None else t.encode("latin-1") for t in (tree_line, ss_str, cov)]
    if row_ss is not None and len(row_ss) != len(rows):
        raise ValueError("stockholm.block: one structure per row")
    out = capi.host_text(capi._stockholm_block_rows, text[0], len(rows), len(col), capi.c_strings(row_names), capi.c_strings(rows),
                         (C.c_void_p * max(len(rel), 1))(*[r.ctypes.data for r in rel]), col.ctypes.data, text[1],
                         None if rf8 is None else rf8.ctypes.data, text[2], None if row_ss is None else capi.c_strings(list(row_ss)))
    return out if weights is None else with_weights(out, row_names, weights)


def block_merged(row_names, rows, residue_rel, ss_str, rf):
    """The merged alignment of pipeline.add_each as one block (dafs_host_stockholm_block_merged): the rows,
    then `#=GR <name> PP` for every row whose residue_rel entry is not None (the placed rows), `#=GC SS_cons`, `#=GC PP_cons`
    (per column the mean of those rows' values, '.' where none has a residue), `#=GC RF`, `//`.  Returns (text, col): col the
    means behind PP_cons, NaN for a '.' column."""
    row_names, rows = list(row_names), list(rows)
    rel = [None if r is None else np.ascontiguousarray(r, np.float64) for r in residue_rel]
    if not len(row_names) == len(rel) == len(rows):
        raise ValueError("stockholm.block_merged: one name and one reliability entry per row")
    if any(r is not None and len(r) < len(row) - row.count("-") for r, row in zip(rel, rows)):
        raise ValueError("stockholm.block_merged: one reliability per residue")
    rf8 = np.ascontiguousarray(np.asarray(rf, bool), np.uint8)
    col = np.zeros(max(len(rf8), 1), np.float64)
    text = capi.host_text(capi._stockholm_block_merged, len(rows), len(rf8), capi.c_strings(row_names), capi.c_strings(rows),
                          (C.c_void_p * max(len(rel), 1))(*[None if r is None else r.ctypes.data for r in rel]), ss_str.encode("latin-1"),
                          rf8.ctypes.data, col.ctypes.data)
    return text, col[:len(rf8)]


class SeedError(ValueError):
    pass


def parse_seed(text):
    """(names, rows) of a seed as its file holds them (str, or the file's bytes), before clean_seed.  Stockholm when the first
    line is `# STOCKHOLM 1.0`: the first alignment up to `//`, interleaved blocks concatenated by name (names in order of first
    appearance), `#` lines (GF, GS, GR, GC) ignored, every other non-blank line `name row`.  Otherwise aligned FASTA as
    `dafs` prints it: lines before the first `>` ignored (the tree line), leading blanks of a name stripped, a record named
    SS_cons skipped, a row may span several lines."""
    data = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    n = C.c_uint32()
    got = capi.host_text(capi._seed_parse, data, len(data), C.byref(n), outs=2, refusal=SeedError)
    return tuple(capi.split_lines(t, n.value) for t in got)


def clean_seed(names, rows):
    """Checks a seed and drops its all-gap columns.  Refuses (SeedError) an empty seed, rows of unequal length, a
    character that is neither a letter nor a gap ('.' or '-'), a row without residues.  Returns (names, rows) with '-'
    for every gap."""
    names, rows = list(names), list(rows)
    if len(names) != len(rows):
        raise SeedError("seed: one name per row")
    cleaned = capi.host_text(capi._seed_clean, len(rows), capi.c_strings(names), capi.c_strings(rows), refusal=SeedError)
    return names, capi.split_lines(cleaned, len(rows))


def read_seed(path):
    """A seed alignment file (Stockholm or aligned FASTA, parse_seed) checked and without its all-gap columns
    (clean_seed): (names, rows), '-' for gaps"""
    with open(path, "rb") as fh:
        return clean_seed(*parse_seed(fh.read()))


def parse_seed_structure(text):
    """parse_seed with the seed's consensus structure: (names, rows, structure), the structure as the
    file holds it -- the `#=GC SS_cons` lines of a Stockholm seed's first alignment concatenated over its blocks, the record
    named SS_cons of an aligned-FASTA seed -- or None when the file has none."""
    data = text.encode("latin-1") if isinstance(text, str) else bytes(text)
    n, has = C.c_uint32(), C.c_int()
    got = capi.host_text(capi._seed_parse_structure, data, len(data), C.byref(n), C.byref(has), outs=3, refusal=SeedError)
    return capi.split_lines(got[0], n.value), capi.split_lines(got[1], n.value), got[2] if has.value else None


def clean_seed_structure(names, rows, structure):
    """clean_seed with the structure's characters: (names, rows, ss), ss a uint32 array over the cleaned columns, the partner
    column at the left column of a pair and 0xFFFFFFFF elsewhere.  `()`, `<>`, `[]`, `{}` are pairs, each kind matched with
    its own kind; letters and `. , : _ - ~` are unpaired; a pair that loses a column with the all-gap columns is dropped.
    Refuses (SeedError) what clean_seed refuses, any other character, a length that is not the rows', an unbalanced kind and
    pairs that cross once all kinds are merged."""
    names, rows = list(names), list(rows)
    if len(names) != len(rows):
        raise SeedError("seed: one name per row")
    st = structure.encode("latin-1") if isinstance(structure, str) else bytes(structure)
    if b"\0" in st:
        raise SeedError("seed: SS_cons holds a NUL byte")
    ss = np.zeros(max(len(rows[0]) if rows else 0, 1), np.uint32)
    cols = C.c_uint32()
    cleaned = capi.host_text(capi._seed_clean_structure, len(rows), capi.c_strings(names), capi.c_strings(rows), st, ss.ctypes.data,
                             C.byref(cols), refusal=SeedError)
    return names, capi.split_lines(cleaned, len(rows)), ss[:cols.value].copy()


def read_seed_structure(path):
    """read_seed with the seed's consensus structure: (names, rows, ss), ss as clean_seed_structure returns it, None when the
    file has no structure"""
    with open(path, "rb") as fh:
        names, rows, structure = parse_seed_structure(fh.read())
    if structure is None:
        return clean_seed(names, rows) + (None,)
    return clean_seed_structure(names, rows, structure)


def clean_seed_knots(names, rows, structure):
    """clean_seed_structure for a structure whose pairs may cross (dafs_host_seed_clean_structure_levels; DESIGN.md section 26;
    `dafs --knots`): (names, rows, ss, level), level a uint8 array over the cleaned columns with the pair's level at both of its
    columns and 0xFF at unpaired ones.  Groups, in this order: `()`, `[]`, `{}`, `<>`, then the letters A..Z, an upper-case
    letter opening and the same letter in lower case closing; each group is matched with itself.  After the all-gap columns
    have gone (a pair that loses a column is dropped), group after group goes to the lowest level at which none of its pairs
    crosses a pair already there.  Refuses (SeedError) what clean_seed refuses, any other character, a length that is not the
    rows', an unbalanced group and a group that would need a fifth level."""
    names, rows = list(names), list(rows)
    if len(names) != len(rows):
        raise SeedError("seed: one name per row")
    st = structure.encode("latin-1") if isinstance(structure, str) else bytes(structure)
    if b"\0" in st:
        raise SeedError("seed: SS_cons holds a NUL byte")
    width = max(len(rows[0]) if rows else 0, 1)
    ss, level = np.zeros(width, np.uint32), np.zeros(width, np.uint8)
    cols = C.c_uint32()
    cleaned = capi.host_text(capi._seed_clean_structure_levels, len(rows), capi.c_strings(names), capi.c_strings(rows), st, ss.ctypes.data,
                             level.ctypes.data, C.byref(cols), refusal=SeedError)
    return names, capi.split_lines(cleaned, len(rows)), ss[:cols.value].copy(), level[:cols.value].copy()


def read_seed_knots(path):
    """read_seed_structure with clean_seed_knots: (names, rows, ss, level), ss and level both None when the file has no
    structure"""
    with open(path, "rb") as fh:
        names, rows, structure = parse_seed_structure(fh.read())
    if structure is None:
        return clean_seed(names, rows) + (None, None)
    return clean_seed_knots(names, rows, structure)


def read_seed_pp(path):
    """The `#=GR <name> PP` lines of a Stockholm file's first alignment (dafs_host_seed_pp), read beside read_seed: per row of the
    file the PP characters over the columns read_seed keeps (a row without a PP line is all '.'), or None when the file holds no
    PP line"""
    with open(path, "rb") as fh:
        data = fh.read()
    n, has = C.c_uint32(), C.c_int()
    got = capi.host_text(capi._seed_pp, data, len(data), C.byref(n), C.byref(has), refusal=SeedError)
    return capi.split_lines(got, n.value) if has.value else None
