"""Plain-Python restatement of the text formats and memory estimates that libdafs_hip.so's host text code defines
(dafs_amd/csrc/host_text.cpp, called by the `dafs` command line and, through dafs_amd/stockholm.py and dafs_amd/pipeline.py, by
the Python driver): the Stockholm block and its PP / cov_SS_cons / RF lines, the --covariation and --pairwise-scores tables,
the seed reader and its refusals, the estimates and the greedy packing; and of DAFS::build_tree (host_tree.cpp).  Nothing
here calls the library: the tests compare it with the library byte for byte (test_text_cpu.py) and build the bytes the
command line must write from a Result's arrays (the GPU tests)."""
import heapq
import math
import re

import numpy as np

import covariation_ref

NONE = 0xFFFFFFFF

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

def build_tree(sim):
    """DAFS::build_tree, src/dafs.cpp:446-492.  Returns (score[2n-1], left, right) with -1 for leaves."""
    n = sim.shape[0]
    T = 2 * n - 1
    score = np.zeros(T, np.float32)
    left = -np.ones(T, np.int64)
    right = -np.ones(T, np.int64)
    d = np.zeros((n, n), np.float32)
    idx = [-1] * T
    for i in range(n):
        idx[i] = i
    pq = []
    for i in range(n - 1):
        for j in range(i + 1, n):
            d[i, j] = d[j, i] = sim[i, j]
            heapq.heappush(pq, (-float(sim[i, j]), -i, -j))  # max-heap on (sim, (i, j))
    cur = n
    while pq:
        s, a, b = heapq.heappop(pq)
        s, a, b = np.float32(-s), -a, -b
        if idx[a] != -1 and idx[b] != -1:
            l, r = idx[a], idx[b]
            idx[a] = idx[b] = -1
            for i in range(cur):
                if idx[i] != -1:
                    ii = idx[i]
                    v = np.float32(np.float32(d[ii, l] + d[ii, r]) * s) / np.float32(2)
                    d[ii, l] = d[l, ii] = v
                    heapq.heappush(pq, (-float(v), -i, -cur))
            score[cur] = s
            left[cur], right[cur] = a, b
            idx[cur] = l
            cur += 1
    return score, left, right


def family_bytes(lens):
    """Device memory one family takes in phase 1, estimated from the stores' sizes (bytes): per pair its row pointers in
    both matching stores, its entries (as the pair kernels reserve them: 24 per shorter-sequence column and direction, col
    + val, the relaxed copy and the interleaved copy of the transforms) and its dense consistency tile; per sequence its
    base-pairing tile and rows; the similarity block.  Not counted: the folding kernels' workspaces and the resident
    nodes of the progressive phase, which hold only the open nodes (tools/time_batch.py reports their measured peak)."""
    lens = [int(x) for x in lens]
    n = len(lens)
    b = 4 * n * n
    for x in range(n):
        b += 8 * lens[x] * lens[x] + 64 * lens[x] + 4096
        for y in range(x + 1, n):
            b += 8 * (lens[x] + lens[y] + 2) + 2 * min(lens[x], lens[y]) * 24 * 32 + 4 * lens[x] * lens[y]
    return b


def pack_families(sizes, max_bytes):
    """Sub-batches of the families (greedy, in input order) whose estimated sizes add up to at most max_bytes each; a
    family over the budget runs alone.  Returns lists of family indices."""
    out, cur, used = [], [], 0
    for k, b in enumerate(sizes):
        if cur and used + b > max_bytes:
            out.append(cur)
            cur, used = [], 0
        cur.append(k)
        used += b
    if cur:
        out.append(cur)
    return out


# per sub-batch, against the 288 GB of an MI355X.  A choice, not a measured limit.  Measured on 512 families of 5-15
# sequences of 80-200 nt (profiles/r04_a_time_batch.json): phase-1 estimate 8.6 GB (one sub-batch), peak of the
# progressive phase's resident nodes 6.0 GB, which family_bytes does not count.
DEFAULT_BATCH_BYTES = 16 << 30


def node_bytes(l1, l2):
    """Device memory of one resident node of l1 x l2 columns (bytes), the bound test_configs_gpu._node_bytes_bound states
    from capi_dd.cpp's nodes_open, folding arrays included: per cell of the two base-pairing matrices 19 + 25 bytes, per cell
    of the alignment tables 26 bytes plus the padded sweep-order copies, traceback slots, row arrays and slack."""
    l1, l2 = int(l1), int(l2)
    return (44 * (l1 * l1 + l2 * l2) + 26 * (l1 + 1) * (l2 + 1) + 8 * (l1 + 63) * (l2 + 64) + 512 * (l1 + 1) * ((l2 + 2048) // 2048)
            + 128 * (l1 + l2) + (1 << 14))


def pair_bytes(l1, l2):
    """Device memory of one two-sequence family of a pairwise run: its phase-1 stores (family_bytes) and its root node, which
    is resident for the whole progressive phase of the chunk (every pair's one node opens in the first round)."""
    return family_bytes([l1, l2]) + node_bytes(l1, l2)


def pair_chunks(lens, pairs, max_bytes):
    """The pairs (indices into `pairs`) in chunks of at most max_bytes of estimated device memory each (pair_bytes), greedy
    in pair order; a pair over the budget runs alone."""
    return pack_families([pair_bytes(lens[x], lens[y]) for x, y in pairs], max_bytes)


def _fmt9(v):
    """%.9g as C's printf writes it for the table (a NaN of either sign as "nan")"""
    v = float(v)
    return "nan" if v != v else "%.9g" % v


def pairwise_scores_tsv(names, pairs, sim, score, iterations):
    """The table of `dafs --pairwise FILE --pairwise-scores OUT` (the C++ writer in cli_main.cpp writes the same bytes): per
    pair, in pair order, "i<TAB>j<TAB>name_i<TAB>name_j<TAB>sim<TAB>score<TAB>iterations" with 1-based i, j and the floats
    as %.9g."""
    return "".join("%d\t%d\t%s\t%s\t%s\t%s\t%d\n" % (x + 1, y + 1, names[x], names[y], _fmt9(sim[x, y]), _fmt9(score[x, y]),
                                                     int(iterations[x, y])) for x, y in pairs)


COV_TABLE_E_MAX = 0.05  # the cut of the table's `other` pairs: fixed, as on the command line (e_max moves cov_SS_cons only)
_CANONICAL = ((0, 3), (3, 0), (2, 1), (1, 2), (2, 3), (3, 2))  # AU UA GC CG GU UG


def covariation_tsv(result):
    """The table of `dafs --covariation OUT` for one result with .covariation (the C++ writer in cli_main.cpp writes the same
    bytes): one line "c1<TAB>c2<TAB>kind<TAB>S<TAB>E<TAB>rows<TAB>canonical<TAB>types" per pair, columns 1-based, floats as
    %.9g.  First every consensus pair by ascending left column (kind ss); then every distinct pair {c, best(c)} that is no
    consensus pair and has E <= 0.05 (COV_TABLE_E_MAX, whatever the result's e_max), ordered by (c1, c2) (kind other), its
    counts taken from the rows."""
    cv, ss = result.covariation, result.ss
    lines, cons = [], set()
    for c in range(len(ss)):
        if int(ss[c]) != NONE:
            cons.add((c, int(ss[c])))
            lines.append("%d\t%d\tss\t%s\t%s\t%d\t%d\t%d\n" % (c + 1, int(ss[c]) + 1, _fmt9(cv["pair_score"][c]), _fmt9(cv["pair_e"][c]),
                                                                 int(cv["pair_rows"][c]), int(cv["pair_canonical"][c]), int(cv["pair_types"][c])))
    other = {}
    for c in range(len(ss)):
        b = int(cv["best"][c])
        if b == NONE or not float(cv["best_e"][c]) <= COV_TABLE_E_MAX:
            continue
        pr = (min(c, b), max(c, b))
        if pr not in cons and pr not in other:
            other[pr] = c
    code = covariation_ref.encode(result.rows) if other else None
    for (c1, c2), c in sorted(other.items()):
        both = (code[:, c1] < 4) & (code[:, c2] < 4)
        each = [int(((code[:, c1] == a) & (code[:, c2] == b)).sum()) for a, b in _CANONICAL]
        lines.append("%d\t%d\tother\t%s\t%s\t%d\t%d\t%d\n" % (c1 + 1, c2 + 1, _fmt9(cv["best_score"][c]), _fmt9(cv["best_e"][c]), int(both.sum()),
                                                                sum(each), sum(1 for v in each if v)))
    return "".join(lines)


def brackets(ss):
    """make_brackets (reference src/nussinov.cpp:401-413): '(' and ')' at the two columns of every pair, '.' elsewhere"""
    out = ["."] * len(ss)
    for c in range(len(ss)):
        if int(ss[c]) != NONE:
            out[c], out[int(ss[c])] = "(", ")"
    return "".join(out)


def result_block(res, headers, rf=None):
    """The Stockholm block of a pipeline Result (of run, run_batch, pairwise or add, with reliability=True) from its arrays:
    rows, ss, reliability, covariation and tree_line where it has them.  headers: the FASTA headers of its rows, in row
    order; rf: the result's .rf (pipeline.add)."""
    cov = None
    if hasattr(res, "covariation"):
        cov = cov_ss_cons(res.ss, res.covariation["pair_e"], res.covariation["e_max"])
    return block(getattr(res, "tree_line", None), names(headers), res.rows, res.reliability["residue"], res.reliability["col"],
                 brackets(res.ss), rf, cov)
