"""Plain-Python restatement of DESIGN.md section 19 "Comparing two alignments": the yardstick of test_compare_cpu.py and
test_compare_gpu.py.  Every count is a Python integer; a quotient is float(a) / float(b), NaN for a zero denominator.  The pair
counts come straight from their definition (quadratic over the residues of the two rows), not from cnt, so that the two routes
check each other."""
import numpy as np

from alistat_ref import NONE, cells  # noqa: F401  (cells: text rows -> codes)

NAN = float("nan")
CLASSES = 11


def quotient(a, b):
    return float(a) / float(b) if b else NAN


def keys(cell_r, cell_t, use_r=None, use_t=None):
    """per row the list over its residues k of (a, b, column in R, column in T): a, b are the columns where they are used, else
    None.  ValueError naming the row (1-based) whose residue codes differ."""
    out = []
    for r, (x, y) in enumerate(zip(cell_r, cell_t)):
        cr = [c for c, v in enumerate(x) if v <= 4]
        ct = [c for c, v in enumerate(y) if v <= 4]
        if [x[c] for c in cr] != [y[c] for c in ct]:
            raise ValueError("row %d holds different residues in the two alignments" % (r + 1))
        out.append([(c if use_r is None or use_r[c] else None, d if use_t is None or use_t[d] else None, c, d) for c, d in zip(cr, ct)])
    return out


def pair_counts(key):
    """(shared, refp, testp), each n x n, from the definition: the residue pairs (k of row r, l of row s), r != s, with equal keys
    that are not None.  Every residue of r is held against every residue of s (numpy does the nres(r) x nres(s) comparisons at
    once); r < s is computed and mirrored, the definition being symmetric."""
    n = len(key)
    a = [np.array([-1 if x[0] is None else x[0] for x in row], np.int64) for row in key]
    b = [np.array([-1 if x[1] is None else x[1] for x in row], np.int64) for row in key]
    shared = [[0] * n for _ in range(n)]
    refp = [[0] * n for _ in range(n)]
    testp = [[0] * n for _ in range(n)]
    for r in range(n):
        for s in range(r + 1, n):
            ea = (a[r][:, None] == a[s][None, :]) & (a[r][:, None] >= 0)
            eb = (b[r][:, None] == b[s][None, :]) & (b[r][:, None] >= 0)
            refp[r][s] = refp[s][r] = int(ea.sum())
            testp[r][s] = testp[s][r] = int(eb.sum())
            shared[r][s] = shared[s][r] = int((ea & eb).sum())
    return shared, refp, testp


def left_pairs(ss):
    """the pairs (c, d), c < d, of a partner array in either form"""
    return set() if ss is None else {(c, d) for c, d in enumerate(ss) if d != NONE and c < d}


def compare(cell_r, cell_t, use_r=None, use_t=None, ss_r=None, ss_t=None, pp=None):
    """every output of dafs_hip_alignment_compare but the pair matrices (pair_counts), as a dict of lists and numbers"""
    key = keys(cell_r, cell_t, use_r, use_t)
    n, len_r, len_t = len(cell_r), len(cell_r[0]), len(cell_t[0])
    k = [0] * len_r
    m = [0] * len_t
    cnt = {}
    for row in key:
        for a, b, _, _ in row:
            if a is not None:
                k[a] += 1
            if b is not None:
                m[b] += 1
            if a is not None and b is not None:
                cnt[(a, b)] = cnt.get((a, b), 0) + 1
    out = dict(residues=[len(row) for row in key], k=k, m=m, shared=[], refp=[], testp=[])
    pp_count = [[0] * CLASSES for _ in range(3)]
    for r, row in enumerate(key):
        sh = rp = tp = 0
        for a, b, _, d in row:
            refn = k[a] - 1 if a is not None else 0
            testn = m[b] - 1 if b is not None else 0
            shr = cnt[(a, b)] - 1 if a is not None and b is not None else 0
            sh, rp, tp = sh + shr, rp + refn, tp + testn
            if pp is not None and pp[r][d] != 255:
                q = pp[r][d]
                pp_count[0][q] += 1
                pp_count[1][q] += refn
                pp_count[2][q] += shr
        out["shared"].append(sh)
        out["refp"].append(rp)
        out["testp"].append(tp)
    out["row_sps"] = [quotient(a, b) for a, b in zip(out["shared"], out["refp"])]
    out["row_ppv"] = [quotient(a, b) for a, b in zip(out["shared"], out["testp"])]
    tot = [sum(out[q]) for q in ("shared", "refp", "testp")]
    assert all(t % 2 == 0 for t in tot)
    out["total_shared"], out["total_refp"], out["total_testp"] = (t // 2 for t in tot)
    out["sps"] = quotient(out["total_shared"], out["total_refp"])
    out["ppv"] = quotient(out["total_shared"], out["total_testp"])
    out["colref"] = [x * (x - 1) // 2 for x in k]
    by_a = [[] for _ in range(len_r)]  # per column of R its (d, cnt(c, d)) with cnt > 0
    for (a, b), v in cnt.items():
        by_a[a].append((b, v))
    out["colshared"] = [sum(v * (v - 1) // 2 for _, v in by_a[c]) for c in range(len_r)]
    out["reproduced"] = [k[c] >= 2 and any(v == k[c] == m[d] for d, v in by_a[c]) for c in range(len_r)]
    out["tc_reproduced"] = sum(out["reproduced"])
    out["tc_columns"] = sum(1 for x in k if x >= 2)
    out["tc"] = quotient(out["tc_reproduced"], out["tc_columns"])
    if pp is not None:
        out["pp_residues"], out["pp_ref"], out["pp_shared"] = pp_count
        out["pp_accuracy"] = [quotient(a, b) for a, b in zip(pp_count[2], pp_count[1])]
    if ss_r is not None and ss_t is not None:
        pr, pt = left_pairs(ss_r), left_pairs(ss_t)
        out["tp"], out["nref"], out["ntest"] = [], [], []
        for row in key:
            at_r = {c: i for i, (_, _, c, _) in enumerate(row)}
            at_t = {d: i for i, (_, _, _, d) in enumerate(row)}
            in_r = {(at_r[c], at_r[d]) for c, d in pr if c in at_r and d in at_r}
            in_t = {(at_t[c], at_t[d]) for c, d in pt if c in at_t and d in at_t}
            out["tp"].append(len(in_r & in_t))
            out["nref"].append(len(in_r))
            out["ntest"].append(len(in_t))
        tp, nref, ntest = (sum(out[q]) for q in ("tp", "nref", "ntest"))
        out["total_tp"], out["total_nref"], out["total_ntest"] = tp, nref, ntest
        out["sensitivity"], out["ss_ppv"], out["f"] = quotient(tp, nref), quotient(tp, ntest), quotient(2 * tp, nref + ntest)
    return out


def brackets(text):
    """a nested bracket string -> the partner array in left-column form"""
    ss, stack = [NONE] * len(text), []
    for c, ch in enumerate(text):
        if ch == "(":
            stack.append(c)
        elif ch == ")":
            ss[stack.pop()] = c
    assert not stack
    return ss


def fmt(v):
    """%.9g, nan for a NaN"""
    return "nan" if v != v else "%.9g" % v


def table(names, only_ref, only_test, out):
    """the --compare table from compare()'s dict"""
    n = len(names)
    lines = ["# rows %d only_ref %d only_test %d columns_ref %d columns_test %d" % (n, only_ref, only_test, len(out["k"]), len(out["m"])),
             "# pairs shared %d ref %d test %d sps %s ppv %s" % (out["total_shared"], out["total_refp"], out["total_testp"], fmt(out["sps"]), fmt(out["ppv"])),
             "# columns reproduced %d of %d tc %s" % (out["tc_reproduced"], out["tc_columns"], fmt(out["tc"]))]
    if "tp" in out:
        lines.append("# structure tp %d ref %d test %d sensitivity %s ppv %s f %s" % (out["total_tp"], out["total_nref"], out["total_ntest"],
                                                                                   fmt(out["sensitivity"]), fmt(out["ss_ppv"]), fmt(out["f"])))
    if "pp_residues" in out:
        for q in range(CLASSES):
            if out["pp_residues"][q]:
                lines.append("# pp %s %d %d %d %s" % ("0123456789*"[q], out["pp_residues"][q], out["pp_ref"][q], out["pp_shared"][q], fmt(out["pp_accuracy"][q])))
    for r in range(n):
        f = [str(r + 1), names[r], str(out["residues"][r]), str(out["shared"][r]), str(out["refp"][r]), str(out["testp"][r]), fmt(out["row_sps"][r]),
             fmt(out["row_ppv"][r])]
        if "tp" in out:
            f += [str(out["tp"][r]), str(out["nref"][r]), str(out["ntest"][r])]
        lines.append("\t".join(f))
    return "\n".join(lines) + "\n"


def columns_table(out):
    return "".join("%d\t%d\t%d\t%d\t%d\n" % (c + 1, out["k"][c], out["colref"][c], out["colshared"][c], out["reproduced"][c]) for c in range(len(out["k"])))


def matrix_table(names, shared, refp, testp):
    n = len(names)
    return "".join("%d\t%d\t%s\t%s\t%d\t%d\t%d\t%s\t%s\n" % (r + 1, s + 1, names[r], names[s], shared[r][s], refp[r][s], testp[r][s],
                                                            fmt(quotient(shared[r][s], refp[r][s])), fmt(quotient(shared[r][s], testp[r][s])))
                   for r in range(n) for s in range(r + 1, n))
