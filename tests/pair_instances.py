"""The compiled instances (G, W) of the pair kernels, k_pairhmm3 (ProbCons, model 0) and k_pairhmm5 (CONTRAlign, model 1),
and inputs that reach the edges of an instance.  A helper module, not a conftest.

TABLES is the tests' statement of what is compiled; discover() asks the library (the plan functions, host only), and
test_pair_instances_cpu.py holds the two against each other.  An instance holds every sweep twice (WR = W and WR = W - 1
columns per lane) and pair_finish in a sparse and a dense form; fits() and ROW_LIMIT restate the two bounds a launch
puts on the lengths."""
import os
from contextlib import contextmanager

GROUPS = (16, 32, 64)
TABLES = {
    0: [(16, 2), (16, 3), (16, 4), (16, 5), (16, 6), (16, 7), (16, 8), (16, 10), (16, 11), (16, 12), (16, 14), (16, 16),
        (32, 2), (32, 3), (32, 4), (32, 5), (32, 6), (32, 7), (32, 8), (32, 10), (32, 12), (32, 14), (32, 16),
        (64, 1), (64, 2), (64, 3), (64, 4), (64, 5), (64, 6), (64, 7), (64, 8), (64, 10), (64, 12), (64, 14), (64, 16), (64, 24), (64, 32)],
    1: [(16, 2), (16, 3), (16, 4), (16, 5), (16, 6), (16, 8), (16, 10), (16, 11), (16, 12),
        (32, 2), (32, 3), (32, 4), (32, 5), (32, 6), (32, 7), (32, 8), (32, 10), (32, 12),
        (64, 1), (64, 2), (64, 3), (64, 4), (64, 5), (64, 6), (64, 7), (64, 8), (64, 10), (64, 12), (64, 16)],
}
assert [len(TABLES[m]) for m in (0, 1)] == [37, 29]

ROWPTR_LDS_MAX = 60 * 1024  # bytes of LDS a launch gives the row pointers: 4 wavefronts x 64/G groups x (max_len1 + 1) words
ROW_LIMIT = {16: 959, 32: 1919, 64: 3839}  # so the longest first sequence of a group size
assert all(4 * (64 // g) * (n + 1) * 4 <= ROWPTR_LDS_MAX < 4 * (64 // g) * (n + 2) * 4 for g, n in ROW_LIMIT.items())


def widths(model, group):
    return [w for g, w in TABLES[model] if g == group]


def rowptr_lds(group, max_len1):
    return 4 * (64 // group) * (max_len1 + 1) * 4


def fits(group, width, max_len1, max_len2):
    """the two bounds of a launch: the columns on the lanes, the row pointers in LDS"""
    return group * width >= max_len2 + 1 and rowptr_lds(group, max_len1) <= ROWPTR_LDS_MAX


@contextmanager
def forced(group=None, width=None):
    """DAFS_HIP_FORCE_GROUP / DAFS_HIP_FORCE_WIDTH for plan calls of this process, then whatever was set before"""
    names = {"DAFS_HIP_FORCE_GROUP": group, "DAFS_HIP_FORCE_WIDTH": width}
    old = {k: os.environ.get(k) for k in names}
    try:
        for k, v in names.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def plan_fn(model):
    from dafs_amd import capi
    return capi.pairhmm5_plan if model else capi.pairhmm_plan


def discover(model):
    """The instances the library holds, in TABLES' order: (G, W) exists where the plan call, forced to it, accepts the
    widest second sequence it can take (max_len2 = G * W - 1).  Host only: no device call is made."""
    from dafs_amd import capi
    plan, found = capi.PairhmmPlan(), []
    for g in GROUPS:
        for w in range(1, 33):
            with forced(g, w):
                rc = plan_fn(model)(1, 10, g * w - 1, plan)
            if rc == 0:
                assert (plan.group, plan.width) == (g, w), (g, w, plan.group, plan.width)
                found.append((g, w))
            else:
                assert rc == -4, (g, w, rc)  # DAFS_HIP_ETOOLONG: nothing is left after the filter
    return found


def random_seq(rng, n):
    return "".join(rng.choice("ACGU") for _ in range(n))


def planted(rng, short, L2):
    """A random ACGU sequence of length L2 that carries a copy of `short` at its start, at its end and, from
    L2 >= 4 * len(short) on, in the middle; for L2 < 2 * len(short) + 2 it is `short` repeated and cut to L2.  Aligned with
    `short`, the copies at the ends put posterior mass into the first and the last column (and row)."""
    n = len(short)
    assert n >= 1 and L2 >= 1
    if L2 < 2 * n + 2:
        return (short * (L2 // n + 1))[:L2]
    s = list(random_seq(rng, L2))
    s[:n] = short
    s[L2 - n:] = short
    if L2 >= 4 * n:
        m = (L2 - n) // 2
        s[m:m + n] = short
    return "".join(s)


def edge_lengths(group, width):
    """second-sequence lengths at the edges of instance (G, W): exact fit of the W form, exact fit of the W-1 form, and the
    W form at its smallest (column L2 on the first lane of the last column slot, the lanes behind it empty)"""
    if width == 1:
        return [group - 1]
    return [group * width - 1, group * (width - 1) - 1, group * (width - 1)]


def corners(rp, col, L1, L2):
    """(entry in the first row, the last row, the first column, the last column) of a CSR answer of the oracle"""
    import numpy as np
    rp = np.asarray(rp, np.int64)
    return (bool(rp[1] > rp[0]), bool(rp[L1] > rp[L1 - 1]), bool((col == 0).any()), bool((col == L2 - 1).any()))
