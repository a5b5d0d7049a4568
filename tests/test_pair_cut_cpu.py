"""The cut of the pair-HMM kernel's candidate pick (dafs_hip_pair_cut, DESIGN.md section 5.1 "Sweep 2p"), no GPU.

The backward sweep keeps a cell as a candidate when its log posterior can reach cut(th); the claim the kernel rests on is
that NO float below the cut can be an entry: every float v < cut(th) has EXP(v) <= th or is <= -16 (where EXP is 0).
EXP is restated here in numpy (ScoreType.h:37-57 with the constants of pc_math.h: Horner in float64, narrowed to
float32) and evaluated on EVERY float of [-16, -0.5), once; M[k] is its running maximum over the floats up to the k-th.
Then, for every th of the grid:
  M(prev(cut(th))) <= th          nothing below the cut can be an entry
  cut(th) >= log(th) - 1/16       the cut is not uselessly low (th below EXP(-0.5); above it the cut is -0.5)
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# pieces of EXP, k4 .. k0: (-0.5, 0], (-1, -0.5], (-2, -1], (-4, -2], (-8, -4], (-16, -8]
PIECES = [
    (-0.5, (0.03254409303190190000, 0.16280432765779600000, 0.49929760485974900000, 0.99995149601363700000, 0.99999925508501600000)),
    (-1.0, (0.01973899026052090000, 0.13822379685007000000, 0.48056651562365000000, 0.99326940370383500000, 0.99906756856399500000)),
    (-2.0, (0.00940528203591384000, 0.09414963667859410000, 0.40825793595877300000, 0.93933625499130400000, 0.98369508190545300000)),
    (-4.0, (0.00217245711583303000, 0.03484829428350620000, 0.22118199801337800000, 0.67049462206469500000, 0.83556950223398500000)),
    (-8.0, (0.00012398771025456900, 0.00349155785951272000, 0.03727721426017900000, 0.17974997741536900000, 0.33249299994217400000)),
    (-16.0, (0.00000051741713416603, 0.00002721456879608080, 0.00053418601865636800, 0.00464101989351936000, 0.01507447981459420000)),
]


def exp_ref(xf):
    """EXP of a float32 array with values <= 0"""
    xf = np.asarray(xf, np.float32)
    x = xf.astype(np.float64)
    out = np.zeros(xf.shape, np.float32)  # x <= -16
    todo = np.ones(xf.shape, bool)
    for lower, (k4, k3, k2, k1, k0) in PIECES:  # the first piece whose open lower end lies below x
        m = todo & (xf > np.float32(lower))
        xm = x[m]
        out[m] = ((((k4 * xm + k3) * xm + k2) * xm + k1) * xm + k0).astype(np.float32)
        todo &= ~m
    return out


@pytest.fixture(scope="module")
def lib():
    so = C.CDLL(os.path.join(ROOT, "dafs_amd", "libdafs_hip.so"))
    so.dafs_hip_pair_cut.restype = C.c_float
    so.dafs_hip_pair_cut.argtypes = [C.c_float]
    return so


def grid():
    ths = [0.01, 0.002]
    ths += list(np.exp(np.linspace(math.log(0.002), math.log(0.6), 400)))
    top = float(exp_ref([-0.5])[0])
    ths += [top, float(np.nextafter(np.float32(top), np.float32(1))), 0.61, 0.7, 0.999, 1.0]
    return [np.float32(t) for t in ths]


@pytest.fixture(scope="module")
def scan(lib):
    """One pass over every float of [-16, -0.5), ascending: ({th: (cut(th), running maximum of EXP over the floats from -16
    up to prev(cut(th)))}, the first float at which the running maximum exceeds 0.01)"""
    hi = int(np.float32(-16.0).view(np.uint32))  # negative floats: a larger pattern is a lower value
    lo = int(np.float32(-0.5).view(np.uint32))
    cuts = {th: np.float32(lib.dafs_hip_pair_cut(C.c_float(float(th)))) for th in grid()}
    want = {}  # index in the ascending scan (0: -16) -> running maximum there
    for cut in cuts.values():
        assert np.float32(-16.0) <= cut <= np.float32(-0.5), cut
        below = np.nextafter(cut, np.float32(-np.inf))  # prev(cut)
        if below > np.float32(-16.0):
            want[hi - int(below.view(np.uint32))] = None
    idx = np.array(sorted(want), np.int64)
    best, first_above = np.float32(0.0), None
    chunk = 1 << 22
    for a in range(0, hi - lo, chunk):
        b = min(a + chunk, hi - lo)
        v = (hi - np.arange(a, b, dtype=np.int64)).astype(np.uint32).view(np.float32)
        m = np.maximum.accumulate(exp_ref(v))
        np.maximum(m, best, out=m)
        for k in idx[(idx >= a) & (idx < b)]:
            want[int(k)] = m[k - a]
        if first_above is None and m[-1] > np.float32(0.01):
            first_above = v[int(np.searchsorted(m, np.float32(0.01), side="right"))]
        best = m[-1]
    res = {}
    for th, cut in cuts.items():
        below = np.nextafter(cut, np.float32(-np.inf))
        res[th] = (cut, want[hi - int(below.view(np.uint32))] if below > np.float32(-16.0) else np.float32(0.0))
    return res, first_above


def test_exp_restatement_matches_the_reference_point(scan):
    """scanning th = 0.01: no float below -4.60885048 reaches it, the float there does (log th = -4.60517)"""
    assert abs(float(scan[1]) - (-4.60885048)) < 2e-6, scan[1]


def test_nothing_below_the_cut_is_an_entry_and_the_cut_is_tight(scan):
    top = exp_ref([-0.5])[0]
    for th, (cut, below_max) in scan[0].items():
        assert below_max <= th, (th, cut, below_max)
        if th > top:
            assert cut == np.float32(-0.5), (th, cut)
        else:
            assert float(cut) >= math.log(float(th)) - 1.0 / 16.0, (th, cut, math.log(float(th)))


def test_the_cut_never_decreases_with_th(lib):
    cuts = [lib.dafs_hip_pair_cut(C.c_float(float(t))) for t in sorted(grid())]
    assert all(a <= b for a, b in zip(cuts, cuts[1:]))
