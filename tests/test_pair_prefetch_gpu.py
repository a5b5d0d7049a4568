"""GPU parity of the pair kernels where sweep 3's two-steps-ahead slab fetch and its unconditional, per-lane masked
record stores (pair_sweeps.h) can go wrong: the clamp of the fetch in the last two steps, slots of cells outside a
pair's grid, the W-1 / W seam, records in consecutive steps of one lane, and the dense form.  Every case is bit for bit
against the oracle, through test_pairhmm_gpu's checker, for both models and every group size.

The record stores go through a buffer descriptor of the wave's list plane and lanes without a record get an offset
outside it, so the capacity of a lane's list is what it was: test_pair_records_gpu's overflow set is not repeated."""
import numpy as np
import pytest

from test_pair_records_gpu import LOW_COMPLEXITY, _forced
from test_pairhmm_gpu import _check_set

pytestmark = pytest.mark.gpu

GROUPS = [16, 32, 64]
MODELS = [0, 1]


def _seqs(lengths, seed):
    rng = np.random.RandomState(seed)
    return ["".join("ACGU"[k] for k in rng.randint(0, 4, n)) for n in lengths]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("group", GROUPS)
def test_shortest_pairs(oracle, group, model):
    """nsteps = L1 + G with L1 = 1, 2, 3 (the fetch two steps ahead is clamped in the last two steps), and the same
    lengths as L2 (one lane owns every column)"""
    seqs = ["A", "AC", "ACG", "ACGU" * 5]
    _check_set(oracle, seqs, force_group=group, model=model)
    _check_set(oracle, seqs[::-1], force_group=group, model=model)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("group", GROUPS)
def test_unequal_pairs_in_one_wave(oracle, group, model):
    """Pairs of very different L1 share a wavefront (G = 16: four of them), so lanes run rows beyond their pair's L1, and
    with L2 far below G * WR whole lanes own no column: their slots are read unguarded and must not become entries"""
    _check_set(oracle, _seqs([2, 9, 33, 70], 17), force_group=group, model=model)


# one small W per group size; the lengths follow from G and W: L2 + 1 = G (W - 1) still runs the W-1 instantiation,
# L2 + 1 = G (W - 1) + 1 is the first that needs W
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("group,width", [(16, 3), (32, 2), (64, 2)])
def test_width_seam(oracle, group, width, model):
    n = group * (width - 1)
    _forced(oracle, _seqs([n - 1, n - 1, n - 1], 5), 0.01, group, width, model)  # every wave: W-1 columns per lane
    _forced(oracle, _seqs([n - 1, n, n], 6), 0.01, group, width, model)          # L2 = n: W columns per lane


@pytest.mark.parametrize("th", [0.01, 0.002])
@pytest.mark.parametrize("group", GROUPS)
def test_records_in_consecutive_steps(oracle, group, th):
    """test_pair_records_gpu asserts from the oracle that this set has entries in most lane-steps near the diagonal:
    a lane appends in consecutive steps, each store two steps behind the fetch it must not disturb"""
    for model in MODELS:
        _check_set(oracle, LOW_COMPLEXITY, th=th, force_group=group, model=model)


@pytest.mark.parametrize("model", MODELS)
def test_dense_form(oracle, model):
    """th = 0: the plane-and-rescan form, which stores into the slab it prefetches from"""
    seqs = _seqs([3, 18, 41], 9)
    for group in GROUPS:
        _check_set(oracle, seqs, th=0.0, force_group=group, model=model)
