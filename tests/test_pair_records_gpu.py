"""GPU parity of the pair kernels' entry records (pair_sweeps.h: one record per lane and step in sweep 3, replayed in
sweep 4) where they are stressed: many entries in one lane-step, and lists that fill up and send the pair kernels to
the dense fallback.  Bit for bit against the oracle, through test_pairhmm_gpu's checker."""
import os

import numpy as np
import pytest

from test_pairhmm_gpu import _check_set

pytestmark = pytest.mark.gpu

# low-complexity pairs of different lengths: the gaps can sit anywhere, so the posteriors spread over wide bands and
# most lane-steps near the diagonal hold several entries
LOW_COMPLEXITY = ["A" * 60, "A" * 45, "AAAAAAAAAAGAAAAAAAAAAAAAAGAAAAAAAAAAAAAAGAAAAAAAA", "AC" * 28, "ACA" * 17, "GGGGGGGGGGAGGGGGGGGGGGG"]


def _forced(oracle, seqs, th, group, width, model=0):
    os.environ["DAFS_HIP_FORCE_WIDTH"] = str(width)
    try:
        _check_set(oracle, seqs, th=th, force_group=group, model=model)
    finally:
        os.environ.pop("DAFS_HIP_FORCE_WIDTH", None)


def _max_entries_per_row_run(oracle, seqs, th):
    best = 0
    for i in range(len(seqs)):
        for j in range(i + 1, len(seqs)):
            rp, col, _ = oracle.align_calculate(seqs[i], seqs[j], th, 0)
            best = max(best, int(np.diff(rp).max()))
    return best


@pytest.mark.parametrize("th", [0.002, 0.01])
@pytest.mark.parametrize("group", [16, 32, 64])
def test_many_entries_per_step(oracle, group, th):
    assert _max_entries_per_row_run(oracle, LOW_COMPLEXITY, th) >= 8  # rows with entries in more than one lane's columns
    _check_set(oracle, LOW_COMPLEXITY, th=th, force_group=group)
    _check_set(oracle, LOW_COMPLEXITY, th=th, force_group=group, model=1)


def test_full_lists_take_the_dense_form(oracle):
    """One column per lane (G = 64, W = 1): a record is 16 bytes and a lane's list holds (L1max + 64) / 4 of them, so a
    column with entries in more rows than that fills its list; the oracle confirms that the set gets there."""
    seqs = ["A" * 60, "A" * 30, "A" * 15, "A" * 45 + "C" * 5]
    th = 0.002
    cap = (max(len(s) for s in seqs) + 64) // 4
    most = 0
    for i in range(len(seqs)):
        for j in range(i + 1, len(seqs)):
            _, col, _ = oracle.align_calculate(seqs[i], seqs[j], th, 0)
            most = max(most, int(np.bincount(col).max()))
    assert most > cap, (most, cap)
    _forced(oracle, seqs, th, 64, 1)
    # the same set through the W = 2 instance: its waves still run one column per lane (every pair fits), but in a plane
    # twice as large, where no list fills up: the record path alone
    _forced(oracle, seqs, th, 64, 2)
