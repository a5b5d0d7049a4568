"""GPU parity of the pair kernels' persistent wavefronts over many rounds of pairs, and on scratch that other pairs, the
other model or nobody has written (pair_sweeps.h, pairhmm3.hip, pairhmm5.hip).  A wavefront takes a batch of 64/G pairs
from a device counter, runs the four sweeps and comes back for the next batch; between batches it keeps its scratch
planes (the DP slab and sweep 3's entry lists), its piece of LDS for the row pointers and its staging window.  The other
pair tests give every wavefront one batch on freshly reserved scratch.  Here: four wavefronts take up to 65 batches (A),
a launch starts on the slab and the lists of another launch (B), on scratch filled with NaN, +inf or 1.0 (C), runs out
of pool in the middle of the rounds (D), and one Context serves both models in turn (E).

Everything is bit for bit against the oracle (pair_raw.check for the raw launches), so no tolerance is involved.  Every
property of a set that depends on lengths or posteriors is asserted from the oracle before the set goes to the device."""
import random

import numpy as np
import pytest

import pair_raw
from dafs_amd import synth
from test_pair_records_gpu import LOW_COMPLEXITY
from test_pairhmm_gpu import _check_set

pytestmark = pytest.mark.gpu

MODELS = (0, 1)
NAN, INF, ONE = 0xFFFFFFFF, 0x7F800000, 0x3F800000
FILL = 0x3F800000  # what a first launch starts on where the fill is not the subject: 1.0, a posterior above every threshold


def _rand(n, seed):
    r = random.Random(seed)
    return "".join(r.choice("ACGU") for _ in range(n))


# ---- the set of tests A, C and D: 65 tasks over 12 sequences -------------------------------------------------------
SEQS = [_rand(n, 100 + n) for n in (1, 2, 3, 9, 17, 31, 33, 47, 63, 70)] + [LOW_COMPLEXITY[2], LOW_COMPLEXITY[1]]  # + 49 and 45 residues


def _tasks():
    """65 of the 66 pairs (65 = 1 mod 4 and 1 mod 2: at G = 16 and G = 32 the last batch has inactive groups, in a
    wavefront that was active before), every third one with the longer sequence second"""
    pairs = [(x, y) for x in range(len(SEQS)) for y in range(x + 1, len(SEQS))]
    pairs.remove((5, 6))
    out = []
    for k, (x, y) in enumerate(pairs):
        longer_first = len(SEQS[x]) >= len(SEQS[y])
        out.append((x, y) if longer_first == (k % 3 != 1) else (y, x))
    return out


def _cost(t):
    return len(SEQS[t[0]]) * len(SEQS[t[1]])


TASKS = _tasks()
ORDERS = {
    "descending": sorted(TASKS, key=_cost, reverse=True),  # the production order (stable, as capi_align.cpp sorts)
    "ascending": sorted(TASKS, key=_cost),
    "shuffled": random.Random(65).sample(TASKS, len(TASKS)),
}


def _batch_steps(order, group):
    """nsteps - G of every batch: the longest first sequence among its 64/G tasks"""
    ng = 64 // group
    return [max(len(SEQS[x]) for x, _ in order[b:b + ng]) for b in range(0, len(order), ng)]


def _longest_monotone_run(v, down):
    """length of the longest subsequence of v that never rises (down) / never falls"""
    best = [1] * len(v)
    for j in range(len(v)):
        for i in range(j):
            if (v[i] >= v[j]) if down else (v[i] <= v[j]):
                best[j] = max(best[j], best[i] + 1)
    return max(best)


def _assert_rounds(group):
    """What the lengths alone guarantee for four wavefronts (see test_many_rounds_on_four_wavefronts)."""
    assert len(TASKS) == 65 and len(set(TASKS)) == 65
    assert any(len(SEQS[x]) > len(SEQS[y]) for x, y in TASKS) and any(len(SEQS[x]) < len(SEQS[y]) for x, y in TASKS)
    nbatches = -(-65 // (64 // group))
    assert nbatches == {16: 17, 32: 33, 64: 65}[group]
    most = -(-nbatches // 4)  # some wavefront runs at least this many batches
    assert most >= 5
    for name in ("descending", "ascending"):
        costs = [_cost(t) for t in ORDERS[name]]
        assert costs == sorted(costs, reverse=name == "descending")
    # At one pair per batch (G = 64) the lengths give more: no `most` batches, in the counter's order, whose step counts
    # all go the wrong way, so the wavefront with `most` batches has at least one transition to a strictly shorter batch
    # (descending) / a strictly longer one (ascending).  With 2 or 4 pairs per batch the longest first sequences lead
    # too many batches for that argument.
    if group == 64:
        assert _longest_monotone_run(_batch_steps(ORDERS["descending"], group), down=False) < most
        assert _longest_monotone_run(_batch_steps(ORDERS["ascending"], group), down=True) < most


def _launches_a(oracle, orders, fills=(FILL,)):
    return [pair_raw.spec(oracle, model, 0.01, SEQS, ORDERS[o], fill, nwaves=4) for model in MODELS for o in orders for fill in fills]


def _check_all(oracle, outs, nwaves=None):
    for out in outs:
        L = out["spec"]
        if nwaves:
            g = pair_raw.geometry(out)
            assert g["nwaves"] == nwaves and g["planned_nwaves"] >= nwaves, g
        pair_raw.check(oracle, out, L["seqs"], L["tasks"], L["th"], L["model"])


@pytest.mark.parametrize("group,window", [(16, None), (32, None), (64, None), (16, 16)])
def test_many_rounds_on_four_wavefronts(oracle, tmp_path, group, window):
    """A.  65 tasks on nwaves = 4, so 17 (G = 16), 33 or 65 batches on four wavefronts, in three task orders: cost
    descending (production: a wavefront's next batch is cheaper -- stale long rows in its row pointers, stale slab steps
    beyond nsteps), cost ascending (steps and rows it never wrote before) and a fixed shuffle.  With the staging window
    forced to 16 positions (descending order only) the window is reused many times per pair and per round.

    Guaranteed, by pigeonhole: some wavefront runs at least ceil(batches / 4) >= 5 batches, and since a wavefront takes
    its batches in the counter's order, each of its transitions in a monotone order goes to a batch of no higher
    (descending) / no lower (ascending) cost.  Cost is len1 * len2, so a single transition may still go to a longer or an
    equal first sequence; at G = 64 _assert_rounds shows from the lengths that the wavefront with the most batches has
    at least one transition to a strictly smaller (descending) / larger (ascending) step count.  Not guaranteed: which
    wavefront takes which batch -- that is the device counter's choice, and the test cannot see it or pin a transition
    to a wavefront.  test_stale_scratch_of_another_launch makes the state of the scratch certain instead."""
    _assert_rounds(group)
    orders = ("descending",) if window else ("descending", "ascending", "shuffled")
    outs = pair_raw.run(tmp_path, _launches_a(oracle, orders), env={"DAFS_HIP_FORCE_GROUP": group, "DAFS_HIP_EMIT_WINDOW": window})
    assert all(pair_raw.geometry(o)["group"] == group for o in outs)
    _check_all(oracle, outs, nwaves=4)


# ---- B: two launches on one scratch ------------------------------------------------------------------------------
def _all_pairs(n):
    return [(x, y) for x in range(n) for y in range(x + 1, n)]


def _most_entries_in_a_column(oracle, seqs, tasks, th, model):
    return max(int(np.bincount(pair_raw.want(oracle, seqs[x], seqs[y], th, model)[1], minlength=1).max()) for x, y in tasks)


def _most_entries_in_a_row(oracle, seqs, tasks, th, model):
    return max(int(np.diff(pair_raw.want(oracle, seqs[x], seqs[y], th, model)[0]).max()) for x, y in tasks)


DENSE_SET = ["A" * 60, "A" * 30, "A" * 15, "A" * 45 + "C" * 5]  # test_full_lists_take_the_dense_form
SHORT_SET = [_rand(n, 200 + n) for n in (12, 20, 35, 50)]
WIDE = [_rand(50, 1), _rand(33, 2)], [_rand(n, n) for n in (64, 67, 70)], [_rand(n, n) for n in (40, 62, 63)]
EMPTY_SET = [s for _, s in synth.random_set(6, 40, seed=7)]  # test_empty_and_nearly_empty_pairs


def _stale_cases(oracle, case, model):
    """(first launch, second launch) as (seqs, tasks, th), in the orders the case runs them"""
    if case == "width":  # G = 32, W = 3: second sequences of 64 .. 70 residues take W columns per lane, up to 63 take W - 1
        firsts, longs, shorts = WIDE
        seqs = firsts + longs + shorts
        wide = (seqs, [(f, 2 + k) for f in range(2) for k in range(3)], 0.01)
        narrow = (seqs, [(f, 5 + k) for f in range(2) for k in range(3)], 0.01)
        assert all(64 <= len(seqs[y]) <= 70 for _, y in wide[1]) and all(len(seqs[y]) <= 63 for _, y in narrow[1])
        return [(wide, narrow), (narrow, wide)]
    if case == "dense":  # G = 64, W = 1: full lists, the dense form leaves posteriors in the slab; then the record form
        full = (DENSE_SET, _all_pairs(4), 0.002)
        short = (SHORT_SET, _all_pairs(4), 0.01)
        cap = (max(len(s) for s in DENSE_SET + SHORT_SET) + 64) // 4  # records of a lane's list (16 bytes each) under the common plan
        assert _most_entries_in_a_column(oracle, *full, model) > cap, "the lists of the first set do not fill"
        assert _most_entries_in_a_column(oracle, *short, model) <= cap, "the short pairs leave the record form"
        return [(full, short), (short, full)]
    if case == "th0":  # dense from the start (th = 0), then the record form on the same sequences
        seqs = [_rand(n, 300 + n) for n in (3, 18, 29, 41)]
        return [((seqs, _all_pairs(4), 0.0), (seqs, _all_pairs(4), 0.01))]
    assert case == "empty"  # records in most lane-steps, then pairs with no entry or next to none
    busy = (LOW_COMPLEXITY, _all_pairs(6), 0.01)
    assert _most_entries_in_a_row(oracle, *busy, model) >= 8
    pairs = _all_pairs(len(EMPTY_SET))
    if model == 1:  # CONTRAlign at th = 0.9: not one entry (as in test_empty_and_nearly_empty_pairs)
        assert not any(pair_raw.nnz(oracle, EMPTY_SET, pairs, 0.9, 1))
        # with no entry in a whole wavefront sweep 4 does not look at the lists at all; at th = 0.6 pairs with none sit
        # beside pairs with a few, so lanes without a record wait while others walk theirs
        few = pair_raw.nnz(oracle, EMPTY_SET, pairs, 0.6, 1)
        assert min(few) == 0 and 1 <= sum(1 for k in few if k) <= 8 and max(few) <= 14, few
        return [(busy, (EMPTY_SET, pairs, 0.9)), (busy, (EMPTY_SET, pairs, 0.6))]
    # ProbCons keeps a few entries of every pair at th = 0.9, so most lanes of a pair have no record; at th = 1 no
    # posterior is above the threshold and no lane has one
    few = pair_raw.nnz(oracle, EMPTY_SET, pairs, 0.9, 0)
    assert min(few) >= 1 and max(few) <= 14, few
    assert not any(pair_raw.nnz(oracle, EMPTY_SET, pairs, 1.0, 0))
    return [(busy, (EMPTY_SET, pairs, 0.9)), (busy, (EMPTY_SET, pairs, 1.0))]


STALE = {"width": (32, 3), "dense": (64, 1), "th0": (16, 3), "empty": (32, 2)}


def _launches_b(oracle, case):
    launches = []
    for model in MODELS:
        for first, second in _stale_cases(oracle, case, model):
            common = (max(len(first[1]), len(second[1])),
                      max(len(s[x]) for s, t, _ in (first, second) for x, _ in t), max(len(s[y]) for s, t, _ in (first, second) for _, y in t))
            launches.append(pair_raw.spec(oracle, model, first[2], first[0], first[1], FILL, plan_for=common))
            launches.append(pair_raw.spec(oracle, model, second[2], second[0], second[1], "spread", plan_for=common))
    return launches


@pytest.mark.parametrize("case", sorted(STALE))
def test_stale_scratch_of_another_launch(oracle, tmp_path, case):
    """B.  Two launches in one child on the same scratch and the same (G, W) instance and plan.  The first starts on a fill
    pattern; before the second, every wavefront's region that still holds the pattern gets a copy of a region that was
    worked in ("spread", which fails unless there is one), so whichever wavefront takes a batch of the second launch finds
    the slab and the lists of another pair:
      width  W columns per lane, then W - 1 (the slots of the last column keep the first launch's values), and the reverse
      dense  lists that fill, so the dense form leaves posteriors in the slab; then short pairs in the record form; and
             the reverse
      th0    dense from the start (th = 0), then the same sequences at th = 0.01
      empty  records in most lane-steps, then pairs without one entry (CONTRAlign at th = 0.9, ProbCons at th = 1) or with
             next to none (ProbCons at th = 0.9, CONTRAlign at th = 0.6): stale records must not become entries"""
    group, width = STALE[case]
    launches = _launches_b(oracle, case)
    assert len(launches) <= 12
    outs = pair_raw.run(tmp_path, launches, env={"DAFS_HIP_FORCE_GROUP": group, "DAFS_HIP_FORCE_WIDTH": width})
    for first, second in zip(outs[0::2], outs[1::2]):
        a, b = pair_raw.geometry(first), pair_raw.geometry(second)
        assert (a["group"], a["width"]) == (group, width), a
        assert all(a[k] == b[k] for k in ("group", "width", "nwaves", "slab_steps", "scratch_bytes")), (a, b)
        assert 1 <= b["spread_worked"] <= a["nwaves"], b
    _check_all(oracle, outs)


# ---- C: scratch that holds anything ------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [16, 64])
def test_scratch_that_holds_anything(oracle, tmp_path, group):
    """C.  The descending order of test A on scratch filled with 0xFFFFFFFF (a NaN; as a record, an entry mask of all
    ones), +inf, and 1.0 (a posterior above every threshold, a slab sum above `total`).  No address is formed from slab
    or list contents without a bound: pc_exp_n clamps its table piece and pc_log_add_n masks its index, CONTRAlign's
    post is the identity, list reads go through the buffer descriptor under the lane's record count, and s_rowptr[im1]
    is indexed from live records or from the zeros of a read outside the buffer (read from the code, not found by
    running)."""
    _assert_rounds(group)
    outs = pair_raw.run(tmp_path, _launches_a(oracle, ("descending",), fills=(NAN, INF, ONE)), env={"DAFS_HIP_FORCE_GROUP": group})
    assert [o["spec"]["scratch"] for o in outs] == [NAN, INF, ONE] * 2
    _check_all(oracle, outs, nwaves=4)


# ---- D: the pool runs out in the middle of the rounds ------------------------------------------------------------
def test_pool_overflow_in_the_middle_of_the_rounds(oracle, tmp_path):
    """D.  Test A's shuffled order at G = 16 on four wavefronts with half the pool the oracle says is needed: the status
    is DAFS_HIP_EOVERFLOW and the child exits 0; pair_nnz (and the row pointers and sim) are right for every task, because
    the wavefronts go on taking batches after a failed reservation; every pair whose reservation fitted is complete;
    at least one fitted and one did not; everything else, the tails included, holds the canary."""
    order = ORDERS["shuffled"]
    launches = []
    for model in MODELS:
        need = 2 * sum(pair_raw.nnz(oracle, SEQS, order, 0.01, model))
        launches.append(pair_raw.spec(oracle, model, 0.01, SEQS, order, FILL, nwaves=4, pool_cap=need // 2))
    outs = pair_raw.run(tmp_path, launches, env={"DAFS_HIP_FORCE_GROUP": 16})
    for out in outs:
        pool_cap = out["spec"]["pool_cap"]
        assert pair_raw.geometry(out)["nwaves"] == 4
        assert int(out["status"][0]) == -5, out["status"]  # DAFS_HIP_EOVERFLOW
        untouched = np.ones(len(out["col"]), bool)
        rpo = fitted = 0
        for p in range(len(order)):
            rpo += pair_raw.check_heads(oracle, out, p, rpo)
            o, k = int(out["pair_off"][p]), int(out["pair_nnz"][p])
            if o + 2 * k > pool_cap:
                continue
            fitted += 1
            assert pair_raw.check_entries(oracle, out, p) == (o, k)
            assert untouched[o:o + 2 * k].all(), (p, "regions overlap")
            untouched[o:o + 2 * k] = False
        assert 1 <= fitted < len(order), fitted
        assert int(out["pool_top"][0]) == 2 * int(out["pair_nnz"].sum())  # the counter keeps counting: the exact requirement
        pair_raw.check_canaries(out, untouched)


# ---- E: one Context, several calls ---------------------------------------------------------------------------------
def test_one_context_serves_both_models_in_turn(oracle):
    """E.  One Context, so one scratch reservation: ProbCons' two planes per wavefront, then CONTRAlign's five over them,
    and back, with sets of different sizes; each call bit for bit against the oracle."""
    from dafs_amd import capi
    short = [_rand(n, 400 + n) for n in (14, 22, 31, 37)]
    ctx = capi.Context(0)
    try:
        _check_set(oracle, LOW_COMPLEXITY, th=0.002, model=0, ctx=ctx)
        _check_set(oracle, short, th=0.01, model=1, ctx=ctx)
        _check_set(oracle, short, th=0.01, model=0, ctx=ctx)
        _check_set(oracle, LOW_COMPLEXITY, th=0.01, model=1, ctx=ctx)
    finally:
        ctx.close()
