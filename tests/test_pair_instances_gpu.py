"""GPU parity of every compiled instance (G, W) of the pair kernels at its edges (pair_sweeps.h, pairhmm3.hip, pairhmm5.hip;
pair_instances.TABLES is the list).  The planner picks an instance from the lengths of a whole batch, so the other pair
tests reach only the few instances their lengths lead to; here every launch is forced to its instance, and the second
sequence has exactly the length at which the instance's last column, its W-1 form or its emptiest W form is in use.
Further: first sequences at the row-pointer limit of each group size (the launch with the most LDS), and the input that
made the planner return a plan the launch refused.

Everything is bit for bit against the oracle (pair_raw.check for the raw launches, canaries included), so no tolerance is
involved.  What a case needs from its sequences -- entries in the first and the last row and column -- is asserted from
the oracle's answer before the device's answer is looked at."""
import random

import numpy as np
import pytest

import pair_instances as pi
import pair_raw

pytestmark = pytest.mark.gpu

TH = 0.01
SEED = 3
FILL = 0x3F800000  # 1.0 in every word of the first launch's scratch: a posterior above every threshold
MODELS = (0, 1)


def _assert_corners(oracle, model, x, y, rows_only=False):
    rp, col = pair_raw.want(oracle, x, y, TH, model)[:2]
    first_row, last_row, first_col, last_col = pi.corners(rp, col, len(x), len(y))
    assert first_row and last_row, ("the inputs miss an edge row", model, len(x), len(y), first_row, last_row)
    assert rows_only or (first_col and last_col), ("the inputs miss an edge column", model, len(x), len(y), first_col, last_col)


def sweep_launches(oracle, model, group):
    """The launches of one (model, G), every one forced to its (G, W); see test_every_instance_at_its_edges."""
    rng = random.Random(SEED)
    shorts = [pi.random_seq(rng, 5), pi.random_seq(rng, group + 7)]
    launches, scratch = [], FILL
    for w in pi.widths(model, group):
        def add(th, seqs, tasks, window=None):
            nonlocal scratch
            launches.append(pair_raw.spec(oracle, model, th, seqs, tasks, scratch, force=(group, w), window=window))
            scratch = "keep"

        for L2 in pi.edge_lengths(group, w):
            seqs = shorts + [pi.planted(rng, s, L2) for s in shorts]
            for x, y in ((0, 2), (1, 3)):
                _assert_corners(oracle, model, seqs[x], seqs[y])
            add(TH, seqs, [(0, 2), (1, 3)])                    # edges: 5 and G + 7 rows
            if model == 0 and L2 == group * w - 1:
                add(TH, seqs, [(0, 2), (1, 3)], window=group)  # window: sweep 4 staged through the smallest window (k_pairhmm3)
            if L2 % group == group - 1:
                add(0.0, seqs, [(1, 3)])                       # dense: every positive cell an entry, at the exact fits
                assert pair_raw.nnz(oracle, seqs, [(1, 3)], 0.0, model)[0] > pair_raw.nnz(oracle, seqs, [(1, 3)], TH, model)[0]
        if group < 64:                                         # mixed wave: the first batch takes W, the last one W - 1
            ng = 64 // group
            fit, fit1, low = group * w - 1, group * (w - 1) - 1, group * (w - 1)
            first = [fit1, fit, 3, low] if ng == 4 else [3 if w % 2 else low, fit]
            lens = first + [fit1]
            assert len(lens) == ng + 1 and max(first) == fit
            seqs, tasks = list(shorts), []
            for k, L2 in enumerate(lens):
                seqs.append(pi.planted(rng, shorts[k % 2], L2))
                tasks.append((k % 2, len(seqs) - 1))
            add(TH, seqs, tasks)
    return launches


@pytest.mark.parametrize("group", pi.GROUPS)
@pytest.mark.parametrize("model", MODELS)
def test_every_instance_at_its_edges(oracle, tmp_path, model, group):
    """For every W of the group, forced to (G, W), in one child on one scratch (a fill pattern under the first launch, then
    whatever the instance before left: "keep"):
      edges  x of 5 and of G + 7 residues (odd and even step counts, rows fewer than lanes) against y of G W - 1 residues
             (column L2 is the last column of the last lane), of G (W-1) - 1 (the same for the W-1 form) and of G (W-1)
             (the W form with one column in its last slot); y carries copies of x at both ends
      window (ProbCons, whose sweep 4 goes through a staging window in LDS) the exact fit of the W form once more with the
             window forced to G positions, the smallest: many windows per pair, over records of WR = W columns
      dense  the G + 7 rows against both exact fits at th = 0: pair_finish's dense form, taken below th = 0.002; every cell
             with a positive posterior is an entry (the oracle keeps p > th), more than at th = 0.01
      mixed  (G < 64) 64/G + 1 tasks: a first batch with y of G W - 1 residues beside shorter ones (3; G (W-1); at G = 16
             both, and G (W-1) - 1), which takes W for all its groups, and a last task of G (W-1) - 1 alone with inactive
             groups, which takes W - 1.  At G = 32 a batch holds two tasks: 3 beside the fit for odd W, G (W-1) for even."""
    launches = sweep_launches(oracle, model, group)
    outs = pair_raw.run(tmp_path, launches, timeout=600)
    assert len(outs) == len(launches)
    for out in outs:
        L = out["spec"]
        g = pair_raw.geometry(out)
        assert [g["group"], g["width"]] == L["force"], (g, L["force"])
        pair_raw.check(oracle, out, L["seqs"], L["tasks"], L["th"], L["model"])
    assert sorted({tuple(o["spec"]["force"]) for o in outs}) == [(group, w) for w in pi.widths(model, group)]


# ---- long rows ------------------------------------------------------------------------------------------------------
LONG = {16: (2, 29), 32: (2, 23), 64: (1, 50)}  # group: (forced W, L2); the W form at G = 16, the W-1 form at G = 32
# CONTRAlign keeps contra_tables (9824 bytes), 25 match and 5 insert scores in static LDS, 9944 bytes and padding: row
# pointers and statics together reach 64 KiB between the two lengths given per group
LDS_64K = {16: (866, 870), 32: (1731, 1740), 64: (3463, 3480)}


def long_launches(oracle, model):
    rng = random.Random(SEED)
    launches = []
    for group in pi.GROUPS:
        w, L2 = LONG[group]
        assert L2 <= group * w - 1
        y = pi.random_seq(rng, L2)
        for L1 in (LDS_64K[group] if model else ()) + (pi.ROW_LIMIT[group],):
            x = pi.planted(rng, y, L1)  # the roles swapped: the long first sequence carries the short second one
            _assert_corners(oracle, model, x, y, rows_only=True)
            launches.append(pair_raw.spec(oracle, model, TH, [x, y], [(0, 1)], "keep" if launches else FILL, force=(group, w)))
    return launches


@pytest.mark.parametrize("model", MODELS)
def test_rows_at_the_row_pointer_limit(oracle, tmp_path, model):
    """First sequences of 959 (G = 16), 1919 (G = 32) and 3839 (G = 64) residues: the row pointers take the 60 KiB a launch
    allows them, the first and the last row hold entries.  For ProbCons the staging window falls to E = G there and the
    launch opts in to more than 64 KiB of LDS.  For CONTRAlign also the lengths of LDS_64K, on both sides of the point
    where the row pointers and the kernel's static tables together pass 64 KiB."""
    launches = long_launches(oracle, model)
    assert len(launches) == (9 if model else 3)
    if model:
        statics = (9944, 9944 + 64)
        assert all(pi.rowptr_lds(g, a) + statics[1] <= 64 * 1024 < pi.rowptr_lds(g, b) + statics[0] for g, (a, b) in LDS_64K.items())
    outs = pair_raw.run(tmp_path, launches, timeout=300)
    for out in outs:
        L = out["spec"]
        g = pair_raw.geometry(out)
        assert [g["group"], g["width"]] == L["force"] and g["slab_steps"] == len(L["seqs"][0]) + g["group"], g
        pair_raw.check(oracle, out, L["seqs"], L["tasks"], L["th"], L["model"])


# ---- the planner's defect, end to end -------------------------------------------------------------------------------
def test_one_long_sequence_before_many_short_ones(oracle):
    """One 1000-residue sequence first, then 92 of 100: 4278 pairs, 92 of them with 1000 rows.  The planner used to take
    G = 16 for that (cheapest for many tasks with narrow second sequences), whose row pointers the launch refuses beyond
    959 rows: align_posteriors failed with "too long".  Every pair of sequence 0 and every 61st of the others against the
    oracle, both models."""
    from dafs_amd import capi
    rng = random.Random(SEED)
    shorts = [pi.random_seq(rng, 100) for _ in range(92)]
    seqs = [pi.planted(rng, shorts[0], 1000)] + shorts
    n = len(seqs)
    pairs = [(x, y) for x in range(n) for y in range(x + 1, n)]
    assert len(pairs) == 4278
    picked = [p for p, (x, y) in enumerate(pairs) if x == 0] + [p for p, (x, y) in enumerate(pairs) if x > 0][::61]
    assert len(picked) == 92 + 69
    for model in MODELS:
        _assert_corners(oracle, model, seqs[0], seqs[1], rows_only=True)
        ctx = capi.Context(0)
        try:
            ctx.set_sequences(seqs)
            res = ctx.align_posteriors(model, TH)
        finally:
            ctx.close()
        assert len(res) == len(pairs)
        for p in picked:
            x, y = pairs[p]
            assert (res.pair_x[p], res.pair_y[p]) == (x, y)
            rp, col, val, rows, order, sim = pair_raw.want(oracle, seqs[x], seqs[y], TH, model)
            grp, gcol, gval = res.csr(p)
            assert np.array_equal(grp, rp) and np.array_equal(gcol, col), (model, x, y, "rows")
            assert gval.tobytes() == val.tobytes(), (model, x, y, "val")
            trp, tcol, tval = res.csr(p, transposed=True)
            assert np.array_equal(tcol, rows[order]) and tval.tobytes() == val[order].tobytes(), (model, x, y, "transposed")
            assert np.array_equal(trp, np.concatenate([[0], np.cumsum(np.bincount(col, minlength=len(seqs[y])))]).astype(np.uint32))
            assert np.float32(res.sim[p]).tobytes() == np.float32(sim).tobytes(), (model, x, y, "sim")
