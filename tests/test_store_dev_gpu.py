"""The device store exchange at its edges (capi_dev.cpp, the seven kernels of store_dev.hip, dafs_hip_mp_install,
dafs_hip_consistency_match_range), byte for byte.  The reference of an export is the context's own
host fetch of the same store (Context.mp, Context.bp: no kernel in common with the device path), cut in numpy by
store_dev_cases.py; test_store_dev_cpu.py shows that those cuts and the cases do what they are for.

The entry points have no binding, so store_dev_raw.py calls them on torch's memory, in one child process for this file
(torch has to start the HIP runtime before the library loads): the functions of CHECKS below run there, and every test
here reports how one of them ended."""
import time

import numpy as np
import pytest

import pct_cases as pc
import store_dev_cases as sc
import store_dev_raw as raw

pytestmark = pytest.mark.gpu
W_A = W_S = 0.25


# ---------------------------------------------------------------------------------------------------------------------
# helpers (child side)
# ---------------------------------------------------------------------------------------------------------------------
def context(seqs):
    from dafs_amd import capi
    c = capi.Context(0)
    c.set_sequences(list(seqs))
    return c


def installed(case):
    """a context with the case's sequences, matching store (set_mp) and base-pairing store (set_bp)"""
    c = context(case.seqs)
    c.set_mp(*case.set_mp_args())
    c.set_bp(case.bps)
    return c


def same_pp(a, b):
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes()
               for u, v in ((a.pair_x, b.pair_x), (a.pair_y, b.pair_y), (a.nnz, b.nnz), (a._rowptr, b._rowptr), (a._col, b._col), (a._val, b._val)))


def refused(call):
    """the call raises because its store is invalid"""
    from dafs_amd import capi
    with pytest.raises(capi.DafsHipError) as e:
        call()
    assert "code -1" in str(e.value)


def nothing_written(bufs):
    for name, t in bufs.items():
        if t is not None:
            assert raw.untouched(t, 0, raw.NAN_WORD if name in ("val", "sim") else raw.WORD), name


def check_export(ctx, relaxed, pp, lens, first, count, sim=None, want=None):
    """one export with every capacity exact against slice_mp: nnz, rowptr, col, val, the two counts, sim, and the
    sentinels behind what was written; returns the buffers and the counts"""
    nnz, rp, col, val = want or sc.slice_mp(pp, lens, first, count)
    rc, n_rp, n_ent, b = raw.mp_export_dev(ctx, relaxed, first, count, len(rp), len(col), sim=sim is not None)
    key = (relaxed, first, count)
    assert rc == raw.OK, (key, rc)
    assert (n_rp, n_ent) == (len(rp), len(col)), (key, n_rp, n_ent, len(rp), len(col))
    assert n_ent == 2 * int(nnz.sum())
    for name, ref in (("nnz", nnz), ("rowptr", rp), ("col", col), ("val", val.view(np.uint32))):
        assert raw.host(b[name])[:len(ref)].tobytes() == ref.tobytes(), (key, name)
        assert raw.untouched(b[name], len(ref), raw.NAN_WORD if name == "val" else raw.WORD), (key, name, "sentinel")
    if sim is not None:
        assert raw.host(b["sim"])[:count].tobytes() == sim[first:first + count].tobytes(), (key, "sim")
        assert raw.untouched(b["sim"], count, raw.NAN_WORD), (key, "sim", "sentinel")
    return b, n_rp, n_ent


def check_exports(ctx, relaxed, lens, extra=()):
    """every range of splits() (and of extra) of the store against the host fetch"""
    pp = ctx.mp(relaxed)
    sim = sc.sim_by_pair(ctx.sim(), len(lens)) if relaxed == 0 else None
    todo = sc.ranges(len(pp), extra)
    assert any(c == 0 for _, c in todo) and any(f + c == len(pp) and f > 0 for f, c in todo)
    for first, count in todo:
        check_export(ctx, relaxed, pp, lens, first, count, sim)
    return pp


def gather(ctx, relaxed, pp, lens, split, sim=None):
    """the exports of a split concatenated on the device: (nnz, rowptr, col, val, sim or None, n_entries), every array with
    PAD spare words behind it"""
    import torch
    parts = {k: [] for k in ("nnz", "rowptr", "col", "val", "sim")}
    total = 0
    for first, count in split:
        b, n_rp, n_ent = check_export(ctx, relaxed, pp, lens, first, count, sim)
        for k, n in (("nnz", count), ("rowptr", n_rp), ("col", n_ent), ("val", n_ent), ("sim", count)):
            if b[k] is not None:
                parts[k].append(b[k][:n])
        total += n_ent
    spare = raw.filled(0)
    cat = {k: torch.cat(v + [spare]) if v else None for k, v in parts.items()}
    return cat["nnz"], cat["rowptr"], cat["col"], cat["val"], cat["sim"], total


def finish(ctx, names, seqs):
    """the rest of pipeline.run on a context whose phase 1 is done: guide tree and progressive phase, run's defaults"""
    from dafs_amd import capi, pipeline
    sim = ctx.sim()
    fam = dict(names=list(names), seqs=list(seqs), first=0, sim=sim, tree=capi.build_tree(sim))
    th_s1 = pipeline.decoder_option("Nussinov", 0.2, None, False, None, "pipeline.run")
    return pipeline._phase2_forest(ctx, False, [fam], [time.perf_counter()] * 4, 4.0, 0.5, 600, 0.01, 0.2, th_s1, 0, False, None, True)[0]


# ---------------------------------------------------------------------------------------------------------------------
# export against the host fetch
# ---------------------------------------------------------------------------------------------------------------------
def export_hand(name):
    def check():
        case = sc.HAND[name]()
        ctx = installed(case)
        try:
            pp = check_exports(ctx, 0, case.lens, sc.MANY_EXTRA if name == "many_pairs" else ())
            assert same_pp(pp, sc.case_pp(case))  # the host fetch itself against the transposes worked out in numpy
        finally:
            ctx.close()
    return check


def computed_context(model=0):
    names, seqs = sc.computed()
    ctx = context(seqs)
    ctx.align_posteriors(model, 0.01, fetch=False)
    return ctx, np.array([len(s) for s in seqs], np.uint32)


def export_computed():
    """align_posteriors' store (relaxed 0, pools in processing order) and consistency_match's (relaxed 1)"""
    ctx, lens = computed_context()
    try:
        pp = check_exports(ctx, 0, lens)
        assert int(pp.nnz.max()) > 0
        ctx.consistency_match(W_A)
        check_exports(ctx, 1, lens)
    finally:
        ctx.close()


def two_numberings():
    """an un-relaxed shard numbers its pairs from 0, the relaxed store of consistency_match_range keeps the global index
    and leaves the other pairs empty"""
    names, seqs = sc.computed()
    full, lens = computed_context()
    shard = context(seqs)
    try:
        pp0, sim = full.mp(0), sc.sim_by_pair(full.sim(), len(seqs))
        full.consistency_match(W_A)
        pp1 = full.mp(1)
        world = sc.world_split(len(pp0), 3)
        assert all(c > 0 for _, c in world)
        for b0, cnt in world:
            shard.align_posteriors(0, 0.01, pair_begin=b0, pair_end=b0 + cnt, fetch=False)
            want = sc.slice_mp(pp0, lens, b0, cnt)
            rc, n_rp, n_ent, b = raw.mp_export_dev(shard, 0, 0, cnt, len(want[1]), len(want[2]))
            assert (rc, n_rp, n_ent) == (raw.OK, len(want[1]), len(want[2])), (b0, rc, n_rp, n_ent)
            for name, ref in zip(("nnz", "rowptr", "col", "val", "sim"), want + (sim[b0:b0 + cnt],)):
                assert raw.host(b[name])[:len(ref)].tobytes() == ref.tobytes(), (b0, name)
                assert raw.untouched(b[name], len(ref), raw.NAN_WORD if name in ("val", "sim") else raw.WORD), (b0, name)
            rc, _, _, b = raw.mp_export_dev(shard, 0, 0, cnt + 1, len(want[1]) + 256, len(want[2]) + 256)
            assert rc == raw.EINVAL, "a shard of %d pairs has no pair %d" % (cnt, cnt)
            nothing_written(b)
        for b0, cnt in world:
            assert raw.consistency_match_range(full, W_A, b0, b0 + cnt) == raw.OK
            check_export(full, 1, pp1, lens, b0, cnt)
            for o0, ocnt in world:
                if o0 != b0:  # outside the shard: no entry, every row pointer 0
                    n_rp = len(sc.slice_mp(pp1, lens, o0, ocnt)[1])
                    rc, got_rp, got_ent, b = raw.mp_export_dev(full, 1, o0, ocnt, n_rp, 0, sim=False)
                    assert (rc, got_rp, got_ent) == (raw.OK, n_rp, 0), (b0, o0, rc, got_rp, got_ent)
                    assert not raw.host(b["nnz"])[:ocnt].any() and not raw.host(b["rowptr"])[:n_rp].any()
                    assert raw.untouched(b["nnz"], ocnt) and raw.untouched(b["rowptr"], n_rp)
                    nothing_written({"col": b["col"], "val": b["val"]})
        assert raw.consistency_match_range(full, W_A, 0, 0) == raw.OK  # pair_end 0: all of them
        assert same_pp(full.mp(1), pp1)
    finally:
        full.close()
        shard.close()


# ---------------------------------------------------------------------------------------------------------------------
# install
# ---------------------------------------------------------------------------------------------------------------------
def check_install_dev(src, dst, lens, split, bp_rows):
    """src's stores, exported along a split, gathered and installed in dst: un-relaxed store, similarity matrix, relaxed
    store and what the base-pairing transform makes of them must be src's"""
    pp0, sim = src.mp(0), src.sim()
    nnz, rp, col, val, d_sim, total = gather(src, 0, pp0, lens, split, sc.sim_by_pair(sim, len(lens)))
    assert raw.mp_install_dev(dst, 0, nnz, rp, col, val, d_sim, total) == raw.OK
    assert same_pp(dst.mp(0), pp0) and dst.sim().tobytes() == sim.tobytes()
    refused(lambda: dst.mp(1))  # an un-relaxed install leaves no relaxed store behind
    src.consistency_match(W_A)
    pp1 = src.mp(1)
    nnz, rp, col, val, _, total = gather(src, 1, pp1, lens, split)
    assert raw.mp_install_dev(dst, 1, nnz, rp, col, val, None, total) == raw.OK
    assert same_pp(dst.mp(1), pp1) and same_pp(dst.mp(0), pp0) and dst.sim().tobytes() == sim.tobytes()
    for c in (src, dst):
        c.set_bp(bp_rows)
        c.consistency_bp(W_S)
    assert sc.same_rows(dst.bp(1), src.bp(1))


def install_dev_hand(name):
    def check():
        case = sc.HAND[name]()
        src, dst = installed(case), context(case.seqs)
        try:
            # many_pairs: the splits of one pair per range are a thousand exports each, which export-many_pairs has checked
            for split in [s for s in sc.splits(len(case.pairs)) if len(s) <= 64]:
                check_install_dev(src, dst, case.lens, split, case.bps)
        finally:
            src.close()
            dst.close()
    return check


def install_dev_computed():
    names, seqs = sc.computed()
    src, lens = computed_context()
    dst = context(seqs)
    try:
        src.fold_posteriors(0.01)
        rows = src.bp(0)
        for split in sc.splits(len(seqs) * (len(seqs) - 1) // 2):
            check_install_dev(src, dst, lens, split, rows)
    finally:
        src.close()
        dst.close()


def continue_computed():
    """a context whose matching stores were installed from gathered exports finishes the run as the direct run does"""
    from dafs_amd import pipeline
    names, seqs = sc.computed()
    src, lens = computed_context()
    dst, direct = context(seqs), context(seqs)
    try:
        want = pipeline.run(list(names), list(seqs), ctx=direct)
        src.fold_posteriors(0.01)
        check_install_dev(src, dst, lens, sc.world_split(len(src.mp(0)), 5), src.bp(0))
        got = finish(dst, names, seqs)
        assert got.output == want.output and got.tree_line == want.tree_line
    finally:
        for c in (src, dst, direct):
            c.close()


def continue_two():
    """two sequences: k_sim_matrix writes the second diagonal entry from a thread that has no pair"""
    from dafs_amd import pipeline
    case = sc.two()
    src, dst, direct = installed(case), context(case.seqs), context(case.seqs)
    try:
        want = pipeline.run(case.names, case.seqs, ctx=direct, bp=case.bps, mp=case.set_mp_args())
        check_install_dev(src, dst, case.lens, [(0, 1)], case.bps)
        assert dst.sim().tobytes() == direct.sim().tobytes() and dst.sim()[1, 1] == 1.0 and dst.sim()[0, 0] == 1.0
        assert finish(dst, case.names, case.seqs).output == want.output
    finally:
        for c in (src, dst, direct):
            c.close()


def install_host(name):
    def check():
        case = sc.HAND[name]()
        src, dst = installed(case), context(case.seqs)
        try:
            pp0, sim = src.mp(0), src.sim()
            by_pair = sc.sim_by_pair(sim, case.n)
            assert raw.mp_install(dst, 0, pp0.nnz, pp0._rowptr, pp0._col, pp0._val, by_pair) == raw.OK
            assert same_pp(dst.mp(0), pp0) and dst.sim().tobytes() == sim.tobytes()
            check_exports(dst, 0, case.lens)  # the device export reads a host-installed store as well
            src.consistency_match(W_A)
            pp1 = src.mp(1)
            assert raw.mp_install(dst, 1, pp1.nnz, pp1._rowptr, pp1._col, pp1._val, None) == raw.OK
            assert same_pp(dst.mp(1), pp1) and same_pp(dst.mp(0), pp0)
            for c in (src, dst):
                c.set_bp(case.bps)
                c.consistency_bp(W_S)
            assert sc.same_rows(dst.bp(1), src.bp(1))
            # a pair whose last forward row pointer disagrees with its nnz is refused, and the store is then invalid
            p = next(p for p in range(len(pp0) - 1, -1, -1) if pp0.nnz[p] > 0) if pp0.nnz.any() else len(pp0) - 1
            bad = pp0._rowptr.copy()
            bad[int(pp0._rp_off[p]) + case.lens[int(pp0.pair_x[p])]] += 1
            assert raw.mp_install(dst, 0, pp0.nnz, bad, pp0._col, pp0._val, by_pair) == raw.EINVAL
            refused(lambda: dst.mp(0))
            assert raw.mp_install(dst, 0, pp0.nnz, pp0._rowptr, pp0._col, pp0._val, by_pair) == raw.OK
            assert same_pp(dst.mp(0), pp0) and dst.sim().tobytes() == sim.tobytes()
        finally:
            src.close()
            dst.close()
    return check


# ---------------------------------------------------------------------------------------------------------------------
# base pairing
# ---------------------------------------------------------------------------------------------------------------------
def check_bp(src, dst, lens, rows, reference=None):
    """src holds the rows: its device export is the bp(0) layout; dst takes them back through set_bp_dev in every block
    order.  reference: a context with src's matching store, whose consistency_bp result dst must reproduce."""
    n = len(lens)
    rp, col, val = sc.slice_bp(rows, range(n))
    assert sc.same_rows(src.bp(0), rows)

    def export_is_rows(ctx, what):
        rc, n_rp, n_ent, b = raw.bp_export_dev(ctx, len(rp), len(col))
        assert (rc, n_rp, n_ent) == (raw.OK, len(rp), len(col)), (what, rc, n_rp, n_ent)
        for name, ref in (("rowptr", rp), ("col", col), ("val", val.view(np.uint32))):
            assert raw.host(b[name])[:len(ref)].tobytes() == ref.tobytes(), (what, name)
            assert raw.untouched(b[name], len(ref), raw.NAN_WORD if name == "val" else raw.WORD), (what, name, "sentinel")

    export_is_rows(src, "set_bp")
    if len(col):
        rc, _, _, b = raw.bp_export_dev(src, len(rp), len(col) - 1)
        assert rc == raw.EOVERFLOW
        nothing_written(b)
    if reference is not None:
        reference.consistency_bp(W_S)
        relaxed = reference.bp(1)
    for name, order in sc.block_orders(n).items():
        assert sorted(order) == list(range(n))
        b_rp, b_col, b_val = sc.slice_bp(rows, order)
        assert raw.set_bp_dev(dst, order, raw.device(b_rp), raw.device(b_col), raw.device(b_val), len(b_col)) == raw.OK, name
        assert sc.same_rows(dst.bp(0), rows), name
        export_is_rows(dst, name)  # entries lie in block order now: k_bp_pack's gather is no identity
        if reference is not None:
            dst.consistency_bp(W_S)
            assert sc.same_rows(dst.bp(1), relaxed), name


def bp_hand(name):
    def check():
        case = sc.HAND[name]()
        src, dst = installed(case), context(case.seqs)
        try:
            dst.set_mp(*case.set_mp_args())
            check_bp(src, dst, case.lens, case.bps, reference=src)
        finally:
            src.close()
            dst.close()
    return check


def bp_only(n):
    def check():
        case = sc.bp_only(n)
        src, dst = context(case.seqs), context(case.seqs)
        try:
            src.set_bp(case.bps)
            check_bp(src, dst, case.lens, case.bps)
        finally:
            src.close()
            dst.close()
    return check


def bp_computed():
    names, seqs = sc.computed()
    src, lens = computed_context()
    dst, _ = computed_context()
    try:
        src.fold_posteriors(0.01)
        rows = src.bp(0)
        assert sum(len(r[1]) for r in rows) > 0
        check_bp(src, dst, lens, rows, reference=src)
    finally:
        src.close()
        dst.close()


# ---------------------------------------------------------------------------------------------------------------------
# the error contract
# ---------------------------------------------------------------------------------------------------------------------
def errors_export():
    """a refused export returns its code, writes nothing, and the next correct export is right"""
    case = pc.lengths()
    ctx = installed(case)
    try:
        pp, np_ = ctx.mp(0), len(case.pairs)
        sim = sc.sim_by_pair(ctx.sim(), case.n)
        nnz, rp, col, val = sc.slice_mp(pp, case.lens, 0, np_)
        assert len(col) > 2

        def export_refused(code, relaxed, first, count, cap, with_sim=True):
            rc, _, _, b = raw.mp_export_dev(ctx, relaxed, first, count, len(rp), cap, sim=with_sim, words=np_)
            assert rc == code, (relaxed, first, count, cap, rc)
            nothing_written(b)
            check_export(ctx, 0, pp, case.lens, 3, np_ - 3, sim)

        export_refused(raw.EINVAL, 0, np_ + 1, 0, len(col))              # first > n_tasks
        export_refused(raw.EINVAL, 0, np_ - 8, 9, len(col))              # count > n_tasks - first
        export_refused(raw.EOVERFLOW, 0, 0, np_, len(col) - 1)           # cap_entries one short
        export_refused(raw.EOVERFLOW, 0, 0, np_, len(col) - 1, False)
        part = sc.slice_mp(pp, case.lens, 5, 7)
        export_refused(raw.EOVERFLOW, 0, 5, 7, len(part[2]) - 1)
        export_refused(raw.EINVAL, 1, 0, np_, len(col))                  # no relaxed store yet
        ctx.consistency_match(W_A)
        pp1 = ctx.mp(1)
        cap1 = len(pp1._col)
        export_refused(raw.EINVAL, 1, 0, np_, cap1)                      # sim with relaxed = 1
        check_export(ctx, 1, pp1, case.lens, 0, np_)
        rc, _, _, b = raw.mp_export_dev(ctx, 1, 0, np_, len(rp), cap1 - 1, sim=False)
        assert rc == raw.EOVERFLOW
        nothing_written(b)
        check_export(ctx, 1, pp1, case.lens, 0, np_)
    finally:
        ctx.close()


def errors_install():
    """a refused install returns EINVAL and leaves the store invalid; a correct one then works"""
    case = pc.lengths()
    src, dst = installed(case), context(case.seqs)
    try:
        pp0, sim = src.mp(0), src.sim()
        split = sc.world_split(len(pp0), 3)
        nnz, rp, col, val, d_sim, total = gather(src, 0, pp0, case.lens, split, sc.sim_by_pair(sim, case.n))
        assert raw.mp_install_dev(dst, 1, nnz, rp, col, val, None, total) == raw.EINVAL  # relaxed without an un-relaxed store
        refused(lambda: dst.mp(1))
        refused(lambda: dst.mp(0))
        assert raw.mp_install_dev(dst, 0, nnz, rp, col, val, None, total) == raw.EINVAL  # un-relaxed without sim
        for off in (2, -2):  # the gathered arrays have raw.PAD spare words behind them
            assert raw.mp_install_dev(dst, 0, nnz, rp, col, val, d_sim, total + off) == raw.EINVAL, off
            refused(lambda: dst.mp(0))
            refused(dst.sim)
        assert raw.mp_install_dev(dst, 0, nnz, rp, col, val, d_sim, total) == raw.OK
        assert same_pp(dst.mp(0), pp0) and dst.sim().tobytes() == sim.tobytes()
        src.consistency_match(W_A)
        pp1 = src.mp(1)
        nnz, rp, col, val, _, total = gather(src, 1, pp1, case.lens, split)
        assert raw.mp_install_dev(dst, 1, nnz, rp, col, val, None, total - 2) == raw.EINVAL
        refused(lambda: dst.mp(1))
        assert same_pp(dst.mp(0), pp0)  # the un-relaxed store is not the one that was refused
        assert raw.mp_install_dev(dst, 1, nnz, rp, col, val, None, total) == raw.OK
        assert same_pp(dst.mp(1), pp1)
    finally:
        src.close()
        dst.close()


def errors_set_bp():
    case = pc.lengths()
    dst = context(case.seqs)
    try:
        n = case.n
        order = sc.block_orders(n)["world_3"]
        rp, col, val = sc.slice_bp(case.bps, order)
        spare = np.zeros(raw.PAD, np.uint32)
        d = [raw.device(np.concatenate([a.view(np.uint32), spare])) for a in (rp, col, val)]
        for off in (1, -1):
            assert raw.set_bp_dev(dst, order, d[0], d[1], d[2], len(col) + off) == raw.EINVAL, off
            refused(lambda: dst.bp(0))
        assert raw.set_bp_dev(dst, order, d[0], d[1], d[2], len(col)) == raw.OK
        assert sc.same_rows(dst.bp(0), case.bps)
        twice = list(order)
        twice[-1] = twice[0]  # a repeated sequence
        assert raw.set_bp_dev(dst, twice, d[0], d[1], d[2], len(col)) == raw.EINVAL
        beyond = list(order)
        beyond[2] = n  # no such sequence
        assert raw.set_bp_dev(dst, beyond, d[0], d[1], d[2], len(col)) == raw.EINVAL
        assert raw.set_bp_dev(dst, order[:-1], d[0], d[1], d[2], len(col)) == raw.EINVAL  # nblocks != N
        assert raw.set_bp_dev(dst, order, d[0], d[1], d[2], len(col), nblocks=n + 1) == raw.EINVAL
        assert raw.set_bp_dev(dst, order, d[0], d[1], d[2], len(col)) == raw.OK
        assert sc.same_rows(dst.bp(0), case.bps)
    finally:
        dst.close()


CHECKS = {}
for _name in sc.HAND:
    CHECKS["export-%s" % _name] = export_hand(_name)
CHECKS["export-computed"] = export_computed
CHECKS["two_numberings"] = two_numberings
for _name in sc.HAND:
    CHECKS["install_dev-%s" % _name] = install_dev_hand(_name)
CHECKS["install_dev-computed"] = install_dev_computed
CHECKS["continue-computed"] = continue_computed
CHECKS["continue-two"] = continue_two
for _name in ("lengths", "empty", "chunks_17", "two"):
    CHECKS["install_host-%s" % _name] = install_host(_name)
for _name in ("lengths", "empty", "chunks_17", "two"):
    CHECKS["bp-%s" % _name] = bp_hand(_name)
for _n in sc.BP_ONLY:
    CHECKS["bp-only_%d" % _n] = bp_only(_n)
CHECKS["bp-computed"] = bp_computed
CHECKS["errors-export"] = errors_export
CHECKS["errors-install"] = errors_install
CHECKS["errors-set_bp"] = errors_set_bp


@pytest.fixture(scope="module")
def outcome(tmp_path_factory):
    return raw.run_checks("test_store_dev_gpu", tmp_path_factory.mktemp("store_dev"))


@pytest.mark.parametrize("name", list(CHECKS))
def test_store_dev(outcome, name):
    assert outcome.get(name, "not run: " + outcome["__child__"]) == "ok"
