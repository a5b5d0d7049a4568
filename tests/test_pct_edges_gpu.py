"""GPU parity of the consistency transforms (k_pct_rows / k_pct_emit, k_pct_bp_rows / k_pct_bp_emit, k_fourway_rows) and of
k_mp_sim on the hand-made stores of pct_cases.py, bit for bit against the oracle's phase 1: rows longer than a 16-lane
group, families beyond one chunk of 16, accumulator rows beyond 64 KiB of LDS up to the refusal, output pools that outgrow
their first guess, and the task table of DAFS_HIP_PCT_YORDER=1.  test_pct_edges_cpu.py asserts that every case reaches the
branch it is for."""
import os

import numpy as np
import pytest

import pct_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture
def ctx():
    from dafs_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def install(ctx, case):
    ctx.set_sequences(case.seqs)
    ctx.set_mp(*case.set_mp_args())
    ctx.set_bp(case.bps)


def fetch(ctx, case, w_a, w_s):
    """the stores the transforms left (the un-relaxed one where a weight is 0), as the oracle's Reference holds them"""
    mp = ctx.mp(1 if w_a != 0 else 0)
    got = {}
    for p, (x, y) in enumerate(case.pairs):
        got[(x, y)] = mp.csr(p, False)
        got[(y, x)] = mp.csr(p, True)
    return got, ctx.bp(1 if w_s != 0 else 0)


def assert_stores(got_mp, got_bp, ref, mp=True, bp=True):
    if mp:
        for key, (rp, col, val) in ref.mp.items():
            grp, gcol, gval = got_mp[key]
            assert np.array_equal(grp, rp), key
            assert np.array_equal(gcol, col), key
            assert gval.tobytes() == val.tobytes(), (key, np.abs(gval - val).max())
    if bp:
        for x, (rp, col, val) in enumerate(ref.bp):
            assert np.array_equal(got_bp[x][0], rp), x
            assert np.array_equal(got_bp[x][1], col), x
            assert got_bp[x][2].tobytes() == val.tobytes(), (x, np.abs(got_bp[x][2] - val).max())


def check_stores(oracle, ctx, case, w_a=0.25, w_s=0.25, w_f=0.0):
    """check_phase1 of test_pct_gpu.py with supplied matching rows: sim(), every pair's forward and transposed rows and every
    sequence's base-pairing rows against the oracle's phase 1, byte for byte.  Returns what the device gave."""
    ref = pc.reference(oracle, case, w_a, w_s, w_f)
    install(ctx, case)
    if w_f != 0:
        ctx.fourway_consistency(w_f)  # replaces the un-relaxed store and the similarity scores
    assert ctx.sim().tobytes() == ref.sim.tobytes()  # k_mp_sim against orc_similarity_score
    ctx.consistency(w_a, w_s)
    got_mp, got_bp = fetch(ctx, case, w_a, w_s)
    assert_stores(got_mp, got_bp, ref)
    return got_mp, got_bp


def same_bytes(a, b):
    (amp, abp), (bmp, bbp) = a, b
    return (all(u.tobytes() == v.tobytes() for k in amp for u, v in zip(amp[k], bmp[k]))
            and all(u.tobytes() == v.tobytes() for s, t in zip(abp, bbp) for u, v in zip(s, t)))


@pytest.mark.parametrize("make,w", [r[1:] for r in pc.RUNS], ids=["%s-%g_%g_%g" % ((r[0],) + r[2]) for r in pc.RUNS])
def test_case(oracle, ctx, make, w):
    check_stores(oracle, ctx, make(), *w)


def test_overflow_retry_then_none(oracle, ctx):
    """the star outgrows both first pool sizes (asserted in test_pct_edges_cpu.py), so the first consistency() of a fresh
    context relaunches both transforms; the second finds the matching pool's hint large enough and relaunches only the
    base-pairing one.  Same bytes both times."""
    case = pc.overflow()
    first = check_stores(oracle, ctx, case)
    ctx.consistency(0.25, 0.25)
    again = fetch(ctx, case, 0.25, 0.25)
    assert_stores(*again, pc.reference(oracle, case))
    assert same_bytes(first, again)


@pytest.mark.parametrize("make", [lambda: pc.chunks(17), pc.lengths], ids=["chunks_17", "lengths"])
def test_yorder(oracle, ctx, make):
    """DAFS_HIP_PCT_YORDER=1: k_pct_rows from pct_task_order's table, whose padding entries these cases need (their task
    count is no multiple of 8), gives the oracle's bytes and the default order's"""
    case = make()
    assert case.row_blocks() % 8 != 0
    plain = check_stores(oracle, ctx, case)
    os.environ["DAFS_HIP_PCT_YORDER"] = "1"
    try:
        ordered = check_stores(oracle, ctx, case)
    finally:
        del os.environ["DAFS_HIP_PCT_YORDER"]
    assert same_bytes(plain, ordered)


def _refused(call):
    from dafs_amd import capi
    with pytest.raises(capi.DafsHipError) as e:
        call()
    assert "code -4" in str(e.value)


def test_match_limit(oracle, ctx):
    """pct_match_launch takes a family of three up to pc.MATCH_TOP residues (test_case[wide_top]) and refuses one more with
    ETOOLONG; the context then works"""
    install(ctx, pc.wide(pc.MATCH_TOP + 1))
    _refused(lambda: ctx.consistency_match(0.25))
    check_stores(oracle, ctx, pc.chunks(16))


def test_bp_limit(oracle, ctx):
    """pct_bp_launch takes pc.BP_TOP residues and refuses one more; the context then works"""
    case = pc.wide(pc.BP_TOP)
    install(ctx, case)
    ctx.consistency_bp(0.25)
    assert_stores(None, ctx.bp(1), pc.reference(oracle, case, 0.0, 0.25), mp=False)
    install(ctx, pc.wide(pc.BP_TOP + 1))
    _refused(lambda: ctx.consistency_bp(0.25))
    check_stores(oracle, ctx, pc.chunks(16))
