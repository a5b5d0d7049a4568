"""CPU tests of the CONTRAfold launch plan (dafs_hipk_contrafold_plan in contrafold.hip, the only place contrafold_launch
takes its decisions from): properties every plan must have for the kernel's carve of the dynamic LDS to stay inside the
launch, at every length the launch accepts and at three sizes of the kernel's static LDS.  The formula is not restated;
what is restated is the kernel's own carve (k_contrafold) and the limits of the hardware.  No kernel is launched."""
import pytest

from dafs_amd import capi

KB = 1024
TOTAL = 160 * KB - 512      # LDS of a CU that one workgroup may hold, static and dynamic together
DYN_BUDGET = 100 * KB       # integer tables and ring
RING = 33                   # CF_RING: spans of FC / FCo the ring holds
LONGEST_LIST = 496          # the most single-branch terms one cell can have (spans up to CF_MAX_SINGLE = 30 inside it)
TYPICAL = 80                # terms per row a buffer must hold before the pool is cut in two
STATICS = (12 * KB, 20 * KB, 28 * KB)
L_MAX = 2131
ETOOLONG = -4
SWITCHES = ("DAFS_HIP_CF_NORING", "DAFS_HIP_CF_NOPOOL", "DAFS_HIP_CF_NOOVERLAP", "DAFS_HIP_CF_CELL_WAVES", "DAFS_HIP_CF_THREADS")
FIELDS = ("threads", "cell_waves", "use_ring", "pool_floats", "pool_bufs", "lds")


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def plan(max_len, static):
    p = capi.ContrafoldPlan()
    rc = capi.contrafold_plan(max_len, static, p)
    assert rc == 0, (max_len, static, rc)
    assert p.static_lds == static
    return p


def fields(p):
    return tuple(getattr(p, f) for f in FIELDS)


def ints_bytes(L):
    return 4 * 12 * (L + 2)   # CF_INTS: s, map, cum, off (L + 2 each), plist and pcnt (4 (L + 2) each)


def ring_bytes(L):
    return 4 * RING * (L + 1)


def carve_end(L, p):
    """where k_contrafold's carve of the dynamic LDS ends for a sequence of L residues launched under plan p: the integer
    tables, the ring of L if the plan has one, and with a pool the list heads and counts of two buffers (4 (L + 1) ints), the
    two bump counters and the pool.  Without a pool the kernel touches nothing behind the ring."""
    end = ints_bytes(L) + (ring_bytes(L) if p.use_ring else 0)
    if p.pool_floats:
        end += 4 * (4 * (L + 1) + 2) + 4 * p.pool_floats
    return end


def check_plan(L, static, p):
    at = (L, static, fields(p))
    assert static + p.lds <= TOTAL, at
    assert p.use_ring in (0, 1) and p.pool_bufs in (1, 2), at
    assert p.threads % 64 == 0 and 64 <= p.threads <= 1024 and 1 <= p.cell_waves <= 16, at
    if p.use_ring:
        assert ints_bytes(L) + ring_bytes(L) <= DYN_BUDGET, at
    if p.pool_floats:
        assert p.pool_floats // p.pool_bufs >= LONGEST_LIST, at
    else:
        assert p.pool_bufs == 1, at
    if p.pool_bufs == 2:
        assert p.pool_floats // 2 >= TYPICAL * (L + 1), at
    assert carve_end(L, p) <= p.lds, at   # the longest member itself


@pytest.mark.parametrize("static", STATICS)
def test_every_plan_fits_and_the_forms_change_once(static):
    """Every accepted length: the plan fits the CU beside the static tables, the ring fits its budget, a pool buffer holds
    one cell's longest list and, of two, the typical demand of a span; and as the length grows the ring, the second buffer
    and the pool are each given up once and never taken back."""
    prev = None
    changes = {"use_ring": 0, "pool_bufs": 0, "pool_on": 0}
    for L in range(1, L_MAX + 1):
        p = plan(L, static)
        check_plan(L, static, p)
        assert (p.threads, p.cell_waves) == (1024, 8), L
        cur = {"use_ring": p.use_ring, "pool_bufs": p.pool_bufs, "pool_on": int(p.pool_floats > 0)}
        if prev is not None:
            for k in cur:
                assert cur[k] <= prev[k], (k, L, static)   # only ever given up
                changes[k] += cur[k] != prev[k]
        prev = cur
    assert all(v <= 1 for v in changes.values()), changes
    # the ring and the second buffer are given up inside the accepted range at every static size tried; the pool only where
    # the static tables are large enough to crowd it out
    assert changes["use_ring"] == 1 and changes["pool_bufs"] == 1, (static, changes)


def _switch_points(static):
    """(last length with two buffers, last with the ring, last with a pool)"""
    ps = [plan(L, static) for L in range(1, L_MAX + 1)]
    return (max(L for L, p in enumerate(ps, 1) if p.pool_bufs == 2), max(L for L, p in enumerate(ps, 1) if p.use_ring),
            max(L for L, p in enumerate(ps, 1) if p.pool_floats))


def test_switch_points_are_where_the_documents_put_them():
    """DESIGN.md and the comments of contrafold.hip name these lengths; a change of the plan must change them too"""
    assert _switch_points(28 * KB) == (160, 259, 2040)
    assert _switch_points(20 * KB)[:2] == (169, 275)
    assert _switch_points(12 * KB)[:2] == (179, 291)


@pytest.mark.parametrize("static", STATICS)
def test_shorter_members_carve_inside_the_launch(static):
    """A batch is planned for its longest member and every shorter one carves the same launch by its own length.  For the
    lengths on both sides of each switch point, one inside each form and the longest accepted: every L' <= max_len ends
    inside `lds`, and its pool does not start before its own tables end (the carve is increasing in L')."""
    la, lb, lp = _switch_points(static)
    for max_len in sorted({1, 33, la, la + 1, (la + lb) // 2, lb, lb + 1, 600, lp, min(lp + 1, L_MAX), L_MAX}):
        p = plan(max_len, static)
        ends = [carve_end(L, p) for L in range(1, max_len + 1)]
        assert max(ends) <= p.lds, (max_len, static)
        assert ends == sorted(ends), (max_len, static)


def test_the_limit():
    p = capi.ContrafoldPlan()
    for static in STATICS:
        assert capi.contrafold_plan(L_MAX, static, p) == 0
        assert capi.contrafold_plan(L_MAX + 1, static, p) == ETOOLONG
        assert capi.contrafold_plan(4000, static, p) == ETOOLONG
    assert capi.contrafold_plan(100, 28 * KB, None) != 0


LENGTHS = (1, 2, 33, 100, 160, 161, 181, 259, 260, 400, 1024, 2040, 2041, L_MAX)


@pytest.mark.parametrize("static", STATICS)
def test_switches_give_the_form_they_name(monkeypatch, static):
    """Each DAFS_HIP_CF_* switch alone: the named form at every length, the other properties intact, and the fields the
    switch does not name as without it (NORING frees room, so the pool may only grow)."""
    base = {L: plan(L, static) for L in LENGTHS}

    def under(name, value):
        monkeypatch.setenv(name, value)
        out = {L: plan(L, static) for L in LENGTHS}
        monkeypatch.delenv(name)
        for L, p in out.items():
            check_plan(L, static, p)
        return out

    for L, p in under("DAFS_HIP_CF_NORING", "1").items():
        b = base[L]
        assert p.use_ring == 0 and p.pool_floats >= b.pool_floats and p.pool_bufs >= b.pool_bufs, L
        assert (p.threads, p.cell_waves) == (b.threads, b.cell_waves)
        if not b.use_ring:
            assert fields(p) == fields(b), L
    for L, p in under("DAFS_HIP_CF_NOPOOL", "1").items():
        assert p.pool_floats == 0 and p.pool_bufs == 1, L
        assert p.lds == ints_bytes(L) + (ring_bytes(L) if p.use_ring else 0), L
        assert p.use_ring == int(ints_bytes(L) + ring_bytes(L) <= DYN_BUDGET), L   # nothing competes with the ring
    for L, p in under("DAFS_HIP_CF_NOOVERLAP", "1").items():
        b = base[L]
        assert p.pool_bufs == 1, L
        assert (p.threads, p.cell_waves, p.use_ring, p.pool_floats, p.lds) == (b.threads, b.cell_waves, b.use_ring, b.pool_floats, b.lds), L
    for v in (1, 3, 8, 16):
        for L, p in under("DAFS_HIP_CF_CELL_WAVES", str(v)).items():
            assert p.cell_waves == v and fields(p)[:1] + fields(p)[2:] == fields(base[L])[:1] + fields(base[L])[2:], (v, L)
    for v in (64, 128, 256, 960, 1024):
        for L, p in under("DAFS_HIP_CF_THREADS", str(v)).items():
            assert p.threads == v and fields(p)[1:] == fields(base[L])[1:], (v, L)
    # values out of range are ignored
    for name, bad in (("DAFS_HIP_CF_CELL_WAVES", ("0", "17", "-1", "x", "")), ("DAFS_HIP_CF_THREADS", ("0", "32", "100", "1088", "2048", "-64", "x", ""))):
        for v in bad:
            for L, p in under(name, v).items():
                assert fields(p) == fields(base[L]), (name, v, L)
