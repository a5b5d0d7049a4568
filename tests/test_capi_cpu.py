"""CPU tests of the C-ABI library: it loads, exports every symbol include/dafs_hip.h declares,
and its host-only helpers (plan, residue codes, model tables) behave.  No compute calls."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_functions():
    src = open(os.path.join(ROOT, "include", "dafs_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dafs_hipk?_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from dafs_amd import capi
    names = declared_functions()
    assert len(names) >= 10
    for n in names:
        assert hasattr(capi.lib, n), "libdafs_hip.so does not export %s" % n


def test_strerror_and_codes():
    from dafs_amd import capi
    assert capi._strerror(0) == b"ok"
    assert b"overflow" in capi._strerror(-5)
    assert b"unknown" in capi._strerror(-99)


def test_pair_ranges_of_the_sharded_phase():
    """dafs_hip_pair_range (what dafs_hip_phase1_sharded shards by) = npairs * k // world: contiguous, covering, in rank
    order -- so the ranks' shards concatenated in rank order are the whole in pair order"""
    from dafs_amd import capi
    assert capi._strerror(-7).startswith(b"dafs_hip: the collective")
    f = capi.lib.dafs_hip_pair_range
    f.restype = None
    f.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    for npairs in (0, 1, 3, 8128, 130816, 10 ** 12 + 7):
        for world in (1, 2, 3, 8, 64):
            want = [npairs * k // world for k in range(world + 1)]
            for r in range(world):
                b, e = C.c_uint64(), C.c_uint64()
                f(npairs, world, r, C.byref(b), C.byref(e))
                assert (b.value, e.value) == (want[r], want[r + 1]), (npairs, world, r)


def test_a_raising_collective_makes_the_callback_fail():
    """an exception of the caller's collective does not cross the library's frames: the dafs_allgather_fn returns non-zero
    (DAFS_HIP_ECOMM in the library) and the exception is kept for Context.phase1_sharded to chain"""
    from dafs_amd import capi
    calls, failures = [], []

    def ok(send, recv, nbytes):
        calls.append((send, recv, nbytes))

    def lost(send, recv, nbytes):
        raise ConnectionError("peer gone")

    assert capi._allgather_callback(ok, failures)(None, 4096, 8192, 24, None) == 0
    assert calls == [(4096, 8192, 24)] and failures == []
    assert capi._allgather_callback(lost, failures)(None, 4096, 8192, 24, None) != 0
    assert len(failures) == 1 and isinstance(failures[0], ConnectionError)


def test_residue_codes():
    from dafs_amd import capi
    assert list(capi.encode("ACGUTNacgutn")) == [0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5]
    assert list(capi.encode("X-~@z")) == [6] * 5


def test_default_model_matches_oracle_tables(oracle):
    from dafs_amd import capi
    m = capi.Pairhmm3Model()
    capi.pairhmm3_default_model(C.byref(m))
    init = np.zeros(3, np.float32); trans = np.zeros(9, np.float32)
    match = np.zeros(256 * 256, np.float32); ins = np.zeros(256, np.float32)
    oracle.lib.orc_probcons_tables.argtypes = [C.c_void_p] * 4
    oracle.lib.orc_probcons_tables(init.ctypes.data, trans.ctypes.data, match.ctypes.data, ins.ctypes.data)
    match = match.reshape(256, 256)
    assert np.array_equal(np.array(list(m.init), np.float32), init)
    t = np.array([list(r) for r in m.trans], np.float32)
    finite = np.isfinite(trans.reshape(3, 3))
    assert np.array_equal(t[finite], trans.reshape(3, 3)[finite])
    for a in range(256):
        ca = capi.residue_code(bytes([a]))
        assert np.float32(m.ins[ca]) == ins[a]
        for b in range(0, 256, 3):
            cb = capi.residue_code(bytes([b]))
            assert np.float32(m.match[ca][cb]) == match[a][b], (a, b)


def test_plan_covers_lengths():
    from dafs_amd import capi
    p = capi.PairhmmPlan()
    for ntasks, l1, l2 in ((1, 1, 1), (45, 82, 82), (496, 80, 80), (8128, 160, 160), (32640, 214, 214), (130816, 428, 428), (3, 2000, 2047)):
        assert capi.pairhmm_plan(ntasks, l1, l2, p) == 0
        assert p.group in (16, 32, 64) and p.group * p.width >= l2 + 1
        assert p.slab_steps == l1 + p.group and p.nwaves % 4 == 0 and p.nwaves <= 8 * 1024
        assert p.scratch_bytes == p.nwaves * p.slab_steps * p.width * 64 * 4 * 2  # DP slab + entry lists
    assert capi.pairhmm_plan(1, 10, 5000, p) == -4
    assert capi.pairhmm_plan(0, 10, 10, p) == -1


def test_pair_launches_refuse_a_wave_count_the_scratch_does_not_cover():
    """dafs_hipk_pairhmm3_launch / dafs_hipk_pairhmm5_launch: nwaves == 0, nwaves not a multiple of 4 and an nwaves whose
    scratch plan.scratch_bytes does not cover are DAFS_HIP_EINVAL before any device call (the arguments hold null
    pointers: nothing here reaches a launch).  The refusal is of the plan alone; a lowered nwaves is not refused for
    these reasons (that it launches is the GPU tests' part)."""
    from dafs_amd import capi
    for plan_fn, launch, Args, planes in ((capi.pairhmm_plan, capi.pairhmm3_launch, capi.Pairhmm3Args, 2),
                                          (capi.pairhmm5_plan, capi.pairhmm5_launch, capi.Pairhmm5Args, 5)):
        a = Args()
        a.ntasks = 65

        def rc(**kw):
            p = capi.PairhmmPlan()
            assert plan_fn(65, 70, 70, p) == 0
            assert p.nwaves >= 8 and p.scratch_bytes == p.nwaves * p.slab_steps * p.width * 64 * 4 * planes
            for k, v in kw.items():
                setattr(p, k, v(p))
            return launch(C.byref(a), C.byref(p), None)

        assert rc(nwaves=lambda p: 0) == -1
        assert rc(nwaves=lambda p: 2) == -1
        assert rc(nwaves=lambda p: p.nwaves + 4) == -1                      # one workgroup more than the scratch holds
        assert rc(scratch_bytes=lambda p: p.scratch_bytes - 1) == -1        # one byte short
        assert rc(scratch_bytes=lambda p: 0) == -1
        assert rc(nwaves=lambda p: 0xFFFFFFFC) == -1                        # no wrap of the product
        assert rc(nwaves=lambda p: 4, scratch_bytes=lambda p: 4 * p.slab_steps * p.width * 64 * 4 * planes - 1) == -1
        assert rc(group=lambda p: 48) == -1                                 # no such instance (as before)
        a.ntasks = 0
        assert rc(nwaves=lambda p: 0) == 0                                  # nothing to do comes first (as before)


def test_dd_node_plan_reproduces_the_recorded_plans(monkeypatch):
    """dafs_hipk_dd_node_plan (the solver's node planner, as nodes_open runs it) against the plans recorded in
    tests/golden/dd_node_plan.npz: (L1, L2) across every threshold of the forms, under each switch setting the GPU tests
    use; and the planner's invariants -- every byte count within the solver's LDS budget, a form only where its score copy
    is carved, the byte counts those of the kernels' LDS layout."""
    from dafs_amd import capi
    g = np.load(os.path.join(ROOT, "tests", "golden", "dd_node_plan.npz"))
    cols = list(g["columns"])
    budget = 156 * 1024
    for k, switch in enumerate(g["switches"]):
        for name in ("WIDE", "SPAN", "NWG", "WG", "SPAN_MW"):
            monkeypatch.delenv("DAFS_HIP_DD_" + name, raising=False)
        if switch:
            monkeypatch.setenv(*switch.split("="))
        rows = g["plans"][g["plans"][:, 0] == k]
        assert len(rows) > 900
        p = capi.DdNodePlan()
        for row in rows:
            L1, L2 = int(row[1]), int(row[2])
            assert capi.dd_node_plan(L1, L2, p) == 0
            got = [getattr(p, c) for c in cols[3:]]
            assert got == [int(v) for v in row[3:]], (switch, L1, L2)
            f, ff = p.lds_flags, p.fold_fast
            assert p.lds <= budget and p.split_lds <= budget
            assert p.lds == 4 * capi.dd_lds_words(L1, L2, f, 0, 0)
            if f & 64:                                         # span form side by side: by-span copies
                assert p.s_xs and p.s_ys and not f & (2 | 4 | 8)
            else:                                              # register forms: sweep-order copies
                assert not (f & (2 | 8)) or p.s_x
                assert not (f & (4 | 8)) or p.s_y
            folders = [4 * capi.dd_lds_words(L1, L2, 0, ff, r + 1) for r in range(2)]
            for r, (sweep, byspan) in enumerate(((p.s_x, p.s_xs), (p.s_y, p.s_ys))):
                form = (ff >> r) & (1 | 4 | 16 | 64)
                assert bin(form).count("1") <= 1
                assert not form & (16 | 64) or byspan
                assert not form & (1 | 4) or sweep
            if p.split_lds:
                assert p.split_lds == max([p.lds] + folders)
            else:
                assert ff == 0


def test_host_build_tree_matches_python_twin():
    """dafs_host_build_tree (host code inside the library, used by the CLI and the pipeline driver) against the
    Python restatement of DAFS::build_tree, on random similarity matrices with ties."""
    from dafs_amd import capi
    from text_ref import build_tree
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 9, 33):
        s = rng.integers(0, 50, size=(n, n)).astype(np.float32) / np.float32(64)
        s = np.maximum(s, s.T)
        np.fill_diagonal(s, 1.0)
        a = capi.build_tree(s)
        b = build_tree(s)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_driver_refuses_option_combinations_it_does_not_implement():
    """pipeline.run: level batches with --bp-update, or a sharded phase 1 with supplied posteriors / the four-way transform,
    raise instead of silently dropping the option (no GPU is touched before the check)"""
    import pytest
    from dafs_amd import pipeline
    with pytest.raises(ValueError):
        pipeline.run(["a", "b"], ["ACGU", "ACGU"], ctx=object(), level_sync=True, bp_update=True)
    for kw in (dict(bp=[]), dict(mp=()), dict(w_pct_f=0.3)):
        with pytest.raises(ValueError):
            pipeline.run(["a", "b"], ["ACGU", "ACGU"], ctx=object(), shard=(None, None), **kw)
