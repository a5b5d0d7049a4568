"""Raw calls of the entry points that have no Python binding, for tests: dafs_hip_mp_export_dev, dafs_hip_mp_install_dev,
dafs_hip_bp_export_dev and dafs_hip_set_bp_dev (capi_dev.cpp) on torch's device memory, dafs_hip_mp_install (capi_align.cpp)
on numpy arrays and dafs_hip_consistency_match_range (capi_pct.cpp).  A helper module, not a conftest.

Every output buffer is a torch int32 tensor of its capacity plus PAD words, filled with a sentinel before the call (WORD
for integers, NAN_WORD, a quiet NaN, where floats land), so a test can see every word the library wrote and that none
lies behind what it reported.  The library works on its own stream and waits for it before an export returns; the callers
here wait for torch's before they hand a buffer over.

torch and the library share one HIP runtime only when torch starts it first, so whatever uses these callers runs in a
child process: run_checks(module) starts this file as a program, which loads torch, then the library, then the test module,
runs the functions the module lists in CHECKS one after another and writes down how each ended.  After a HIP error or a
failed barrier of a world it starts nothing further."""
import ctypes as C
import json
import os
import subprocess
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
WORD, NAN_WORD = 0xDEADBEEF, 0x7FC0BEEF
OK, EINVAL, EOVERFLOW, ECOMM = 0, -1, -5, -7
_u64p = C.POINTER(C.c_uint64)
_SIGNATURES = {
    "dafs_hip_mp_export_dev": [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64] + [C.c_void_p] * 5 + [C.c_uint64, _u64p, _u64p],
    "dafs_hip_mp_install_dev": [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_uint64],
    "dafs_hip_bp_export_dev": [C.c_void_p] + [C.c_void_p] * 3 + [C.c_uint64, _u64p, _u64p],
    "dafs_hip_set_bp_dev": [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4 + [C.c_uint64],
    "dafs_hip_mp_install": [C.c_void_p, C.c_int] + [C.c_void_p] * 5,
    "dafs_hip_consistency_match_range": [C.c_void_p, C.c_float, C.c_uint64, C.c_uint64],
}


def _fn(name):
    from dafs_amd import capi
    f = getattr(capi.lib, name)
    f.restype, f.argtypes = C.c_int, _SIGNATURES[name]
    return f


def _i32(word):
    return word - (1 << 32) if word >= (1 << 31) else word


def filled(words, pattern=WORD):
    """a device buffer of `words` words and PAD more, every word the pattern"""
    import torch
    return torch.full((int(words) + PAD,), _i32(pattern), dtype=torch.int32, device="cuda:0")


def device(a):
    """a numpy array of 4-byte items as a device buffer (int32 words), one word at least so that it has an address"""
    import torch
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    t = torch.zeros(max(a.size, 1), dtype=torch.int32, device="cuda:0")
    if a.size:
        t[:a.size] = torch.from_numpy(a.reshape(-1).view(np.int32).copy())
    return t


def host(t, dtype=np.uint32):
    return t.cpu().numpy().view(dtype)


def untouched(t, written, pattern=WORD):
    """every word of the buffer from `written` on still holds the pattern"""
    h = host(t)
    return len(h) >= written + PAD and bool(np.all(h[written:] == pattern))


def _ptr(t):
    return None if t is None else t.data_ptr()


def mp_export_dev(ctx, relaxed, first, count, cap_rowptr, cap_entries, sim=True, words=None):
    """dafs_hip_mp_export_dev into fresh buffers: returns (rc, n_rowptr, n_entries, {"nnz", "rowptr", "col", "val", "sim"}).
    nnz and sim have room for `words` pairs (count where it is None), rowptr for cap_rowptr words, col and val for
    cap_entries, each with PAD words behind; sim False passes no sim buffer."""
    import torch
    words = count if words is None else words
    b = {"nnz": filled(words), "rowptr": filled(cap_rowptr), "col": filled(cap_entries), "val": filled(cap_entries, NAN_WORD),
         "sim": filled(words, NAN_WORD) if sim else None}
    n_rp, n_ent = C.c_uint64(WORD), C.c_uint64(WORD)
    torch.cuda.synchronize()
    rc = _fn("dafs_hip_mp_export_dev")(ctx._h, relaxed, first, count, _ptr(b["nnz"]), _ptr(b["rowptr"]), _ptr(b["col"]), _ptr(b["val"]),
                                       _ptr(b["sim"]), cap_entries, C.byref(n_rp), C.byref(n_ent))
    torch.cuda.synchronize()
    return rc, n_rp.value, n_ent.value, b


def mp_install_dev(ctx, relaxed, nnz, rowptr, col, val, sim, n_entries):
    """dafs_hip_mp_install_dev from device buffers (sim None for a relaxed store); returns rc"""
    import torch
    torch.cuda.synchronize()
    rc = _fn("dafs_hip_mp_install_dev")(ctx._h, relaxed, _ptr(nnz), _ptr(rowptr), _ptr(col), _ptr(val), _ptr(sim), n_entries)
    torch.cuda.synchronize()
    return rc


def bp_export_dev(ctx, cap_rowptr, cap_entries):
    """dafs_hip_bp_export_dev into fresh buffers: returns (rc, n_rowptr, n_entries, {"rowptr", "col", "val"})"""
    import torch
    b = {"rowptr": filled(cap_rowptr), "col": filled(cap_entries), "val": filled(cap_entries, NAN_WORD)}
    n_rp, n_ent = C.c_uint64(WORD), C.c_uint64(WORD)
    torch.cuda.synchronize()
    rc = _fn("dafs_hip_bp_export_dev")(ctx._h, _ptr(b["rowptr"]), _ptr(b["col"]), _ptr(b["val"]), cap_entries, C.byref(n_rp), C.byref(n_ent))
    torch.cuda.synchronize()
    return rc, n_rp.value, n_ent.value, b


def set_bp_dev(ctx, seq_of_block, rowptr, col, val, n_entries, nblocks=None):
    """dafs_hip_set_bp_dev: seq_of_block is a host array, the rest device buffers; returns rc"""
    import torch
    order = np.ascontiguousarray(seq_of_block, np.uint32)
    torch.cuda.synchronize()
    rc = _fn("dafs_hip_set_bp_dev")(ctx._h, len(order) if nblocks is None else nblocks, order.ctypes.data, _ptr(rowptr), _ptr(col), _ptr(val), n_entries)
    torch.cuda.synchronize()
    return rc


def mp_install(ctx, relaxed, nnz, rowptr, col, val, sim):
    """dafs_hip_mp_install, the host twin, from numpy arrays (sim None for a relaxed store); returns rc"""
    nnz = np.ascontiguousarray(nnz, np.uint32); rowptr = np.ascontiguousarray(rowptr, np.uint32)
    col = np.ascontiguousarray(col, np.uint32); val = np.ascontiguousarray(val, np.float32)
    sim = None if sim is None else np.ascontiguousarray(sim, np.float32)
    return _fn("dafs_hip_mp_install")(ctx._h, relaxed, nnz.ctypes.data, rowptr.ctypes.data, col.ctypes.data if len(col) else None,
                                      val.ctypes.data if len(val) else None, None if sim is None else sim.ctypes.data)


def consistency_match_range(ctx, w_pct_a, pair_begin, pair_end):
    return _fn("dafs_hip_consistency_match_range")(ctx._h, w_pct_a, pair_begin, pair_end)


# ---------------------------------------------------------------------------------------------------------------------
# the child
# ---------------------------------------------------------------------------------------------------------------------
class Stop(Exception):
    """a check raises it when nothing further may start on the device"""


def run_checks(module, tmp_path, timeout=600):
    """Runs the CHECKS of the test module `module` in one child; returns {check: "ok" or what went wrong}.  A check the
    child did not reach is reported as such."""
    out = str(tmp_path / ("%s.json" % module))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), module, out], cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    res = {}
    if os.path.exists(out):
        with open(out) as f:
            res = json.load(f)
    res["__child__"] = "ok" if r.returncode == 0 else "exit status %d\n%s" % (r.returncode, r.stderr[-4000:])
    return res


def _child(module, out_path):
    import torch  # before the library: both then share torch's HIP runtime, as in bench.py
    torch.cuda.init()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from dafs_amd import capi  # noqa: F401
    import store_dev_raw as me  # the copy the test modules import: its Stop is the one they raise
    mod = __import__(module)
    res, stopped = {}, None
    for name, fn in mod.CHECKS.items():
        if stopped:
            res[name] = "not run: %s" % stopped
            continue
        t0 = time.perf_counter()
        try:
            fn()
            torch.cuda.synchronize()
            res[name] = "ok"
        except BaseException as e:  # noqa: BLE001
            res[name] = traceback.format_exc()
            if isinstance(e, (me.Stop, KeyboardInterrupt)) or (isinstance(e, RuntimeError) and any(w in str(e) for w in ("HIP", "hipError", "illegal"))):
                stopped = "%s ended with %r" % (name, e)
        print("%-70s %6.2f s  %s" % (name, time.perf_counter() - t0, res[name].strip().splitlines()[-1]), flush=True)
        with open(out_path, "w") as f:
            json.dump(res, f)
    with open(out_path, "w") as f:
        json.dump(res, f)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
