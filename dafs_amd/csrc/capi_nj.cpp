// dafs_amd/csrc/capi_nj.cpp -- dafs_hip_nj_tree (L1) and dafs_hipk_nj (L0): the neighbour-joining tree of a distance matrix on
// the device (nj.hip; the contract in DESIGN.md section 22).  The reference has no counterpart.  (dafs_host_nj_distances, which
// needs no device, is in host_tree.cpp.)
//
// Host work: the checks, the device memory of one call (the uploaded matrix, the workspace, the three output arrays; none of
// it is kept in the context and none of the context's stores is touched) and the refusals a launch reports in its workspace.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/dafs_hip.h"
#include "call_frame.h"
#include "call_host.h"
#include "nj.h"

using namespace dafs;

// What the head words of one join launch say: the message and the code, or DAFS_HIP_OK.  `who` names the call; in a batch
// `what` names a matrix ("matrix", "replicate") and k is its number.
int dafs::nj_head_verdict(const char* who, const char* what, uint32_t k, uint32_t n, const nj_head& h) {
  const bool early = h.fault || h.joins != n - 1;
  if (!h.nonfinite && !early && !h.written) return DAFS_HIP_OK;
  char where[64], msg[200];
  if (what) snprintf(where, sizeof where, "%s: %s %u", who, what, k);
  else snprintf(where, sizeof where, "%s", who);
  if (h.nonfinite) snprintf(msg, sizeof msg, "%s: %u entries above the diagonal are not finite", where, h.nonfinite);
  else if (early) snprintf(msg, sizeof msg, "%s: the joins ended early", where);
  else snprintf(msg, sizeof msg, "%s: the joins overflowed: %u values written into the distances, the row sums or the lengths are not finite", where, h.written);
  set_last_error(msg);
  return !h.nonfinite && early ? DAFS_HIP_ELAUNCH : DAFS_HIP_EINVAL;
}

extern "C" size_t dafs_hipk_nj_workspace(uint32_t n) { return n && n <= kNjMaxN ? nj_workspace_bytes(n) : 0; }

extern "C" int dafs_hipk_nj(uint32_t n, const double* d_dist, void* d_workspace, int32_t* d_left, int32_t* d_right, double* d_length,
                            void* hip_stream) {
  if (n < 2 || n > kNjMaxN) return refuse("nj: the launch takes 2 to 16384 rows");
  if (!d_dist || !d_workspace || !d_left || !d_right || !d_length) return refuse("nj: a missing argument");
  if ((uintptr_t)d_workspace & 255) return refuse("nj: the workspace must be 256-byte aligned");
  return nj_launch(n, d_dist, d_workspace, d_left, d_right, d_length, (hipStream_t)hip_stream);
}

extern "C" int dafs_hip_nj_tree(dafs_hip_ctx* c, uint32_t n, const double* dist, int32_t* left, int32_t* right, double* length) {
  if (!c || !dist || !left || !right || !length) return refuse("nj_tree: a missing argument");
  if (n == 0 || n > kNjMaxN) return refuse("nj_tree: it takes 1 to 16384 rows");
  for (uint32_t x = 0; x + 1 < n; ++x)
    for (uint32_t y = x + 1; y < n; ++y)
      if (!isfinite(dist[(size_t)x * n + y])) {
        char msg[128];
        snprintf(msg, sizeof msg, "nj_tree: the entry (%u, %u) above the diagonal is not finite", x, y);
        return refuse(msg);
      }
  if (n == 1) {  // the one-leaf tree: no launch
    left[0] = right[0] = -1;
    length[0] = 0.0;
    return DAFS_HIP_OK;
  }
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const size_t T = 2 * (size_t)n - 1;
  carve cv;  // the three output arrays of one allocation
  const size_t o_length = cv.take(T * 8), o_left = cv.take(T * 4), o_right = cv.take(T * 4);
  nj_head head;
  memset(&head, 0, sizeof head);
  call_frame f(c);
  void *in, *ws, *out;
  if (!(in = f.alloc((size_t)n * n * 8)) || !(ws = f.alloc(nj_workspace_bytes(n))) || !(out = f.alloc(cv.bytes()))) return DAFS_HIP_ENOMEM;
  double* d_length = (double*)((uint8_t*)out + o_length);
  int32_t* d_left = (int32_t*)((uint8_t*)out + o_left);
  int32_t* d_right = (int32_t*)((uint8_t*)out + o_right);
  int rc;
  if (f.up(in, dist, (size_t)n * n * 8)) return DAFS_HIP_ELAUNCH;
  if ((rc = nj_launch(n, (const double*)in, ws, d_left, d_right, d_length, f.st))) return rc;
  if (f.down(&head, ws, sizeof head)) return DAFS_HIP_ELAUNCH;
  if ((rc = f.finish())) return rc;
  if ((rc = nj_head_verdict("nj_tree", nullptr, 0, n, head))) return rc;
  if (hip_check(hipMemcpy(length, d_length, T * 8, hipMemcpyDeviceToHost)) || hip_check(hipMemcpy(left, d_left, T * 4, hipMemcpyDeviceToHost)) ||
      hip_check(hipMemcpy(right, d_right, T * 4, hipMemcpyDeviceToHost)))
    return DAFS_HIP_ELAUNCH;
  return DAFS_HIP_OK;
}
