// dafs_amd/csrc/capi_nj.cpp -- dafs_hip_nj_tree (L1) and dafs_hipk_nj (L0): the neighbour-joining tree of a distance matrix on
// the device (nj.hip; the contract in DESIGN.md section 22), and dafs_host_nj_distances, the distances of an alignment's rows
// from the integer matrices of dafs_hip_alignment_identity.  The reference has no counterpart.
//
// Host work: the checks, the device memory of one call (the uploaded matrix, the workspace, the three output arrays; none of
// it is kept in the context and none of the context's stores is touched) and the refusals a launch reports in its workspace.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/dafs_hip.h"
#include "ctx.h"
#include "hip_util.h"
#include "last_error.h"
#include "nj.h"

using namespace dafs;

namespace {

struct dev_mem {  // the arrays of one call
  void* p = nullptr;
  ~dev_mem() { if (p) (void)hipFree(p); }
};

int refuse(const char* what) {
  set_last_error(what);
  return DAFS_HIP_EINVAL;
}

}  // namespace

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
  const size_t T = 2 * (size_t)n - 1, o_len = (T * 8 + 255) & ~(size_t)255, o_idx = (T * 4 + 255) & ~(size_t)255;
  dev_mem in, ws, out;
  if (hip_check(hipMalloc(&in.p, (size_t)n * n * 8)) || hip_check(hipMalloc(&ws.p, nj_workspace_bytes(n))) ||
      hip_check(hipMalloc(&out.p, o_len + 2 * o_idx)))
    return DAFS_HIP_ENOMEM;
  hipStream_t st = c->stream;
  double* d_length = (double*)out.p;
  int32_t* d_left = (int32_t*)((uint8_t*)out.p + o_len);
  int32_t* d_right = (int32_t*)((uint8_t*)out.p + o_len + o_idx);
  int rc = DAFS_HIP_OK;
  nj_head head;
  memset(&head, 0, sizeof head);
  if (hip_check(hipMemcpyAsync(in.p, dist, (size_t)n * n * 8, hipMemcpyHostToDevice, st))) rc = DAFS_HIP_ELAUNCH;
  if (!rc) rc = nj_launch(n, (const double*)in.p, ws.p, d_left, d_right, d_length, st);
  if (!rc && hip_check(hipMemcpyAsync(&head, ws.p, sizeof head, hipMemcpyDeviceToHost, st))) rc = DAFS_HIP_ELAUNCH;
  if (hip_check(hipStreamSynchronize(st)) && !rc) rc = DAFS_HIP_ELAUNCH;  // in every case: the copies read and write the caller's memory
  if (rc) return rc;
  char msg[160];
  if (head.nonfinite) {
    snprintf(msg, sizeof msg, "nj_tree: %u entries above the diagonal are not finite", head.nonfinite);
    return refuse(msg);
  }
  if (head.fault || head.joins != n - 1) {
    set_last_error("nj_tree: the joins ended early");
    return DAFS_HIP_ELAUNCH;
  }
  if (head.written) {
    snprintf(msg, sizeof msg, "nj_tree: the joins overflowed: %u values written into the distances, the row sums or the lengths are not finite",
             head.written);
    return refuse(msg);
  }
  if (hip_check(hipMemcpy(length, d_length, T * 8, hipMemcpyDeviceToHost)) || hip_check(hipMemcpy(left, d_left, T * 4, hipMemcpyDeviceToHost)) ||
      hip_check(hipMemcpy(right, d_right, T * 4, hipMemcpyDeviceToHost)))
    return DAFS_HIP_ELAUNCH;
  return DAFS_HIP_OK;
}

// DESIGN.md section 22, "Distances from an alignment".  The Jukes-Cantor value is quantised to 2^-20 the way LNQ is in section
// 13, so that an ulp of log() cannot move a bit: it would have to carry -0.75 * log(x) * 2^20 + 0.5 across an integer.
extern "C" int dafs_host_nj_distances(uint32_t n, const uint32_t* ident, const uint32_t* aligned, int model, double* dist) {
  if (!n || !ident || !aligned || !dist) return refuse("nj_distances: a missing argument");
  if (model != DAFS_NJ_P && model != DAFS_NJ_JC) return refuse("nj_distances: unknown model");
  const double kQ = 1048576.0, kCapK = 3.0 * 1048576.0;
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t s = 0; s < n; ++s) {
      const size_t at = (size_t)r * n + s;
      if (r == s) { dist[at] = 0.0; continue; }
      const uint32_t comp = aligned[at];
      if (ident[at] > comp) return refuse("nj_distances: more identical columns than aligned ones");
      const uint32_t mism = comp - ident[at];
      double d;
      if (model == DAFS_NJ_P) {
        d = comp ? (double)mism / (double)comp : 1.0;
      } else if (comp == 0 || 4 * (uint64_t)mism >= 3 * (uint64_t)comp) {
        d = 3.0;
      } else {
        const double x = 1.0 - (4.0 * (double)mism) / (3.0 * (double)comp);
        double k = floor(-0.75 * log(x) * kQ + 0.5);
        if (!(k < kCapK)) k = kCapK;
        d = k / kQ;
      }
      dist[at] = d;
    }
  return DAFS_HIP_OK;
}
