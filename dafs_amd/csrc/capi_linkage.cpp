// dafs_amd/csrc/capi_linkage.cpp -- dafs_hip_linkage_tree (L1) and dafs_hipk_linkage (L0): single, complete and average linkage
// of a similarity matrix on the device (linkage.hip; the contract in DESIGN.md section 21).  The reference has no counterpart.
//
// Host work: the checks, the device memory of one call (the uploaded matrix, the workspace, the three output arrays; none of
// it is kept in the context and none of the context's stores is touched) and the refusal a launch reports in its workspace.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/dafs_hip.h"
#include "ctx.h"
#include "hip_util.h"
#include "last_error.h"
#include "linkage.h"

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

bool known_linkage(int l) { return l == DAFS_LINKAGE_SINGLE || l == DAFS_LINKAGE_COMPLETE || l == DAFS_LINKAGE_AVERAGE; }

// DAFS_HIP_LINKAGE_LDS=0: the per-row state in global memory at every n (tests reach that form at a small n)
bool want_lds(uint32_t n) {
  const char* e = getenv("DAFS_HIP_LINKAGE_LDS");
  if (e && strtol(e, nullptr, 10) == 0 && *e) return false;
  return linkage_fits_lds(n);
}

}  // namespace

extern "C" size_t dafs_hipk_linkage_workspace(uint32_t n) { return n && n <= kLinkageMaxN ? linkage_workspace_bytes(n) : 0; }

extern "C" int dafs_hipk_linkage(int linkage, uint32_t n, const float* d_sim, void* d_workspace, float* d_score, int32_t* d_left,
                                 int32_t* d_right, void* hip_stream) {
  if (!known_linkage(linkage)) return refuse("linkage: unknown linkage rule");
  if (n < 2 || n > kLinkageMaxN) return refuse("linkage: the launch takes 2 to 65536 rows");
  if (!d_sim || !d_workspace || !d_score || !d_left || !d_right) return refuse("linkage: a missing argument");
  if ((uintptr_t)d_workspace & 255) return refuse("linkage: the workspace must be 256-byte aligned");
  return linkage_launch(linkage, n, d_sim, d_workspace, d_score, d_left, d_right, want_lds(n), (hipStream_t)hip_stream);
}

extern "C" int dafs_hip_linkage_tree(dafs_hip_ctx* c, int linkage, uint32_t n, const float* sim, float* score, int32_t* left, int32_t* right) {
  if (!c || !score || !left || !right) return refuse("linkage_tree: a missing argument");
  if (!known_linkage(linkage)) return refuse("linkage_tree: unknown linkage rule");
  if (n == 0 || n > kLinkageMaxN) return refuse("linkage_tree: it takes 1 to 65536 rows");
  if (!sim) {
    if (c->fam.nfam() != 1) return refuse("linkage_tree: the context's own similarity block needs a context of one family");
    if (c->sim.empty()) return refuse("linkage_tree: the context holds no similarity block (dafs_hip_similarity or dafs_hip_align_posteriors first)");
    if (n != c->len.size() || c->sim.size() != (size_t)n * n) return refuse("linkage_tree: n is not the context's number of sequences");
  }
  if (n == 1) {  // the one-leaf tree: no launch
    score[0] = 0.0f;
    left[0] = right[0] = -1;
    return DAFS_HIP_OK;
  }
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const size_t T = 2 * (size_t)n - 1, o_left = (T * 4 + 255) & ~(size_t)255;
  dev_mem in, ws, out;
  if (sim && hip_check(hipMalloc(&in.p, (size_t)n * n * 4))) return DAFS_HIP_ENOMEM;
  if (hip_check(hipMalloc(&ws.p, linkage_workspace_bytes(n))) || hip_check(hipMalloc(&out.p, 3 * o_left))) return DAFS_HIP_ENOMEM;
  hipStream_t st = c->stream;
  float* d_score = (float*)out.p;
  int32_t* d_left = (int32_t*)((uint8_t*)out.p + o_left);
  int32_t* d_right = (int32_t*)((uint8_t*)out.p + 2 * o_left);
  int rc = DAFS_HIP_OK;
  linkage_head head;
  memset(&head, 0, sizeof head);
  if (sim && hip_check(hipMemcpyAsync(in.p, sim, (size_t)n * n * 4, hipMemcpyHostToDevice, st))) rc = DAFS_HIP_ELAUNCH;
  if (!rc) rc = linkage_launch(linkage, n, sim ? (const float*)in.p : c->d_sim.ptr, ws.p, d_score, d_left, d_right, want_lds(n), st);
  if (!rc && hip_check(hipMemcpyAsync(&head, ws.p, sizeof head, hipMemcpyDeviceToHost, st))) rc = DAFS_HIP_ELAUNCH;
  if (hip_check(hipStreamSynchronize(st)) && !rc) rc = DAFS_HIP_ELAUNCH;  // in every case: the copies read and write the caller's memory
  if (rc) return rc;
  if (head.nonfinite) {
    char msg[128];
    snprintf(msg, sizeof msg, "linkage_tree: %u entries above the diagonal are not finite", head.nonfinite);
    return refuse(msg);
  }
  if (head.joins != n - 1) {
    set_last_error("linkage_tree: the joins ended early");
    return DAFS_HIP_ELAUNCH;
  }
  if (hip_check(hipMemcpy(score, d_score, T * 4, hipMemcpyDeviceToHost)) || hip_check(hipMemcpy(left, d_left, T * 4, hipMemcpyDeviceToHost)) ||
      hip_check(hipMemcpy(right, d_right, T * 4, hipMemcpyDeviceToHost)))
    return DAFS_HIP_ELAUNCH;
  return DAFS_HIP_OK;
}
