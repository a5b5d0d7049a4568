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
#include "call_frame.h"
#include "call_host.h"
#include "linkage.h"

using namespace dafs;

namespace {

bool known_linkage(int l) { return l == DAFS_LINKAGE_SINGLE || l == DAFS_LINKAGE_COMPLETE || l == DAFS_LINKAGE_AVERAGE; }

// DAFS_HIP_LINKAGE_LDS=0: the per-row state in global memory at every n (tests reach that form at a small n)
bool want_lds(uint32_t n) { return !env_off("DAFS_HIP_LINKAGE_LDS") && linkage_fits_lds(n); }

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
  const size_t T = 2 * (size_t)n - 1;
  carve cv;  // the three output arrays of one allocation
  const size_t o_score = cv.take(T * 4), o_left = cv.take(T * 4), o_right = cv.take(T * 4);
  linkage_head head;
  memset(&head, 0, sizeof head);
  call_frame f(c);
  void *in = nullptr, *ws, *out;
  if (sim && !(in = f.alloc((size_t)n * n * 4))) return DAFS_HIP_ENOMEM;
  if (!(ws = f.alloc(linkage_workspace_bytes(n))) || !(out = f.alloc(cv.bytes()))) return DAFS_HIP_ENOMEM;
  float* d_score = (float*)((uint8_t*)out + o_score);
  int32_t* d_left = (int32_t*)((uint8_t*)out + o_left);
  int32_t* d_right = (int32_t*)((uint8_t*)out + o_right);
  int rc;
  if (f.up(in, sim, sim ? (size_t)n * n * 4 : 0)) return DAFS_HIP_ELAUNCH;
  if ((rc = linkage_launch(linkage, n, sim ? (const float*)in : c->d_sim.ptr, ws, d_score, d_left, d_right, want_lds(n), f.st))) return rc;
  if (f.down(&head, ws, sizeof head)) return DAFS_HIP_ELAUNCH;
  if ((rc = f.finish())) return rc;
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
