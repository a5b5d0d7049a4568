// dafs_amd/csrc/nj.h -- launch interface of the neighbour-joining kernels (nj.hip; dafs_hip_nj_tree and dafs_hipk_nj in
// capi_nj.cpp; the contract, to the bit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dafs {

// What the build supports: the working copy is n x n doubles; 16 384 rows are a working copy of 2 GiB.
constexpr uint32_t kNjMaxN = 16384;
constexpr uint32_t kNjRowThreads = 256;      // k_nj_init, k_nj_pick: one wavefront per row, four rows per workgroup
constexpr uint32_t kNjUpdateThreads = 1024;  // k_nj_update: one workgroup

// The head of the workspace: what a launch leaves for its caller.
struct nj_head {
  uint32_t nonfinite;  // entries x < y that are not finite; non-zero: no join ran, the join nodes are not written
  uint32_t written;    // non-finite values written into D, R or length, at the start and over all joins; non-zero: refuse
  uint32_t joins;      // joins made (n - 1 after a complete run)
  uint32_t fault;      // a pick outside the active slots (cannot happen; the join is then skipped and the count stays short)
};

// Workspace layout: head (256 bytes), the working copy D (n x n doubles), then per row R and the row's best Q (8 n bytes each),
// node and the row's best column (4 n bytes each), every block rounded up to 256 bytes.
constexpr size_t kNjHeadBytes = 256;
inline size_t nj_round(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t nj_workspace_bytes(uint32_t n) {
  return kNjHeadBytes + nj_round((size_t)n * n * 8) + 2 * nj_round((size_t)n * 8) + 2 * nj_round((size_t)n * 4);
}

// k_nj_update keeps the row it has just written in LDS for the running sum of R[a]: per chunk of 64 slots 64 doubles and one
// mask of the slots that take part, and one chunk of padding: 130 KiB at n = 16 384, of the 160 KiB of one workgroup.
inline size_t nj_update_lds_bytes(uint32_t n) { return ((size_t)(n + 63) / 64 + 1) * (64 * 8 + 8); }

// k_nj_init, k_nj_rowsum, then n - 1 times k_nj_pick and k_nj_update, on st; no allocation, no wait.  dist: n x n device doubles,
// only x < y read, left as it is.  n >= 2.
int nj_launch(uint32_t n, const double* dist, void* workspace, int32_t* left, int32_t* right, double* length, hipStream_t st);

// What the head of a finished launch says, for every caller (capi_nj.cpp): DAFS_HIP_OK, or the code with the message set.
int nj_head_verdict(const char* who, const char* what, uint32_t k, uint32_t n, const nj_head& h);

}  // namespace dafs
