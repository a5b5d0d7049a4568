// dafs_amd/csrc/linkage.h -- launch interface of the linkage kernels (linkage.hip; dafs_hip_linkage_tree and dafs_hipk_linkage
// in capi_linkage.cpp; the contract, to the bit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dafs {

// What the build supports: the working copy is n x n floats with 64-bit offsets, a node index is an int32 (2 n - 1 nodes) and
// a row index a uint32; 65 536 rows are a working copy of 16 GiB.
constexpr uint32_t kLinkageMaxN = 65536;
constexpr uint32_t kLinkageThreads = 1024;    // k_linkage_joins: one workgroup
constexpr uint32_t kLinkageInitThreads = 256; // k_linkage_init: four rows per workgroup
// Per row 16 bytes of state (nearest value, nearest column, size, node); k_linkage_joins keeps them in LDS while they and
// the reduction scratch fit the 160 KiB of one workgroup: n <= 10 224.
constexpr size_t kLinkageLdsBytes = 160 * 1024, kLinkageLdsScratch = 256;
inline bool linkage_fits_lds(uint32_t n) { return (size_t)n * 16 + kLinkageLdsScratch <= kLinkageLdsBytes; }

// The head of the workspace: what a launch leaves for its caller.
struct linkage_head {
  uint32_t nonfinite;          // entries x < y that are not finite; non-zero: no join ran, the join nodes are not written
  uint32_t joins;              // joins made (n - 1 after a complete run)
  unsigned long long rescans;  // rows rescanned by the repair step, over all joins
};

// Workspace layout: head (256 bytes), the working copy S (n x n floats), then per row nn_val, nn_idx, size, node (4 n bytes
// each, the global form of the per-row state; carved in every case so that the size does not depend on the switch).
constexpr size_t kLinkageHeadBytes = 256;
inline size_t linkage_workspace_bytes(uint32_t n) {
  const size_t rows = (((size_t)n * 4 + 255) & ~(size_t)255) * 4;
  return kLinkageHeadBytes + (((size_t)n * n * 4 + 255) & ~(size_t)255) + rows;
}

// k_linkage_init, then k_linkage_joins, on st; no allocation, no wait.  sim: n x n device floats, only x < y read, left as it
// is.  use_lds: the per-row state in LDS (needs linkage_fits_lds(n)).  n >= 2.
int linkage_launch(int linkage, uint32_t n, const float* sim, void* workspace, float* score, int32_t* left, int32_t* right, bool use_lds,
                   hipStream_t st);

}  // namespace dafs
