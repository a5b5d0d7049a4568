// dafs_amd/csrc/nj_boot.h -- launch interface of the bootstrap kernels (nj_boot.hip; dafs_hip_nj_trees, dafs_hipk_nj_batch and
// dafs_hip_alignment_bootstrap in capi_nj_boot.cpp; the contract, to the bit).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nj.h"

namespace dafs {

// k_nj_batch: one workgroup per matrix, R, node and the row of the join in LDS (20 bytes per slot and one chunk of padding:
// 41 KiB at 2 048 slots, below the 64 KiB a kernel gets without asking).
constexpr uint32_t kNjBatchThreads = 1024;
constexpr uint32_t kNjBatchMaxN = 2048;
inline size_t nj_batch_lds_bytes(uint32_t n) {
  const size_t chunks = ((size_t)n + 63) / 64;
  return chunks * 64 * 8 + (chunks + 1) * 64 * 8 + (chunks + 1) * 8 + chunks * 64 * 4;
}

// The workspace of `count` matrices: the heads (one nj_head each), then either every matrix's working copy (the batched form)
// or the workspace of one nj_launch (the looped form); a caller gets room for both.
inline size_t nj_batch_heads_bytes(uint32_t count) { return nj_round((size_t)count * sizeof(nj_head)); }
inline size_t nj_batch_copy_bytes(uint32_t n) { return nj_round((size_t)n * n * 8); }
inline size_t nj_batch_workspace_bytes(uint32_t n, uint32_t count) {
  const size_t batched = n <= kNjBatchMaxN ? (size_t)count * nj_batch_copy_bytes(n) : 0, looped = nj_workspace_bytes(n);
  return nj_batch_heads_bytes(count) + (batched > looped ? batched : looped);
}

// The limit of the batched form: kNjBatchMaxN, or what DAFS_NJ_BATCH_MAX_N (tests only; 0: never) lowers it to.
uint32_t nj_batch_max_n();

// `count` trees on st: dist [count][n][n] device doubles (x < y read, left as they are), outputs [count][2n-1].  n >= 2.
// batched: k_nj_batch in one launch (n <= kNjBatchMaxN); otherwise nj_launch per matrix and a copy of its head.
int nj_batch_launch(uint32_t n, uint32_t count, const double* dist, void* workspace, int32_t* left, int32_t* right, double* length, bool batched,
                    hipStream_t st);

// One entry of the fix-up list: a Jukes-Cantor value so near a quantisation step that the host's log() decides it
struct boot_fix { uint32_t k, r, s, mism, comp; };

struct boot_args {
  const uint8_t* cells;   // the used columns, transposed: cells[u * n + r], u < U
  uint64_t* planes;       // per replicate of the chunk words * 4 * n words in the layout of alistat.h
  double* dist;           // per replicate n x n doubles; the entries r < s are written
  uint32_t* fix_count;    // one counter, zeroed by the caller
  boot_fix* fix;          // fix_cap entries
  uint64_t seed;
  double guard;           // g: |y - nearest integer| <= g goes to the list
  uint32_t n, U, words, chunk;  // words = ceil(U / 64); chunk = words staged in LDS at a time
  uint32_t k0, count;     // the replicates k0 .. k0 + count - 1
  uint32_t fix_cap;
  int model;
};

constexpr uint32_t kBootMaxReplicates = 65536;
constexpr uint32_t kBootChunkReplicates = 32768;  // grid.z stays below 65 536

int boot_pack(const boot_args& a, hipStream_t st);
int boot_dist(const boot_args& a, hipStream_t st);

}  // namespace dafs
