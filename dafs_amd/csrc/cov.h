// dafs_amd/csrc/cov.h -- launch interface of the covariation kernels (cov.hip; dafs_hip_alignment_covariation in capi_cov.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dafs {

// Bit planes of an alignment: word w of base a of column c at planes[(w * 4 + a) * len + c], bit b of it set when row
// w * 32 + b holds base a in column c.  Word-major: the lanes of a wavefront, one column each, read consecutive words.
struct cov_args {
  const uint32_t* planes;
  const int64_t* lnq;                 // LNQ[0..n]
  unsigned long long* col_sum;        // R[len] (two's complement int64)
  const long long* total;             // T (device), written by cov_total
  long long* g;                       // len x len Gq or null (COV_SUMS)
  unsigned long long* best_key;       // per column the order-preserving key of its largest S (COV_BEST writes, COV_ARG reads)
  uint32_t* best;                     // per column the smallest partner that reaches it (COV_ARG)
  const double* cand;                 // ascending candidate scores (COV_NULL)
  unsigned long long* tail;           // [copies][ncand] counters (COV_NULL)
  double ratio;                       // (double)len / (double)(len - 1)
  uint32_t n, len, words, chunk;      // words = ceil(n / 32); chunk = words staged in LDS at a time
  uint32_t ncand, copies;             // copies: a power of two <= 64
};

enum cov_pass { COV_SUMS = 0, COV_BEST, COV_ARG, COV_NULL };

struct cov_ss_args {
  const uint32_t* ss;  // left column -> right column
  double* score;
  uint32_t *rows, *canonical, *types;
};

constexpr uint32_t kCovMaxChunk = 32;  // words of 32 rows per LDS stage: 40 KB

// code: n x len bytes, row-major, 0..4 -> planes (4 * words * len words)
int cov_pack(const uint8_t* code, uint32_t n, uint32_t len, uint32_t* planes, hipStream_t st);
// out = code with every column shuffled on its own: the Fisher-Yates of DESIGN.md section 13 with base = mix(seed + golden * (k + 1))
int cov_shuffle(const uint8_t* code, uint8_t* out, uint32_t n, uint32_t len, uint64_t base, hipStream_t st);
// A tree of 2n-1 nodes on the device in dafs_host_build_tree's layout, checked by the host: the children of join v are
// earlier nodes, parent[v] > v for every node but the root 2n-2 (whose entry is not read).
struct cov_tree {
  const int32_t *left, *right, *parent;
};
constexpr uint32_t kCovTreeThreads = 64;  // k_cov_fitch, k_cov_draw, k_cov_evolve: one wavefront of columns per workgroup
// Fitch sets and states of every column along the tree: chg[(2n-1) * len] gets the change records, node[(2n-1) * len]
// (one byte per node and column) is the kernel's scratch and holds state(root) in its last row afterwards
int cov_fitch(const uint8_t* code, const cov_tree& t, uint32_t n, uint32_t len, uint8_t* node, uint8_t* chg, hipStream_t st);
// out = null alignment by evolution along the tree with base = mix(seed + golden * (k + 1)), in two kernels: every branch's
// drawn change records into its row of node (the last row, the root's, is left as cov_fitch wrote it), then the states
// root-down.  With lds the states of the n-1 joins live in LDS (64 bytes per join: while cov_evolve_fits_lds), else each
// replaces the join's record in node.  n >= 2.
constexpr uint32_t kCovEvolveLdsBytes = 64 * 1024;  // what a workgroup gets without asking for more
inline bool cov_evolve_fits_lds(uint32_t n) { return (size_t)(n - 1) * kCovTreeThreads <= kCovEvolveLdsBytes; }
int cov_evolve(const uint8_t* code, const uint8_t* chg, const cov_tree& t, uint32_t n, uint32_t len, uint64_t base, uint8_t* node,
               uint8_t* out, bool lds, hipStream_t st);
// one pass over every column pair c1 < c2
int cov_pairs(cov_pass pass, const cov_args& a, hipStream_t st);
// *total = sum of col_sum
int cov_total(const unsigned long long* col_sum, uint32_t len, long long* total, hipStream_t st);
// the consensus pairs: S, rows, canonical, types at the left columns, 0 elsewhere
int cov_ss(const cov_args& a, const cov_ss_args& s, hipStream_t st);

}  // namespace dafs
