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
// one pass over every column pair c1 < c2
int cov_pairs(cov_pass pass, const cov_args& a, hipStream_t st);
// *total = sum of col_sum
int cov_total(const unsigned long long* col_sum, uint32_t len, long long* total, hipStream_t st);
// the consensus pairs: S, rows, canonical, types at the left columns, 0 elsewhere
int cov_ss(const cov_args& a, const cov_ss_args& s, hipStream_t st);

}  // namespace dafs
