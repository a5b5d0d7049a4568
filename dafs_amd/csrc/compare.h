// dafs_amd/csrc/compare.h -- launch interface of the alignment comparison kernels (compare.hip; dafs_hip_alignment_compare in
// capi_compare.cpp; definitions in DESIGN.md section 19).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dafs {

// Two alignments of the same n sequences: R (reference, len_r columns) and T (test, len_t columns), as cells in the codes of
// alistat.h.  Row r holds the same residues in both, so residue k of row r has a column in R and a column in T.
//
// Keys.  M[r * len_r + c], the row-major key plane over R's columns: 0 for no residue or an unused column of R; b + 1 for a
// residue placed in the used column b of T; kCmpUnaligned for a residue of a used R column whose T column is unused (it counts
// for refp and never for shared).
constexpr uint32_t kCmpUnaligned = 0xFFFFFFFFu;

struct cmp_args {
  const uint8_t *cell_r, *cell_t;  // n x len_r, n x len_t
  const uint8_t *use_r, *use_t;    // len_r, len_t bytes, or null: every column
  const uint32_t *ss_r, *ss_t;     // the partner column at the left column of a pair, DAFS_HIP_NONE elsewhere; or null
  const uint8_t* pp;               // n x len_t classes 0..10, 255: none; or null
  uint32_t n, len_r, len_t;
  // k_cmp_map
  uint32_t* nres;                  // [n] residues of the row
  uint32_t *col_r, *col_t;         // [n x len_r], [n x len_t]: the column of residue k of row r (the first nres[r] of a row)
  uint32_t* idx_r;                 // [n x len_r]: the residue at column c of R, DAFS_HIP_NONE for a gap
  uint32_t* key;                   // M
  uint32_t* occ_t;                 // [n x len_t]: 1 for a residue in a used column of T, else 0; or null (not wanted)
  // k_cmp_count_cols, k_cmp_count
  uint32_t *k, *m;                 // [len_r], [len_t]
  uint32_t* cnt;                   // [len_r x len_t], dense
  // k_cmp_residue
  unsigned long long* row;         // [3 x n]: shared(r), refp(r), testp(r)
  unsigned long long* bins;        // [3 x 11]: residues, sum of refn, sum of shr per PP class
  // k_cmp_columns
  unsigned long long *colref, *colshared;  // [len_r]
  uint8_t* reproduced;                     // [len_r]
  // k_cmp_ss
  unsigned long long* ss_row;      // [3 x n]: tp(r), nref(r), ntest(r)
};

constexpr uint32_t kCmpMaxRows = 1u << 20, kCmpMaxLen = 1u << 20, kCmpMatrixRows = 16384;
constexpr uint64_t kCmpMaxCells = 1ull << 30;   // len_r * len_t: the dense cnt
constexpr uint32_t kCmpMaxChunk = 128;          // columns per LDS stage: (65 + 16) * 4 * 128 bytes = 41 KB
constexpr uint32_t kCmpBandBlocks = 1u << 21;   // of 1024 threads: a launch stays under 2^32 work-items
constexpr uint32_t kCmpClasses = 11;

int cmp_map(const cmp_args& a, hipStream_t st);
// k, m and cnt (all zeroed here)
int cmp_count(const cmp_args& a, hipStream_t st);
// the row sums and, with a.pp, the class bins (bins zeroed here)
int cmp_residue(const cmp_args& a, hipStream_t st);
int cmp_columns(const cmp_args& a, hipStream_t st);
int cmp_ss(const cmp_args& a, hipStream_t st);
// One pass over the row pairs r < s of a key plane of n x len words; both triangles are written.  present[r * n + s] = columns
// where both keys are non-zero; with shared, shared[r * n + s] = columns where the keys are equal, non-zero and not
// kCmpUnaligned.  chunk: columns per LDS stage; band_blocks: workgroups per launch at most.
int cmp_pairs(const uint32_t* key, uint32_t n, uint32_t len, uint32_t chunk, uint32_t band_blocks, uint32_t* present, uint32_t* shared, hipStream_t st);

}  // namespace dafs
