// dafs_amd/csrc/alistat.h -- launch interface of the alignment statistics kernels (alistat.hip; dafs_hip_alignment_identity and
// dafs_hip_alignment_weights in capi_alistat.cpp; definitions in DESIGN.md section 18).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dafs {

// Cell codes: A 0, C 1, G 2, U/T 3, any other letter 4 (a residue that matches nothing), a gap 5.
//
// Bit planes of an alignment's rows: word w (columns w * 64 .. w * 64 + 63) of plane p of row r at planes[(w * 4 + p) * n + r],
// bit b of it set for column w * 64 + b; a bit is set in used columns only.  Word-major: the lanes of a wavefront, one row
// each, read consecutive words.
enum ali_plane { ALI_LO = 0, ALI_HI, ALI_BASE, ALI_RES };  // code bit 0, code bit 1, code <= 3, code <= 4

struct ali_args {
  const uint64_t* planes;
  const uint32_t* res;           // res(r)
  const uint8_t* cand;           // rows that may be somebody's nearest, or null: every row (ALI_NEAREST)
  uint32_t* ident;               // n x n or null (ALI_MATRIX)
  uint32_t* aligned;             // n x n or null (ALI_MATRIX)
  unsigned long long* best;      // per row the largest ali_best_key of its candidates, 0: none (ALI_NEAREST)
  uint32_t* red;                 // n x redw bit matrix (ALI_RED)
  double threshold;              // t of ALI_RED
  uint32_t n, words, chunk, redw;  // words = ceil(len / 64); chunk = words staged in LDS at a time; redw = ceil(n / 32)
  uint32_t band_blocks;            // workgroups per launch at most: the passes go over bands of rows r
};

enum ali_pass { ALI_MATRIX = 0, ALI_NEAREST, ALI_RED };

constexpr uint32_t kAliMaxChunk = 16;  // words of 64 columns per LDS stage: 40 KB
constexpr uint32_t kAliBandBlocks = 1u << 21;  // of 1024 threads: a launch stays under 2^32 work-items
constexpr uint32_t kAliMaxRows = 1u << 20, kAliMaxLen = 1u << 20;

// red(r, s): one multiplication and one comparison in double (no contraction: every unit is built with -ffp-contract=off)
__host__ __device__ inline bool ali_redundant(uint32_t ident, uint32_t den, double t) { return (double)ident >= t * (double)den; }

// The nearest row as one 64-bit maximum.  q = floor(ident * 2^41 / den) keeps the order of the fractions exactly for
// den <= 2^20: two different fractions with denominators up to 2^20 differ by 2^-40 at least, so their q differ by 2 at
// least, and equal fractions have equal q.  q + 1 <= 2^41 + 1 fills bits 20..61 (0 is left for "no candidate"); bits 0..19
// hold 2^20 - 1 - s, so among equal fractions the smallest s is the largest key.
__host__ __device__ inline unsigned long long ali_best_key(uint32_t ident, uint32_t den, uint32_t s) {
  return ((((unsigned long long)ident << 41) / den + 1) << 20) | (unsigned long long)(kAliMaxRows - 1 - s);
}
__host__ __device__ inline uint32_t ali_best_row(unsigned long long key) { return kAliMaxRows - 1 - (uint32_t)(key & (kAliMaxRows - 1)); }

// cell: n x len codes, row-major; use: len bytes or null (all columns) -> planes (4 * words * n words), res[n] and base[n]
// (cells of the row with code <= 4 and <= 3 in used columns; both zeroed by the caller)
int ali_pack(const uint8_t* cell, const uint8_t* use, uint32_t n, uint32_t len, uint64_t* planes, uint32_t* res, uint32_t* base, hipStream_t st);
// one pass over the row pairs: r < s for ALI_MATRIX and ALI_NEAREST, every r != s for ALI_RED
int ali_pairs(ali_pass pass, const ali_args& a, hipStream_t st);
// ident(r, s) and den(r, s) of s = the row of best[r]; 0 where best[r] is 0
int ali_nearest_counts(const ali_args& a, uint32_t* nearest_ident, uint32_t* nearest_den, hipStream_t st);

// weights: cell_t = the transpose of cell (len x n)
int ali_transpose(const uint8_t* cell, uint32_t n, uint32_t len, uint8_t* cell_t, hipStream_t st);
// cnt[a * len + c] = k_c(a) and inv[a * len + c] = 1.0 / (double)(t_c * k_c(a)) for a = 0..4 (0.0 where k_c(a) = 0)
int ali_columns(const uint8_t* cell, uint32_t n, uint32_t len, uint32_t* cnt, double* inv, hipStream_t st);
// u[r] = (sum over used columns c ascending with code <= 4 of inv[code][c]) / (double)(number of such columns)
int ali_row_weights(const uint8_t* cell_t, const uint8_t* use, const double* inv, uint32_t n, uint32_t len, double* u, hipStream_t st);

}  // namespace dafs
