// dafs_amd/csrc/ali_tile.h -- device code over the bit planes of alistat.h that more than one file runs: a cell's four plane
// bits (k_ali_pack, k_boot_pack) and the pair-count tile of 16 rows r x 64 rows s (k_ali_pairs, k_boot_dist): its shape, its
// place in LDS, the identity count of a word, and the staging and counting of all chunks (ALI_TILE_COUNTS).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "alistat.h"

namespace dafs {

// The tile: 16 wavefronts; wavefront v owns r = i0 + v, lane l owns s = j0 + l.
constexpr uint32_t ALI_TI = 16, ALI_TJ = 64;
constexpr uint32_t ALI_TILE_THREADS = ALI_TI * 64;  // 1024: a wavefront per row r

// What a launcher needs of the tiling of n rows: the blocks of r and of s, and the LDS of one workgroup
struct ali_tile_shape {
  uint32_t bi, bj;
  size_t lds;  // y[chunk][4][ALI_TJ], then x[chunk][4][ALI_TI]
};
inline ali_tile_shape ali_tile_shape_of(uint32_t n, uint32_t chunk) {
  return {(n + ALI_TI - 1) / ALI_TI, (n + ALI_TJ - 1) / ALI_TJ, (size_t)chunk * 4 * (ALI_TI + ALI_TJ) * sizeof(uint64_t)};
}

// whether the tile at (i0, j0) holds a pair r < s
__device__ __forceinline__ bool ali_tile_upper(uint32_t i0, uint32_t j0) { return j0 + ALI_TJ - 1 > i0; }

// cell code v in column bit b of the four words of its row
__device__ __forceinline__ void ali_pack_cell(uint64_t v, uint32_t b, uint64_t* word) {
  word[ALI_LO] |= (v & 1) << b;
  word[ALI_HI] |= ((v >> 1) & 1) << b;
  word[ALI_BASE] |= (uint64_t)(v <= 3 ? 1 : 0) << b;
  word[ALI_RES] |= (uint64_t)(v <= 4 ? 1 : 0) << b;
}

// identical bases in the 64 columns of one word of two rows
__device__ __forceinline__ uint32_t ali_ident_word(const uint64_t* x, const uint64_t* y) {
  return (uint32_t)__popcll(~(x[ALI_LO] ^ y[ALI_LO]) & ~(x[ALI_HI] ^ y[ALI_HI]) & x[ALI_BASE] & y[ALI_BASE]);
}

// The tile in LDS (ali_tile_shape::lds bytes): the words of a chunk of the s block, y[chunk][4][ALI_TJ], word-major, so the 32
// lanes of a ds_read_b64 group read 64 consecutive banks; then those of the r block, x[chunk][4][ALI_TI], read as a broadcast.
__device__ __forceinline__ uint64_t* ali_tile_y(uint64_t* lds) { return lds; }
__device__ __forceinline__ uint64_t* ali_tile_x(uint64_t* lds, uint32_t chunk) { return lds + (size_t)chunk * 4 * ALI_TJ; }

// The counts of the row pair of wavefront WV and lane LANE over all WORDS words, by a whole workgroup of ALI_TILE_THREADS
// threads (the __launch_bounds__ and the launch of both kernels): per chunk of CHUNK words the plane words of the s block
// (from row J0) and of the r block (from row I0) go into LY and LX between two __syncthreads(), rows from N on as 0; then
// every staged word adds to IDENT and, where ALIGNED (a constant), to ALIGNED_SUM.  A statement macro and not a function on
// purpose: hipcc optimises a function with loops on its own before it inlines it, which gave k_ali_pairs other code in every
// form tried (the note of the refactoring); the text below is compiled in the kernel itself.  The
// arguments are plain variables or members, read more than once; the macro's own names begin with at_, which no argument may.
// Each of the two files that use it ends with #undef ALI_TILE_COUNTS.
#define ALI_TILE_COUNTS(PLANES, N, WORDS, CHUNK, I0, J0, WV, LANE, LY, LX, ALIGNED, IDENT, ALIGNED_SUM)                    \
  do {                                                                                                                     \
    for (uint32_t at_w0 = 0; at_w0 < (WORDS); at_w0 += (CHUNK)) {                                                          \
      const uint32_t at_wc = (WORDS) - at_w0 < (CHUNK) ? (WORDS) - at_w0 : (CHUNK);                                        \
      __syncthreads();                                                                                                     \
      for (uint32_t at_t = threadIdx.x; at_t < at_wc * 4 * ALI_TJ; at_t += ALI_TILE_THREADS) {                             \
        const uint32_t at_row = (J0) + (at_t & (ALI_TJ - 1)), at_pl = at_t / ALI_TJ; /* at_pl = w * 4 + plane */           \
        (LY)[at_t] = at_row < (N) ? (PLANES)[((size_t)at_w0 * 4 + at_pl) * (N) + at_row] : 0ull;                           \
      }                                                                                                                    \
      for (uint32_t at_t = threadIdx.x; at_t < at_wc * 4 * ALI_TI; at_t += ALI_TILE_THREADS) {                             \
        const uint32_t at_row = (I0) + (at_t & (ALI_TI - 1)), at_pl = at_t / ALI_TI;                                       \
        (LX)[at_t] = at_row < (N) ? (PLANES)[((size_t)at_w0 * 4 + at_pl) * (N) + at_row] : 0ull;                           \
      }                                                                                                                    \
      __syncthreads();                                                                                                     \
      for (uint32_t at_w = 0; at_w < at_wc; ++at_w) {                                                                      \
        uint64_t at_x[4], at_y[4];                                                                                         \
        _Pragma("unroll") for (int at_p = 0; at_p < 4; ++at_p) {                                                           \
          at_x[at_p] = (LX)[(at_w * 4 + at_p) * ALI_TI + (WV)];                                                            \
          at_y[at_p] = (LY)[(at_w * 4 + at_p) * ALI_TJ + (LANE)];                                                          \
        }                                                                                                                  \
        IDENT += ali_ident_word(at_x, at_y);                                                                               \
        if (ALIGNED) ALIGNED_SUM += (uint32_t)__popcll(at_x[ALI_RES] & at_y[ALI_RES]);                                     \
      }                                                                                                                    \
    }                                                                                                                      \
  } while (0)

}  // namespace dafs
