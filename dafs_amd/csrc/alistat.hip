// dafs_amd/csrc/alistat.hip -- how similar the rows of an alignment are: pairwise identity, the nearest row, the redundancy
// bit matrix and position-based weights (dafs_hip_alignment_identity, dafs_hip_alignment_weights, capi_alistat.cpp;
// definitions in DESIGN.md section 18).
//
// The rows are held as bit planes, four 64-bit words per row and 64 columns (alistat.h).  The counts of a row pair are
// population counts of a few ANDs of those words, exact integers.  What crosses threads is an integer sum (res), a 64-bit
// maximum (the nearest row) or a whole 32-bit word that one lane writes (the bit matrix), so tiling and chunking change no bit.
//
// k_ali_pairs: the transposed problem of k_cov_pairs (cov.hip).  A workgroup of 16 wavefronts takes a tile of 16 rows r x 64
// rows s; wavefront v owns r = i0 + v, lane l owns s = j0 + l, so a lane owns one row pair and keeps its counters in
// registers.  The plane words of both row blocks are staged in LDS in chunks of `chunk` words: the s words word-major, so
// the 32 lanes of a ds_read_b64 group read 64 consecutive banks, the r words a broadcast.  What k_boot_dist (nj_boot.hip)
// shares with this tile is in ali_tile.h: its shape, its place in LDS, the staging and the counts (ALI_TILE_COUNTS); so are
// the four plane bits of a cell, for k_ali_pack and k_boot_pack.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dafs_hip.h"
#include "ali_tile.h"
#include "alistat.h"
#include "hip_util.h"
#include "stage.h"

namespace dafs {

template <int PASS>
__global__ __launch_bounds__(ALI_TILE_THREADS) void k_ali_pairs(ali_args a, uint32_t i_block0) {
  extern __shared__ uint64_t lds[];  // ali_tile_shape::lds
  __shared__ unsigned long long red_i[ALI_TI], red_j[ALI_TJ];
  const uint32_t i0 = (i_block0 + blockIdx.x) * ALI_TI, j0 = blockIdx.y * ALI_TJ;
  if (PASS != ALI_RED && !ali_tile_upper(i0, j0)) return;  // the whole workgroup leaves
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t r = i0 + wv, s = j0 + lane;
  uint64_t* ly = ali_tile_y(lds);
  uint64_t* lx = ali_tile_x(lds, a.chunk);
  if (PASS == ALI_NEAREST && threadIdx.x < ALI_TJ) red_j[threadIdx.x] = 0;
  uint32_t ident = 0, aligned = 0;
  ALI_TILE_COUNTS(a.planes, a.n, a.words, a.chunk, i0, j0, wv, lane, ly, lx, PASS == ALI_MATRIX, ident, aligned);

  if (PASS == ALI_MATRIX) {  // both triangles from the upper one; the diagonal is the host's (res and base)
    if (r < s && s < a.n) {
      if (a.ident) {
        a.ident[(size_t)r * a.n + s] = ident;
        a.ident[(size_t)s * a.n + r] = ident;
      }
      if (a.aligned) {
        a.aligned[(size_t)r * a.n + s] = aligned;
        a.aligned[(size_t)s * a.n + r] = aligned;
      }
    }
  } else if (PASS == ALI_NEAREST) {
    const bool valid = r < s && s < a.n;
    unsigned long long kr = 0, ks = 0;  // what the pair offers to row r and to row s
    if (valid) {
      const uint32_t rr = a.res[r], rs = a.res[s], den = rr < rs ? rr : rs;
      if (!a.cand || a.cand[s]) kr = ali_best_key(ident, den, s);
      if (!a.cand || a.cand[r]) ks = ali_best_key(ident, den, r);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {  // row r is this wavefront's alone
      const unsigned long long o = __shfl_xor(kr, d, 64);
      kr = o > kr ? o : kr;
    }
    if (lane == 0) red_i[wv] = kr;
    if (ks) atomicMax(&red_j[lane], ks);
    __syncthreads();
    if (threadIdx.x < ALI_TI && red_i[threadIdx.x]) atomicMax(&a.best[i0 + threadIdx.x], red_i[threadIdx.x]);  // a key came from rows below n only
    if (threadIdx.x >= 64 && threadIdx.x < 64 + ALI_TJ) {
      const uint32_t t = threadIdx.x - 64;
      if (red_j[t]) atomicMax(&a.best[j0 + t], red_j[t]);
    }
  } else {  // ALI_RED: every tile; a wavefront holds 64 bits of row r, which lane 0 writes as two whole words
    bool red = false;
    if (r < a.n && s < a.n && r != s) {
      const uint32_t rr = a.res[r], rs = a.res[s];
      red = ali_redundant(ident, rr < rs ? rr : rs, a.threshold);
    }
    const unsigned long long bits = __ballot(red);
    if (lane == 0 && r < a.n) {
      const uint32_t w = j0 / 32;  // j0 is a multiple of 64
      uint32_t* row = a.red + (size_t)r * a.redw;
      if (w < a.redw) row[w] = (uint32_t)bits;
      if (w + 1 < a.redw) row[w + 1] = (uint32_t)(bits >> 32);
    }
  }
}

// one thread per (row, word): the four words of its 64 columns, and the row's counts
__global__ __launch_bounds__(256) void k_ali_pack(const uint8_t* __restrict__ cell, const uint8_t* __restrict__ use, uint32_t n, uint32_t len,
                                                  uint64_t* __restrict__ planes, uint32_t* res, uint32_t* base) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
  if (r >= n) return;
  uint64_t word[4] = {0ull, 0ull, 0ull, 0ull};
  const uint32_t c1 = len - w * 64 < 64 ? len - w * 64 : 64;
  for (uint32_t b = 0; b < c1; ++b) {
    const uint32_t col = w * 64 + b;
    if (use && !use[col]) continue;
    ali_pack_cell(cell[(size_t)r * len + col], b, word);
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) planes[((size_t)w * 4 + p) * n + r] = word[p];
  if (word[ALI_RES]) atomicAdd(&res[r], (uint32_t)__popcll(word[ALI_RES]));
  if (word[ALI_BASE]) atomicAdd(&base[r], (uint32_t)__popcll(word[ALI_BASE]));
}

// one thread per row: the counts of the pair (r, its nearest row)
__global__ __launch_bounds__(256) void k_ali_nearest_counts(ali_args a, uint32_t* __restrict__ nearest_ident, uint32_t* __restrict__ nearest_den) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.n) return;
  const unsigned long long key = a.best[r];
  uint32_t ident = 0, den = 0;
  if (key) {
    const uint32_t s = ali_best_row(key);  // below n: the key was made from a row of the alignment
    for (uint32_t w = 0; w < a.words; ++w) {
      uint64_t x[4], y[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        x[p] = a.planes[((size_t)w * 4 + p) * a.n + r];
        y[p] = a.planes[((size_t)w * 4 + p) * a.n + s];
      }
      ident += ali_ident_word(x, y);
    }
    den = a.res[r] < a.res[s] ? a.res[r] : a.res[s];
  }
  nearest_ident[r] = ident;
  nearest_den[r] = den;
}

// cell (n x len) -> cell_t (len x n), tiles of 32 x 32 through LDS
__global__ __launch_bounds__(1024) void k_ali_transpose(const uint8_t* __restrict__ cell, uint32_t n, uint32_t len, uint8_t* __restrict__ cell_t) {
  __shared__ uint8_t tile[32][33];
  const uint32_t c = blockIdx.x * 32 + threadIdx.x, r = blockIdx.y * 32 + threadIdx.y;
  if (r < n && c < len) tile[threadIdx.y][threadIdx.x] = cell[(size_t)r * len + c];
  __syncthreads();
  const uint32_t r2 = blockIdx.y * 32 + threadIdx.x, c2 = blockIdx.x * 32 + threadIdx.y;
  if (r2 < n && c2 < len) cell_t[(size_t)c2 * n + r2] = tile[threadIdx.x][threadIdx.y];
}

// one thread per column and block of 64 rows: k_c(a) of those rows, added to the column's counters (integers: any order)
constexpr uint32_t kAliCountRows = 64;
__global__ __launch_bounds__(256) void k_ali_count(const uint8_t* __restrict__ cell, uint32_t n, uint32_t len, uint32_t* cnt) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x, r0 = blockIdx.y * kAliCountRows;
  if (c >= len) return;
  const uint32_t r1 = n - r0 < kAliCountRows ? n : r0 + kAliCountRows;
  uint32_t k[5] = {0u, 0u, 0u, 0u, 0u};
  for (uint32_t r = r0; r < r1; ++r) {
    const uint32_t v = cell[(size_t)r * len + c];
#pragma unroll
    for (int q = 0; q < 5; ++q) k[q] += v == (uint32_t)q ? 1u : 0u;
  }
#pragma unroll
  for (int q = 0; q < 5; ++q)
    if (k[q]) atomicAdd(&cnt[(size_t)q * len + c], k[q]);
}

// one thread per column: t_c and the term 1 / (t_c * k_c(a)) that a row with code a adds there
__global__ __launch_bounds__(256) void k_ali_columns(const uint32_t* __restrict__ cnt, uint32_t len, double* __restrict__ inv) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= len) return;
  uint32_t k[5], t = 0;
#pragma unroll
  for (int q = 0; q < 5; ++q) {
    k[q] = cnt[(size_t)q * len + c];
    t += k[q] ? 1u : 0u;
  }
#pragma unroll
  for (int q = 0; q < 5; ++q) inv[(size_t)q * len + c] = k[q] ? 1.0 / (double)(t * k[q]) : 0.0;
}

// one thread per row: its used columns in ascending order, one running sum (the order is the contract)
__global__ __launch_bounds__(256) void k_ali_row_weights(const uint8_t* __restrict__ cell_t, const uint8_t* __restrict__ use,
                                                         const double* __restrict__ inv, uint32_t n, uint32_t len, double* __restrict__ u) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  double v = 0.0;
  uint32_t res = 0;
  for (uint32_t c = 0; c < len; ++c) {
    if (use && !use[c]) continue;
    const uint32_t code = cell_t[(size_t)c * n + r];
    if (code <= 4) {
      v += inv[(size_t)code * len + c];
      ++res;
    }
  }
  u[r] = v / (double)res;  // res > 0: the caller refused a row without residues
}

int ali_pack(const uint8_t* cell, const uint8_t* use, uint32_t n, uint32_t len, uint64_t* planes, uint32_t* res, uint32_t* base, hipStream_t st) {
  const uint32_t words = (len + 63) / 64;  // <= 2^14: fits grid.y
  STAGE_LAUNCH(ST_ALI_PACK, st) hipLaunchKernelGGL(k_ali_pack, dim3((n + 255) / 256, words), dim3(256), 0, st, cell, use, n, len, planes, res, base);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int ali_pairs(ali_pass pass, const ali_args& a, hipStream_t st) {
  if (a.n < 2 || a.n > kAliMaxRows || !a.words || !a.chunk || a.chunk > kAliMaxChunk) return DAFS_HIP_EINVAL;
  if (!a.band_blocks) return DAFS_HIP_EINVAL;
  const ali_tile_shape tile = ali_tile_shape_of(a.n, a.chunk);  // <= 2^16 x 2^14 blocks
  static const int ids[3] = {ST_ALI_MATRIX, ST_ALI_NEAREST, ST_ALI_RED};
  // bands of rows r, so that one launch stays below band_blocks workgroups (2^21 of 1024 threads: under 2^32 work-items)
  const uint32_t band = a.band_blocks / tile.bj ? a.band_blocks / tile.bj : 1;
  for (uint32_t i = 0; i < tile.bi; i += band) {
    const dim3 grid(tile.bi - i < band ? tile.bi - i : band, tile.bj);
    STAGE_LAUNCH(ids[pass], st) switch (pass) {
      case ALI_MATRIX: hipLaunchKernelGGL(k_ali_pairs<ALI_MATRIX>, grid, dim3(ALI_TILE_THREADS), tile.lds, st, a, i); break;
      case ALI_NEAREST: hipLaunchKernelGGL(k_ali_pairs<ALI_NEAREST>, grid, dim3(ALI_TILE_THREADS), tile.lds, st, a, i); break;
      default: hipLaunchKernelGGL(k_ali_pairs<ALI_RED>, grid, dim3(ALI_TILE_THREADS), tile.lds, st, a, i); break;
    }
    if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  }
  return DAFS_HIP_OK;
}

int ali_nearest_counts(const ali_args& a, uint32_t* nearest_ident, uint32_t* nearest_den, hipStream_t st) {
  STAGE_LAUNCH(ST_ALI_NEAREST_COUNTS, st)
  hipLaunchKernelGGL(k_ali_nearest_counts, dim3((a.n + 255) / 256), dim3(256), 0, st, a, nearest_ident, nearest_den);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int ali_transpose(const uint8_t* cell, uint32_t n, uint32_t len, uint8_t* cell_t, hipStream_t st) {
  STAGE_LAUNCH(ST_ALI_TRANSPOSE, st)
  hipLaunchKernelGGL(k_ali_transpose, dim3((len + 31) / 32, (n + 31) / 32), dim3(32, 32), 0, st, cell, n, len, cell_t);  // <= 2^15 x 2^15
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int ali_columns(const uint8_t* cell, uint32_t n, uint32_t len, uint32_t* cnt, double* inv, hipStream_t st) {
  if (hip_check(hipMemsetAsync(cnt, 0, (size_t)5 * len * sizeof(uint32_t), st))) return DAFS_HIP_ELAUNCH;
  STAGE_LAUNCH(ST_ALI_COUNT, st)
  hipLaunchKernelGGL(k_ali_count, dim3((len + 255) / 256, (n + kAliCountRows - 1) / kAliCountRows), dim3(256), 0, st, cell, n, len, cnt);  // grid.y <= 2^14
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  STAGE_LAUNCH(ST_ALI_COLUMNS, st) hipLaunchKernelGGL(k_ali_columns, dim3((len + 255) / 256), dim3(256), 0, st, cnt, len, inv);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int ali_row_weights(const uint8_t* cell_t, const uint8_t* use, const double* inv, uint32_t n, uint32_t len, double* u, hipStream_t st) {
  STAGE_LAUNCH(ST_ALI_ROW_WEIGHTS, st) hipLaunchKernelGGL(k_ali_row_weights, dim3((n + 255) / 256), dim3(256), 0, st, cell_t, use, inv, n, len, u);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

}  // namespace dafs

#undef ALI_TILE_COUNTS
