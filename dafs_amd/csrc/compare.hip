// dafs_amd/csrc/compare.hip -- how far two alignments of the same sequences agree: shared residue pairs (SPS, PPV), reproduced
// columns (TC), the per-pair tables, accuracy per PP class and shared base pairs (dafs_hip_alignment_compare,
// capi_compare.cpp; definitions in DESIGN.md section 19).
//
// Everything is an integer count, so what crosses threads is an integer sum: tiling, chunking and the order of the atomics
// change no bit.  All but the pair tables is O(n * len): k_cmp_map gives every residue its two columns and the key plane M,
// k_cmp_count_cols / k_cmp_count fill k_c, m_d and the dense cnt(c, d), k_cmp_residue gathers them per residue, k_cmp_columns
// per column of R, k_cmp_ss counts base pairs per row.
//
// k_cmp_pairs is k_ali_pairs (alistat.hip) over 32-bit keys instead of bit planes: a workgroup of 16 wavefronts takes a tile
// of 16 rows r x 64 rows s; wavefront v owns r = i0 + v, lane l owns s = j0 + l, so a lane owns one row pair and keeps its
// counters in registers.  The keys of both row blocks are staged in LDS in chunks of `chunk` columns: the s block
// column-major with a stride of 65 words, so the lanes of a read and the lanes of a staging write hit distinct banks, the r
// block row-major, read as a broadcast.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dafs_hip.h"
#include "compare.h"
#include "hip_util.h"
#include "stage.h"

namespace dafs {

constexpr uint32_t TI = 16, TJ = 64, TJP = TJ + 1;

// one wavefront per row: T first (the columns of its residues), then R (columns, residue indices and keys)
__global__ __launch_bounds__(256) void k_cmp_map(cmp_args a) {
  const uint32_t lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const bool live = r < a.n;
  const unsigned long long below = (1ull << lane) - 1;
  if (live) {
    const uint8_t* cell = a.cell_t + (size_t)r * a.len_t;
    uint32_t* col = a.col_t + (size_t)r * a.len_t;
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < a.len_t; c0 += 64) {  // the trip count is the wavefront's
      const uint32_t c = c0 + lane;
      const bool res = c < a.len_t && cell[c] <= 4;
      const unsigned long long bal = __ballot(res);
      if (res) col[base + (uint32_t)__popcll(bal & below)] = c;  // below nres(r) <= len_t
      if (a.occ_t && c < a.len_t) a.occ_t[(size_t)r * a.len_t + c] = res && (!a.use_t || a.use_t[c]) ? 1u : 0u;
      base += (uint32_t)__popcll(bal);
    }
  }
  __syncthreads();  // col_t of this row is read below by other lanes of the wavefront
  if (live) {
    const uint8_t* cell = a.cell_r + (size_t)r * a.len_r;
    const uint32_t* col_t = a.col_t + (size_t)r * a.len_t;
    uint32_t base = 0;
    for (uint32_t c0 = 0; c0 < a.len_r; c0 += 64) {
      const uint32_t c = c0 + lane;
      const bool res = c < a.len_r && cell[c] <= 4;
      const unsigned long long bal = __ballot(res);
      const uint32_t k = base + (uint32_t)__popcll(bal & below);
      uint32_t key = 0;
      if (res) {  // the caller checked that both rows hold the same residues: k < nres(r) <= len_t
        a.col_r[(size_t)r * a.len_r + k] = c;
        if (!a.use_r || a.use_r[c]) {
          const uint32_t b = col_t[k];
          key = !a.use_t || a.use_t[b] ? b + 1 : kCmpUnaligned;
        }
      }
      if (c < a.len_r) {
        a.idx_r[(size_t)r * a.len_r + c] = res ? k : DAFS_HIP_NONE;
        a.key[(size_t)r * a.len_r + c] = key;
      }
      base += (uint32_t)__popcll(bal);
    }
    if (lane == 0) a.nres[r] = base;
  }
}

// one thread per column and block of 64 rows: the residues of those rows in the column, added to its counter if it is used
constexpr uint32_t kCmpCountRows = 64;
__global__ __launch_bounds__(256) void k_cmp_count_cols(const uint8_t* __restrict__ cell, const uint8_t* __restrict__ use, uint32_t n, uint32_t len,
                                                        uint32_t* out) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x, r0 = blockIdx.y * kCmpCountRows;
  if (c >= len || (use && !use[c])) return;
  const uint32_t r1 = n - r0 < kCmpCountRows ? n : r0 + kCmpCountRows;
  uint32_t k = 0;
  for (uint32_t r = r0; r < r1; ++r) k += cell[(size_t)r * len + c] <= 4 ? 1u : 0u;
  if (k) atomicAdd(&out[c], k);
}

// one workgroup per row: cnt(a, b) += 1 for every residue with both keys
__global__ __launch_bounds__(256) void k_cmp_count(cmp_args a) {
  const uint32_t r = blockIdx.x;
  const uint32_t* key = a.key + (size_t)r * a.len_r;
  for (uint32_t c = threadIdx.x; c < a.len_r; c += 256) {
    const uint32_t v = key[c];
    if (v && v != kCmpUnaligned) atomicAdd(&a.cnt[(size_t)c * a.len_t + (v - 1)], 1u);  // v - 1 < len_t: a column of T
  }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// one workgroup per row: refn, testn and shr of its residues, summed; the residues' PP classes
__global__ __launch_bounds__(256) void k_cmp_residue(cmp_args a) {
  __shared__ unsigned long long sum[3], bins[3 * kCmpClasses];
  const uint32_t r = blockIdx.x;
  if (threadIdx.x < 3) sum[threadIdx.x] = 0;
  if (threadIdx.x < 3 * kCmpClasses) bins[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t nres = a.nres[r];
  unsigned long long shared = 0, refp = 0, testp = 0;
  for (uint32_t k = threadIdx.x; k < nres; k += 256) {
    const uint32_t cr = a.col_r[(size_t)r * a.len_r + k], ct = a.col_t[(size_t)r * a.len_t + k];
    const bool ua = !a.use_r || a.use_r[cr], ub = !a.use_t || a.use_t[ct];
    const uint32_t refn = ua ? a.k[cr] - 1 : 0, testn = ub ? a.m[ct] - 1 : 0;  // the residue itself is counted: both >= 1
    const uint32_t shr = ua && ub ? a.cnt[(size_t)cr * a.len_t + ct] - 1 : 0;
    shared += shr;
    refp += refn;
    testp += testn;
    if (a.pp) {
      const uint32_t q = a.pp[(size_t)r * a.len_t + ct];
      if (q < kCmpClasses) {
        atomicAdd(&bins[q], 1ull);
        if (refn) atomicAdd(&bins[kCmpClasses + q], (unsigned long long)refn);
        if (shr) atomicAdd(&bins[2 * kCmpClasses + q], (unsigned long long)shr);
      }
    }
  }
  shared = wave_sum(shared);
  refp = wave_sum(refp);
  testp = wave_sum(testp);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&sum[0], shared);
    atomicAdd(&sum[1], refp);
    atomicAdd(&sum[2], testp);
  }
  __syncthreads();
  if (threadIdx.x < 3) a.row[(size_t)threadIdx.x * a.n + r] = sum[threadIdx.x];
  if (a.pp && threadIdx.x < 3 * kCmpClasses && bins[threadIdx.x]) atomicAdd(&a.bins[threadIdx.x], bins[threadIdx.x]);
}

// one wavefront per column c of R: its row of cnt
__global__ __launch_bounds__(256) void k_cmp_columns(cmp_args a) {
  const uint32_t lane = threadIdx.x & 63, c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= a.len_r) return;  // whole wavefronts; no barrier below
  const uint32_t kc = a.k[c];
  const uint32_t* cnt = a.cnt + (size_t)c * a.len_t;
  unsigned long long sh = 0;
  bool rep = false;
  for (uint32_t d = lane; d < a.len_t; d += 64) {
    const unsigned long long v = cnt[d];
    if (v) sh += v * (v - 1) / 2;
    rep = rep || (kc >= 2 && v == kc && a.m[d] == kc);
  }
  sh = wave_sum(sh);
  const bool any = __ballot(rep) != 0;
  if (lane == 0) {
    a.colref[c] = (unsigned long long)kc * (kc ? kc - 1 : 0) / 2;
    a.colshared[c] = sh;
    a.reproduced[c] = any ? 1 : 0;
  }
}

// one thread per row: the base pairs of ss_r and of ss_t that the row holds both ends of, and those in both
__global__ __launch_bounds__(256) void k_cmp_ss(cmp_args a) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= a.n) return;
  const uint32_t* idx = a.idx_r + (size_t)r * a.len_r;
  const uint32_t* col_t = a.col_t + (size_t)r * a.len_t;
  const uint8_t* cell_t = a.cell_t + (size_t)r * a.len_t;
  unsigned long long tp = 0, nref = 0, ntest = 0;
  for (uint32_t c = 0; c < a.len_r; ++c) {
    const uint32_t d = a.ss_r[c];
    if (d == DAFS_HIP_NONE) continue;  // d < len_r: checked by the caller
    const uint32_t k = idx[c], l = idx[d];
    if (k == DAFS_HIP_NONE || l == DAFS_HIP_NONE) continue;
    ++nref;
    if (a.ss_t[col_t[k]] == col_t[l]) ++tp;  // the left column in T is residue k's: k < l in both
  }
  for (uint32_t c = 0; c < a.len_t; ++c) {
    const uint32_t d = a.ss_t[c];
    if (d != DAFS_HIP_NONE && cell_t[c] <= 4 && cell_t[d] <= 4) ++ntest;
  }
  a.ss_row[r] = tp;
  a.ss_row[(size_t)a.n + r] = nref;
  a.ss_row[(size_t)2 * a.n + r] = ntest;
}

template <bool SHARED>
__global__ __launch_bounds__(1024) void k_cmp_pairs(const uint32_t* __restrict__ key, uint32_t n, uint32_t len, uint32_t chunk, uint32_t* present,
                                                    uint32_t* shared, uint32_t i_block0) {
  extern __shared__ uint32_t lds[];  // y[chunk][TJP], then x[TI][chunk]
  const uint32_t i0 = (i_block0 + blockIdx.x) * TI, j0 = blockIdx.y * TJ;
  if (j0 + TJ - 1 <= i0) return;  // no pair r < s in this tile (the whole workgroup leaves)
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t r = i0 + wv, s = j0 + lane;
  uint32_t* ly = lds;
  uint32_t* lx = lds + (size_t)chunk * TJP;
  uint32_t np = 0, ns = 0;
  for (uint32_t c0 = 0; c0 < len; c0 += chunk) {
    const uint32_t wc = len - c0 < chunk ? len - c0 : chunk;
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < wc * TJ; t += 1024) {  // consecutive threads: consecutive columns of one row
      const uint32_t row = t / wc, c = t - row * wc;
      ly[c * TJP + row] = j0 + row < n ? key[(size_t)(j0 + row) * len + c0 + c] : 0u;
    }
    for (uint32_t t = threadIdx.x; t < wc * TI; t += 1024) {
      const uint32_t row = t / wc, c = t - row * wc;
      lx[row * chunk + c] = i0 + row < n ? key[(size_t)(i0 + row) * len + c0 + c] : 0u;
    }
    __syncthreads();
    const uint32_t* x = lx + wv * chunk;
    const uint32_t* y = ly + lane;
#pragma unroll 4
    for (uint32_t c = 0; c < wc; ++c) {
      const uint32_t xv = x[c], yv = y[c * TJP];
      np += ((xv != 0u) & (yv != 0u)) ? 1u : 0u;
      if (SHARED) ns += ((xv == yv) & (xv + 1u > 1u)) ? 1u : 0u;  // neither 0 nor kCmpUnaligned
    }
  }
  if (r < s && s < n) {  // both triangles from the upper one; the diagonal stays 0
    if (present) {
      present[(size_t)r * n + s] = np;
      present[(size_t)s * n + r] = np;
    }
    if (SHARED && shared) {
      shared[(size_t)r * n + s] = ns;
      shared[(size_t)s * n + r] = ns;
    }
  }
}

int cmp_map(const cmp_args& a, hipStream_t st) {
  STAGE_LAUNCH(ST_CMP_MAP, st) hipLaunchKernelGGL(k_cmp_map, dim3((a.n + 3) / 4), dim3(256), 0, st, a);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int cmp_count(const cmp_args& a, hipStream_t st) {
  if (hip_check(hipMemsetAsync(a.k, 0, (size_t)a.len_r * 4, st)) || hip_check(hipMemsetAsync(a.m, 0, (size_t)a.len_t * 4, st)) ||
      hip_check(hipMemsetAsync(a.cnt, 0, (size_t)a.len_r * a.len_t * 4, st)))
    return DAFS_HIP_ELAUNCH;
  const uint32_t by = (a.n + kCmpCountRows - 1) / kCmpCountRows;  // <= 2^14
  STAGE_LAUNCH(ST_CMP_COUNT_COLS, st)
  hipLaunchKernelGGL(k_cmp_count_cols, dim3((a.len_r + 255) / 256, by), dim3(256), 0, st, a.cell_r, a.use_r, a.n, a.len_r, a.k);
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  STAGE_LAUNCH(ST_CMP_COUNT_COLS, st)
  hipLaunchKernelGGL(k_cmp_count_cols, dim3((a.len_t + 255) / 256, by), dim3(256), 0, st, a.cell_t, a.use_t, a.n, a.len_t, a.m);
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  STAGE_LAUNCH(ST_CMP_COUNT, st) hipLaunchKernelGGL(k_cmp_count, dim3(a.n), dim3(256), 0, st, a);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int cmp_residue(const cmp_args& a, hipStream_t st) {
  if (hip_check(hipMemsetAsync(a.bins, 0, (size_t)3 * kCmpClasses * 8, st))) return DAFS_HIP_ELAUNCH;
  STAGE_LAUNCH(ST_CMP_RESIDUE, st) hipLaunchKernelGGL(k_cmp_residue, dim3(a.n), dim3(256), 0, st, a);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int cmp_columns(const cmp_args& a, hipStream_t st) {
  STAGE_LAUNCH(ST_CMP_COLUMNS, st) hipLaunchKernelGGL(k_cmp_columns, dim3((a.len_r + 3) / 4), dim3(256), 0, st, a);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int cmp_ss(const cmp_args& a, hipStream_t st) {
  STAGE_LAUNCH(ST_CMP_SS, st) hipLaunchKernelGGL(k_cmp_ss, dim3((a.n + 255) / 256), dim3(256), 0, st, a);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int cmp_pairs(const uint32_t* key, uint32_t n, uint32_t len, uint32_t chunk, uint32_t band_blocks, uint32_t* present, uint32_t* shared, hipStream_t st) {
  if (n < 2 || n > kCmpMatrixRows || !len || !chunk || chunk > kCmpMaxChunk || !band_blocks) return DAFS_HIP_EINVAL;
  if (chunk > len) chunk = len;
  const uint32_t bi = (n + TI - 1) / TI, bj = (n + TJ - 1) / TJ;  // <= 2^10 x 2^8
  const size_t lds = (size_t)chunk * (TJP + TI) * sizeof(uint32_t);
  // bands of rows r, so that one launch stays below band_blocks workgroups
  const uint32_t band = band_blocks / bj ? band_blocks / bj : 1;
  for (uint32_t i = 0; i < bi; i += band) {
    const dim3 grid(bi - i < band ? bi - i : band, bj);
    if (shared) {
      STAGE_LAUNCH(ST_CMP_PAIRS, st) hipLaunchKernelGGL(k_cmp_pairs<true>, grid, dim3(1024), lds, st, key, n, len, chunk, present, shared, i);
    } else {
      STAGE_LAUNCH(ST_CMP_PAIRS_OCC, st) hipLaunchKernelGGL(k_cmp_pairs<false>, grid, dim3(1024), lds, st, key, n, len, chunk, present, shared, i);
    }
    if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  }
  return DAFS_HIP_OK;
}

}  // namespace dafs
