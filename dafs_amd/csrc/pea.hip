// dafs_amd/csrc/pea.hip -- the two kernels that choose a level's threshold by pseudo-expected accuracy.
// Every cell counts as q(p) = trunc(clamp(p, 0, 1) * 2^30), an integer, and every sum is a sum of those in uint64: no order
// of summation and no floating-point rounding can move a decision.  k_pea_total sums the upper triangle of the unmasked
// matrix once (S); k_pea_pick sums, per candidate threshold, the cells its decode paired (T) and counts them (n), keeps the
// first candidate that no other beats, and lets it stand as the level only when it beats the levels already kept.  A
// structure (T, n) has F = 2 T / (n 2^30 + S); two of them are compared by cross-multiplying in 128-bit integers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dafs_hip.h"
#include "dd.h"
#include "hip_util.h"
#include "stage.h"

namespace dafs {

#define PEA_NONE 0xFFFFFFFFu
#define PEA_THREADS 256
#define PEA_ROWS 16  // matrix rows per workgroup of k_pea_total: four per wavefront, as k_levels_mask walks them

__device__ __forceinline__ uint64_t pea_q(float p) { return (uint64_t)(fminf(fmaxf(p, 0.0f), 1.0f) * 0x1p30f); }

__device__ __forceinline__ uint64_t pea_wave_sum(uint64_t v) {
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;  // lane 0 holds the wavefront's sum
}

// (ta, na) beats (tb, nb): ta (nb 2^30 + S) > tb (na 2^30 + S).  T < 2^45 and n 2^30 + S < 2^58 for every matrix that fits
// the device, so the products need more than 64 bits and fit 128 easily.
__device__ __forceinline__ bool pea_beats(uint64_t ta, uint64_t na, uint64_t tb, uint64_t nb, uint64_t S) {
  const unsigned __int128 l = (unsigned __int128)ta * (unsigned __int128)((nb << 30) + S);
  const unsigned __int128 r = (unsigned __int128)tb * (unsigned __int128)((na << 30) + S);
  return l > r;
}

// blockIdx.y: the alignment; blockIdx.x: PEA_ROWS of its rows, four per wavefront, the lanes along the row; cells right of
// the diagonal only.  A row of a multiple of four columns goes in float4 pieces.  One atomic add per workgroup.
__global__ __launch_bounds__(PEA_THREADS) void k_pea_total(const pea_desc* descs, const uint32_t* act) {
  __shared__ uint64_t s_part[PEA_THREADS / 64];
  const pea_desc d = descs[act[blockIdx.y]];
  const uint32_t L = d.L, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (blockIdx.x * PEA_ROWS + 1 >= L) return;  // no row of this workgroup has a cell (uniform: before any barrier)
  uint64_t sum = 0;
  for (uint32_t r = 0; r < PEA_ROWS / 4; ++r) {
    const uint32_t i = blockIdx.x * PEA_ROWS + wave * (PEA_ROWS / 4) + r;
    if (i + 1 >= L) break;
    const float* __restrict__ row = d.p + (size_t)i * L;
    if ((L & 3u) == 0) {
      for (uint32_t q = (i + 1) / 4 + lane; q < L / 4; q += 64) {
        const float4 v = *(const float4*)(row + 4 * q);
        if (4 * q > i) sum += pea_q(v.x);
        if (4 * q + 1 > i) sum += pea_q(v.y);
        if (4 * q + 2 > i) sum += pea_q(v.z);
        sum += pea_q(v.w);  // 4 q + 3 >= i + 1 for every piece from (i + 1) / 4 on
      }
    } else {
      for (uint32_t j = i + 1 + lane; j < L; j += 64) sum += pea_q(row[j]);
    }
  }
  sum = pea_wave_sum(sum);
  if (lane == 0) s_part[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (uint32_t w = 0; w < PEA_THREADS / 64; ++w) t += s_part[w];
    if (t) atomicAdd((unsigned long long*)d.sum, (unsigned long long)t);
  }
}

// One workgroup per alignment, after the C candidate decodes of level k: their T and n, the choice, and the level's own
// structure and score.  Every workgroup writes its own alignment's arrays only, with plain stores.
__global__ __launch_bounds__(PEA_THREADS) void k_pea_pick(const pea_desc* descs, const uint32_t* act, uint32_t k, uint32_t C) {
  __shared__ uint64_t s_t[DAFS_HIP_MAX_CANDIDATES][PEA_THREADS / 64];
  __shared__ uint32_t s_n[DAFS_HIP_MAX_CANDIDATES][PEA_THREADS / 64];
  __shared__ uint32_t s_best;
  const pea_desc d = descs[act[blockIdx.x]];
  const uint32_t L = d.L, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (uint32_t c = 0; c < C; ++c) {
    const uint32_t* __restrict__ ss = d.css + (size_t)c * (L + 1);
    uint64_t t = 0;
    uint32_t n = 0;
    for (uint32_t i = tid; i < L; i += PEA_THREADS) {
      const uint32_t j = ss[i];
      if (j < L) { t += pea_q(d.p[(size_t)i * L + j]); ++n; }
    }
    t = pea_wave_sum(t);
    for (int s = 32; s > 0; s >>= 1) n += __shfl_down(n, s, 64);  // at most L / 2 pairs: 32 bits
    if (lane == 0) { s_t[c][wave] = t; s_n[c][wave] = n; }
  }
  __syncthreads();
  if (tid == 0) {
    const uint64_t S = *d.sum, t_low = d.base[0], n_low = d.base[1];
    uint64_t best_t = 0, best_n = 0;
    uint32_t best = PEA_NONE;
    for (uint32_t c = 0; c < C; ++c) {
      uint64_t t = 0, n = 0;
      for (uint32_t w = 0; w < PEA_THREADS / 64; ++w) { t += s_t[c][w]; n += s_n[c][w]; }
      d.ctp[(size_t)k * C + c] = t;
      d.cnp[(size_t)k * C + c] = (uint32_t)n;
      // ties go to the earlier, higher threshold: a later one has to beat it
      if (best == PEA_NONE || pea_beats(t_low + t, n_low + n, t_low + best_t, n_low + best_n, S)) { best = c; best_t = t; best_n = n; }
    }
    const bool keep = pea_beats(t_low + best_t, n_low + best_n, t_low, n_low, S);
    d.chosen[k] = keep ? best : PEA_NONE;
    d.tp[k] = keep ? best_t : 0;
    d.np[k] = keep ? (uint32_t)best_n : 0u;
    d.score[k] = keep ? d.cscore[best] : 0.0f;
    if (keep) { d.base[0] = t_low + best_t; d.base[1] = n_low + best_n; }
    s_best = keep ? best : PEA_NONE;
  }
  __syncthreads();
  const uint32_t best = s_best;
  if (best == PEA_NONE) {
    for (uint32_t i = tid; i < L; i += PEA_THREADS) d.lss[i] = PEA_NONE;
  } else {
    const uint32_t* __restrict__ ss = d.css + (size_t)best * (L + 1);
    for (uint32_t i = tid; i < L; i += PEA_THREADS) d.lss[i] = ss[i];
  }
}

int pea_total_launch(const pea_desc* d_descs, const uint32_t* d_act, uint32_t n, uint32_t max_len, hipStream_t st) {
  if (!n || max_len < 2) return DAFS_HIP_OK;
  if (n > 65535) return DAFS_HIP_EINVAL;  // one grid y per alignment
  STAGE_LAUNCH(ST_PEA_TOTAL, st)
    hipLaunchKernelGGL(k_pea_total, dim3((max_len + PEA_ROWS - 1) / PEA_ROWS, n), dim3(PEA_THREADS), 0, st, d_descs, d_act);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int pea_pick_launch(const pea_desc* d_descs, const uint32_t* d_act, uint32_t n, uint32_t k, uint32_t ncand, hipStream_t st) {
  if (!n) return DAFS_HIP_OK;
  if (ncand < 1 || ncand > DAFS_HIP_MAX_CANDIDATES) return DAFS_HIP_EINVAL;
  STAGE_LAUNCH(ST_PEA_PICK, st) hipLaunchKernelGGL(k_pea_pick, dim3(n), dim3(PEA_THREADS), 0, st, d_descs, d_act, k, ncand);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

}  // namespace dafs
