// dafs_amd/csrc/levels.hip -- the two kernels between the levels of a level-by-level decode.
// Level k of the decode is the standalone Nussinov decoder (k_nussinov_batch, dd.hip) on the matrix in which every cell is
// zero that has an end paired at a lower level or that crosses no pair of some lower level: constraints 1 and 3 of IPknot's
// program (reference src/ipknot.cpp:145-206), constraint 2 being the decoder's own.  k_levels_merge folds a level's
// structure into the merged one and derives the level's column keys; k_levels_mask applies them to the matrix in place.
// Masks only grow with the level, so only the newest level's has to be applied.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dafs_hip.h"
#include "dd.h"
#include "hip_util.h"
#include "stage.h"

namespace dafs {

#define LV_NONE 0xFFFFFFFFu
#define LV_THREADS 256
#define LV_LDS_COLS 4096  // alignments up to this width walk their keys in LDS
#define LV_ROWS 16        // matrix rows per workgroup of k_levels_mask: four per wavefront

// The keys of a nested structure s over L columns, by one lane: a walk with the stack threaded through key itself (an open
// pair's key holds the pair that was open before it until its right end closes it).
__device__ void lv_keys(uint32_t L, const uint32_t* s, uint32_t* key) {
  uint32_t cur = LV_NONE;
  for (uint32_t c = 0; c < L; ++c) {
    if (s[c] != LV_NONE) { key[c] = cur; cur = c; }
    else if (cur != LV_NONE && s[cur] == c) { const uint32_t up = key[cur]; key[cur] = kLvPaired; key[c] = kLvPaired; cur = up; }
    else key[c] = cur;
  }
}

// One workgroup per alignment; every workgroup writes its own alignment's arrays only.
__global__ __launch_bounds__(LV_THREADS) void k_levels_merge(const lv_desc* descs, const uint32_t* act, uint32_t k, int want_key) {
  __shared__ uint32_t s_ss[LV_LDS_COLS], s_key[LV_LDS_COLS];
  const lv_desc d = descs[act[blockIdx.x]];
  const uint32_t L = d.L, tid = threadIdx.x;
  if (k == 0) {
    for (uint32_t i = tid; i < L; i += LV_THREADS) { d.ss[i] = LV_NONE; d.level[i] = 0xFF; }
    __syncthreads();
  }
  int any = 0;
  for (uint32_t i = tid; i < L; i += LV_THREADS) {
    const uint32_t j = d.lss[i];
    if (j < L) { d.ss[i] = j; d.level[i] = (uint8_t)k; d.level[j] = (uint8_t)k; any = 1; }  // a column is in one pair: no two lanes meet
  }
  any = __syncthreads_or(any);
  if (tid == 0) d.flag[(size_t)k * d.flag_stride] = any ? 1u : 0u;
  if (!want_key || !any) return;  // no pair: every higher level is empty, nothing reads the keys
  if (L <= LV_LDS_COLS) {
    for (uint32_t i = tid; i < L; i += LV_THREADS) s_ss[i] = d.lss[i];
    __syncthreads();
    if (tid == 0) lv_keys(L, s_ss, s_key);
    __syncthreads();
    for (uint32_t i = tid; i < L; i += LV_THREADS) d.key[i] = s_key[i];
  } else if (tid == 0) lv_keys(L, d.lss, d.key);
}

// blockIdx.y: the alignment; blockIdx.x: LV_ROWS of its rows, four per wavefront, the lanes along the row.  Only cells right
// of the diagonal: the decoders read p[i * L + j] with i < j and nothing else (nuss_cell, nuss_wg_span in dd.hip).  A row of
// a multiple of four columns goes in float4 pieces, read only where a piece keeps some of its cells.
__global__ __launch_bounds__(LV_THREADS) void k_levels_mask(const lv_desc* descs, const uint32_t* act) {
  const lv_desc d = descs[act[blockIdx.y]];
  const uint32_t L = d.L, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t* __restrict__ key = d.key;
  for (uint32_t r = 0; r < LV_ROWS / 4; ++r) {
    const uint32_t i = blockIdx.x * LV_ROWS + wave * (LV_ROWS / 4) + r;
    if (i + 1 >= L) return;
    const uint32_t ki = key[i];
    float* row = d.p + (size_t)i * L;
    auto gone = [&](uint32_t j, uint32_t kj) { return j > i && (ki == kLvPaired || kj == kLvPaired || kj == ki); };
    if ((L & 3u) == 0) {
      for (uint32_t q = (i + 1) / 4 + lane; q < L / 4; q += 64) {
        const uint4 kj = *(const uint4*)(key + 4 * q);
        const bool g0 = gone(4 * q, kj.x), g1 = gone(4 * q + 1, kj.y), g2 = gone(4 * q + 2, kj.z), g3 = gone(4 * q + 3, kj.w);
        if (!(g0 || g1 || g2 || g3)) continue;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (!(g0 && g1 && g2 && g3)) v = *(const float4*)(row + 4 * q);
        if (g0) v.x = 0.0f;
        if (g1) v.y = 0.0f;
        if (g2) v.z = 0.0f;
        if (g3) v.w = 0.0f;
        *(float4*)(row + 4 * q) = v;
      }
    } else {
      for (uint32_t j = i + 1 + lane; j < L; j += 64)
        if (gone(j, key[j])) row[j] = 0.0f;
    }
  }
}

int levels_merge_launch(const lv_desc* d_descs, const uint32_t* d_act, uint32_t n, uint32_t k, int want_key, hipStream_t st) {
  if (!n) return DAFS_HIP_OK;
  STAGE_LAUNCH(ST_LEVELS_MERGE, st) hipLaunchKernelGGL(k_levels_merge, dim3(n), dim3(LV_THREADS), 0, st, d_descs, d_act, k, want_key);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int levels_mask_launch(const lv_desc* d_descs, const uint32_t* d_act, uint32_t n, uint32_t max_len, hipStream_t st) {
  if (!n || max_len < 2) return DAFS_HIP_OK;
  if (n > 65535) return DAFS_HIP_EINVAL;  // one grid y per alignment
  STAGE_LAUNCH(ST_LEVELS_MASK, st)
    hipLaunchKernelGGL(k_levels_mask, dim3((max_len + LV_ROWS - 1) / LV_ROWS, n), dim3(LV_THREADS), 0, st, d_descs, d_act);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

}  // namespace dafs
