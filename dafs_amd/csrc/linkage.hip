// dafs_amd/csrc/linkage.hip -- single, complete and average linkage on the device (the reference has no
// counterpart, tests/linkage_ref.py is the plain restatement).
//
// k_linkage_init   a grid over the rows, one wavefront per row: the symmetric working copy S from the upper triangle of the
//                  input (-inf on the diagonal), each row's nearest partner (value, smallest column among equals), the count
//                  of non-finite entries among those read, and the leaves of the output arrays.
// k_linkage_joins  ONE workgroup of 1024 threads makes all n - 1 joins in one launch.  A join is an argmax over n row maxima,
//                  two row reads, one row and one column write and the repair of the rows whose nearest partner was touched: a
//                  few microseconds, where a barrier across workgroups costs 26 us at 256 of them.  So a join never leaves the
//                  workgroup: every wait is a __syncthreads(), the loop has exactly n - 1 trips and nothing in it polls.
//
// Per row the kernel keeps (nn_val, nn_idx): the largest entry of the row of S and the smallest column holding it.  S is
// symmetric, so the best pair (highest value, then smallest a, then smallest b; a < b) is the smallest row a whose maximum is
// the overall maximum, with b = nn_idx[a]: a smaller row holding that value would be a smaller a, a smaller column of row a a
// smaller b.  Retired slots hold -inf in (nn_val, every column of theirs in an active row), so no scan tests for activity; the
// ROWS of retired slots are never read again and are left as they are.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dafs_hip.h"
#include "hip_util.h"
#include "linkage.h"
#include "stage.h"

namespace dafs {

namespace {

constexpr uint32_t kNeedScan = 0xFFFFFFFFu;  // nn_idx of a row that the repair step has to rescan
constexpr uint32_t kWaves = kLinkageThreads / 64;

__device__ __forceinline__ float neg_inf() { return __uint_as_float(0xFF800000u); }

// (value descending, index ascending); -0 equals 0
__device__ __forceinline__ bool better(float v1, uint32_t i1, float v2, uint32_t i2) { return v1 > v2 || (v1 == v2 && i1 < i2); }

__device__ __forceinline__ void wave_best(float& v, uint32_t& i) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const float ov = __shfl_xor(v, d, 64);
    const uint32_t oi = __shfl_xor(i, d, 64);
    if (better(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

// the largest entry of a row and the smallest column holding it, over the lanes of one wavefront (every lane gets it)
__device__ __forceinline__ void scan_row(const float* __restrict__ row, uint32_t n, uint32_t lane, float& bv, uint32_t& bi) {
  bv = neg_inf();
  bi = kNeedScan;
#pragma unroll 4
  for (uint32_t j = lane; j < n; j += 64) {
    const float v = row[j];
    if (v > bv) { bv = v; bi = j; }  // j ascends within a lane: the first of equals stays
  }
  wave_best(bv, bi);
}

// The new S(a, k) from p = S(a, k), q = S(b, k) and the sizes before the join.  Equal values (0 and -0) give slot a's.
template <int RULE>
__device__ __forceinline__ float joined(float p, float q, uint32_t na, uint32_t nb) {
  if (RULE == DAFS_LINKAGE_SINGLE) return p >= q ? p : q;
  if (RULE == DAFS_LINKAGE_COMPLETE) return p <= q ? p : q;
  // the products are exact in double; the sum, the quotient and the narrowing are one IEEE rounding each
  const double s = (double)na * (double)p + (double)nb * (double)q;
  return (float)(s / (double)(na + nb));
}

__global__ __launch_bounds__(kLinkageInitThreads) void k_linkage_init(uint32_t n, const float* __restrict__ sim, float* __restrict__ S,
                                                                      linkage_head* head, float* g_val, uint32_t* g_idx, float* score,
                                                                      int32_t* left, int32_t* right) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t row = blockIdx.x * (kLinkageInitThreads / 64) + (threadIdx.x >> 6);
  if (row >= n) return;
  float* out = S + (size_t)row * n;
  float bv = neg_inf();
  uint32_t bi = kNeedScan, bad = 0;
  for (uint32_t j = lane; j < n; j += 64) {
    float v = neg_inf();
    if (j > row) {
      v = sim[(size_t)row * n + j];
      if ((__float_as_uint(v) & 0x7F800000u) == 0x7F800000u) ++bad;  // counted once, from the row that owns the entry
    } else if (j < row) {
      v = sim[(size_t)j * n + row];
    }
    out[j] = v;
    if (v > bv) { bv = v; bi = j; }
  }
  if (bad) atomicAdd(&head->nonfinite, bad);
  wave_best(bv, bi);
  if (lane == 0) {
    g_val[row] = bv;
    g_idx[row] = bi == kNeedScan ? 0u : bi;
    score[row] = 0.0f;
    left[row] = -1;
    right[row] = -1;
  }
}

template <int RULE, bool LDS>
__global__ __launch_bounds__(kLinkageThreads) void k_linkage_joins(uint32_t n, float* S, linkage_head* head, float* g_val, uint32_t* g_idx,
                                                                   uint32_t* g_size, int32_t* g_node, float* score, int32_t* left,
                                                                   int32_t* right) {
  extern __shared__ __align__(16) unsigned char lds_rows[];
  __shared__ float red_v[kWaves];
  __shared__ uint32_t red_i[kWaves];
  __shared__ uint32_t pick[2];
  if (head->nonfinite) return;  // refused: no join runs
  float* nn_val = LDS ? (float*)lds_rows : g_val;
  uint32_t* nn_idx = LDS ? (uint32_t*)lds_rows + n : g_idx;
  uint32_t* size = LDS ? (uint32_t*)lds_rows + 2 * (size_t)n : g_size;
  int32_t* node = LDS ? (int32_t*)lds_rows + 3 * (size_t)n : g_node;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (uint32_t i = tid; i < n; i += kLinkageThreads) {
    if (LDS) { nn_val[i] = g_val[i]; nn_idx[i] = g_idx[i]; }
    size[i] = 1;
    node[i] = (int32_t)i;
  }
  __syncthreads();
  unsigned long long rescans = 0;
  uint32_t t = 0;
  for (; t + 1 < n; ++t) {
    // the best pair: the smallest row whose maximum is the overall maximum, and that row's nearest column
    float bv = neg_inf();
    uint32_t bi = kNeedScan;
    for (uint32_t i = tid; i < n; i += kLinkageThreads) {
      const float v = nn_val[i];
      if (v > bv) { bv = v; bi = i; }
    }
    wave_best(bv, bi);
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    if (wave == 0) {
      bv = lane < kWaves ? red_v[lane] : neg_inf();
      bi = lane < kWaves ? red_i[lane] : kNeedScan;
      wave_best(bv, bi);
      if (lane == 0) { pick[0] = bi; pick[1] = bi < n ? nn_idx[bi] : kNeedScan; }
    }
    __syncthreads();
    const uint32_t a = pick[0], b = pick[1];
    if (a >= n || b >= n || a == b) break;  // finite input always leaves a pair; never index beyond the matrix
    const uint32_t na = size[a], nb = size[b];
    float* Sa = S + (size_t)a * n;
    float* Sb = S + (size_t)b * n;
    // row a and column a from rows a and b, slot b retired, and the repair of every other row's nearest partner
    bv = neg_inf();
    bi = kNeedScan;
    for (uint32_t k = tid; k < n; k += kLinkageThreads) {
      if (k == a) continue;
      if (k == b) {  // one lane writes the join, from the entry it then retires
        score[n + t] = Sa[b];
        left[n + t] = node[a];
        right[n + t] = node[b];
        Sa[b] = neg_inf();
        Sb[a] = neg_inf();
        continue;
      }
      const float mv = nn_val[k];
      if (!(mv > neg_inf())) continue;  // a retired slot: its column of rows a and b holds -inf already
      const float v = joined<RULE>(Sa[k], Sb[k], na, nb);
      Sa[k] = v;
      S[(size_t)k * n + a] = v;
      Sb[k] = neg_inf();
      S[(size_t)k * n + b] = neg_inf();
      if (v > bv) { bv = v; bi = k; }
      const uint32_t mi = nn_idx[k];
      if (mi == a || mi == b) {
        // v <= max(p, q) <= mv.  Equal: no column below mi was tied and a <= mi, so a is the nearest now.  Lower: rescan.
        if (v >= mv) { nn_val[k] = v; nn_idx[k] = a; }
        else nn_idx[k] = kNeedScan;
      } else if (v == mv && a < mi) {
        nn_idx[k] = a;
      }
    }
    wave_best(bv, bi);
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    if (wave == 0) {
      bv = lane < kWaves ? red_v[lane] : neg_inf();
      bi = lane < kWaves ? red_i[lane] : kNeedScan;
      wave_best(bv, bi);
      if (lane == 0) {
        nn_val[a] = bv;
        nn_idx[a] = bi == kNeedScan ? 0u : bi;
        nn_val[b] = neg_inf();
        size[a] = na + nb;
        node[a] = (int32_t)(n + t);
      }
    }
    __syncthreads();  // S and the per-row state as the join left them
    // rescans, one row per wavefront; a wavefront owns the rows of its 64-row chunks
    for (uint32_t base = wave * 64; base < n; base += kLinkageThreads) {
      const uint32_t k = base + lane;
      unsigned long long todo = __ballot(k < n && nn_idx[k] == kNeedScan);
      while (todo) {
        const uint32_t row = base + (uint32_t)(__ffsll((long long)todo) - 1);
        todo &= todo - 1;
        float v;
        uint32_t i;
        scan_row(S + (size_t)row * n, n, lane, v, i);
        if (lane == 0) { nn_val[row] = v; nn_idx[row] = i == kNeedScan ? 0u : i; ++rescans; }
      }
    }
    __syncthreads();
  }
  if (tid == 0) head->joins = t;
  if (lane == 0 && rescans) atomicAdd(&head->rescans, rescans);
}

template <int RULE>
int launch_joins(uint32_t n, float* S, linkage_head* head, float* g_val, uint32_t* g_idx, uint32_t* g_size, int32_t* g_node, float* score,
                 int32_t* left, int32_t* right, bool use_lds, hipStream_t st) {
  static bool optin[16] = {};
  if (use_lds) {
    const size_t lds = (size_t)n * 16;
    if (lds > 64 * 1024 && !lds_optin_once((const void*)k_linkage_joins<RULE, true>, (int)(kLinkageLdsBytes - kLinkageLdsScratch), optin))
      return DAFS_HIP_ELAUNCH;
    STAGE_LAUNCH(ST_LINKAGE_JOINS, st)
    hipLaunchKernelGGL((k_linkage_joins<RULE, true>), dim3(1), dim3(kLinkageThreads), lds, st, n, S, head, g_val, g_idx, g_size, g_node, score,
                       left, right);
  } else {
    STAGE_LAUNCH(ST_LINKAGE_JOINS, st)
    hipLaunchKernelGGL((k_linkage_joins<RULE, false>), dim3(1), dim3(kLinkageThreads), 0, st, n, S, head, g_val, g_idx, g_size, g_node, score,
                       left, right);
  }
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

}  // namespace

int linkage_launch(int linkage, uint32_t n, const float* sim, void* workspace, float* score, int32_t* left, int32_t* right, bool use_lds,
                   hipStream_t st) {
  if (n < 2 || n > kLinkageMaxN || !sim || !workspace || !score || !left || !right) return DAFS_HIP_EINVAL;
  if (use_lds && !linkage_fits_lds(n)) return DAFS_HIP_EINVAL;
  uint8_t* w = (uint8_t*)workspace;
  linkage_head* head = (linkage_head*)w;
  float* S = (float*)(w + kLinkageHeadBytes);
  const size_t rows = ((size_t)n * 4 + 255) & ~(size_t)255;
  uint8_t* per_row = w + kLinkageHeadBytes + (((size_t)n * n * 4 + 255) & ~(size_t)255);
  float* g_val = (float*)per_row;
  uint32_t* g_idx = (uint32_t*)(per_row + rows);
  uint32_t* g_size = (uint32_t*)(per_row + 2 * rows);
  int32_t* g_node = (int32_t*)(per_row + 3 * rows);
  if (hip_check(hipMemsetAsync(head, 0, kLinkageHeadBytes, st))) return DAFS_HIP_ELAUNCH;
  const uint32_t per_block = kLinkageInitThreads / 64;
  STAGE_LAUNCH(ST_LINKAGE_INIT, st)
  hipLaunchKernelGGL(k_linkage_init, dim3((n + per_block - 1) / per_block), dim3(kLinkageInitThreads), 0, st, n, sim, S, head, g_val, g_idx, score,
                     left, right);
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  switch (linkage) {
    case DAFS_LINKAGE_SINGLE: return launch_joins<DAFS_LINKAGE_SINGLE>(n, S, head, g_val, g_idx, g_size, g_node, score, left, right, use_lds, st);
    case DAFS_LINKAGE_COMPLETE: return launch_joins<DAFS_LINKAGE_COMPLETE>(n, S, head, g_val, g_idx, g_size, g_node, score, left, right, use_lds, st);
    case DAFS_LINKAGE_AVERAGE: return launch_joins<DAFS_LINKAGE_AVERAGE>(n, S, head, g_val, g_idx, g_size, g_node, score, left, right, use_lds, st);
  }
  return DAFS_HIP_EINVAL;
}

}  // namespace dafs
