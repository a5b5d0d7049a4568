// dafs_amd/csrc/nj.hip -- neighbour joining on the device (the reference has no counterpart,
// tests/nj_ref.py is the plain restatement).
//
// k_nj_init    a grid over the rows, one wavefront per row: the symmetric working copy D from the upper triangle of the input
//              (0 on the diagonal), the count of non-finite entries among those read, the leaves and zeroed lengths.
// k_nj_rowsum  one thread per row k: R[k], the running sum of column k of D in ascending row order (D is symmetric, so the
//              threads of a wavefront read neighbouring words; the diagonal's +0 leaves every bit of the sum alone).
// k_nj_pick    a grid over the rows, one wavefront per active row i: the smallest Q(i, j) over the active j > i and the smallest
//              j holding it, into (row_q, row_j).  Retired rows exit at once.
// k_nj_update  ONE workgroup: the rows' tuples reduced to the pair (a, b), the two branch lengths, the O(m) update of row and
//              column a and of R, then R[a] summed by one wavefront in ascending k, and the retirement of b.
//
// Q changes in every entry at every join, so no per-row cache survives a join (unlike linkage.hip): every join scans all active
// pairs, which one workgroup cannot do in acceptable time at large n.  The order between the steps of a join is therefore
// stream order (pick, then update, enqueued back to back, 2 (n - 1) launches fixed by n alone) and, inside k_nj_update,
// __syncthreads().  No workgroup waits for another and nothing polls.
//
// A retired slot b keeps R[b] = NaN: Q(i, b) is then NaN, which no comparison prefers, so the scan reads no activity flag.
// Among active slots a NaN in Q needs an infinite R, which was counted when it was written, and the call then refuses.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dafs_hip.h"
#include "hip_util.h"
#include "nj.h"
#include "stage.h"

namespace dafs {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kUpdateWaves = kNjUpdateThreads / 64;

__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ uint32_t nonfinite(double v) {
  return ((unsigned long long)__double_as_longlong(v) & 0x7FF0000000000000ull) == 0x7FF0000000000000ull ? 1u : 0u;
}

// (value ascending, index ascending); a NaN is never better, and (+inf, kNone) is "no candidate"
__device__ __forceinline__ bool better(double v1, uint32_t i1, double v2, uint32_t i2) { return v1 < v2 || (v1 == v2 && i1 < i2); }

__device__ __forceinline__ void wave_best(double& v, uint32_t& i) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double ov = __shfl_xor(v, d, 64);
    const uint32_t oi = __shfl_xor(i, d, 64);
    if (better(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

// lane l's value in every lane (l is a constant after unrolling: two v_readlane_b32)
__device__ __forceinline__ double lane_value(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

__global__ __launch_bounds__(kNjRowThreads) void k_nj_init(uint32_t n, const double* __restrict__ dist, double* __restrict__ D, nj_head* head,
                                                           int32_t* node, int32_t* left, int32_t* right, double* length) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t row = blockIdx.x * (kNjRowThreads / 64) + (threadIdx.x >> 6);
  if (row >= n) return;
  double* out = D + (size_t)row * n;
  uint32_t bad = 0;
  for (uint32_t j = lane; j < n; j += 64) {
    double v = 0.0;
    if (j > row) {
      v = dist[(size_t)row * n + j];
      bad += nonfinite(v);  // counted once, from the row that owns the entry
    } else if (j < row) {
      v = dist[(size_t)j * n + row];
    }
    out[j] = v;
  }
  if (bad) atomicAdd(&head->nonfinite, bad);
  if (lane == 0) {
    node[row] = (int32_t)row;
    left[row] = -1;
    right[row] = -1;
    length[row] = 0.0;
    if (row + 1 < n) length[n + row] = 0.0;  // the root's stays
  }
}

__global__ __launch_bounds__(kNjRowThreads) void k_nj_rowsum(uint32_t n, const double* __restrict__ D, nj_head* head, double* R) {
  const uint32_t k = blockIdx.x * kNjRowThreads + threadIdx.x;
  if (k >= n || head->nonfinite) return;  // refused: no join runs
  double s = 0.0;
#pragma unroll 8
  for (uint32_t j = 0; j < n; ++j) s += D[(size_t)j * n + k];
  R[k] = s;
  if (nonfinite(s)) atomicAdd(&head->written, 1u);
}

__global__ __launch_bounds__(kNjRowThreads) void k_nj_pick(uint32_t n, uint32_t m, const double* __restrict__ D, const double* __restrict__ R,
                                                           const int32_t* __restrict__ node, const nj_head* head, double* row_q, uint32_t* row_j) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * (kNjRowThreads / 64) + (threadIdx.x >> 6);
  if (i >= n || node[i] < 0 || head->nonfinite) return;
  const double* Di = D + (size_t)i * n;
  const double c = (double)(m - 2), Ri = R[i];
  double bq = pos_inf();
  uint32_t bj = kNone;
#pragma unroll 4
  for (uint32_t j = i + 1 + lane; j < n; j += 64) {
    const double q = (c * Di[j] - Ri) - R[j];
    if (q < bq) { bq = q; bj = j; }  // j ascends within a lane: the first of equals stays
  }
  wave_best(bq, bj);
  if (lane == 0) { row_q[i] = bq; row_j[i] = bj; }
}

__global__ __launch_bounds__(kNjUpdateThreads) void k_nj_update(uint32_t n, uint32_t t, double* D, double* R, int32_t* node, nj_head* head,
                                                                const double* __restrict__ row_q, const uint32_t* __restrict__ row_j,
                                                                int32_t* left, int32_t* right, double* length) {
  extern __shared__ __align__(16) unsigned char lds_row[];  // the new row a: nj_update_lds_bytes(n)
  __shared__ double red_v[kUpdateWaves];
  __shared__ uint32_t red_i[kUpdateWaves];
  __shared__ uint32_t pick[2];
  if (head->nonfinite) return;  // refused: no join runs
  const uint32_t chunks = (n + 63) / 64;
  double* row_u = (double*)lds_row;                                                   // per slot the new D(a, k), +0 where k takes no part
  unsigned long long* row_part = (unsigned long long*)(row_u + (size_t)(chunks + 1) * 64);  // per 64 slots: which take part
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t m = n - t;
  // the best pair: the smallest active row whose minimum is the overall minimum, and that row's column
  double bv = pos_inf();
  uint32_t bi = kNone;
  for (uint32_t i = tid; i < n; i += kNjUpdateThreads) {
    if (node[i] < 0 || row_j[i] == kNone) continue;
    const double v = row_q[i];
    if (v < bv) { bv = v; bi = i; }
  }
  wave_best(bv, bi);
  if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
  __syncthreads();
  if (wave == 0) {
    bv = lane < kUpdateWaves ? red_v[lane] : pos_inf();
    bi = lane < kUpdateWaves ? red_i[lane] : kNone;
    wave_best(bv, bi);
    if (lane == 0) {
      uint32_t a = bi, b = kNone;
      if (a < n) {
        b = row_j[a];
      } else {  // no Q below +inf: the candidate the scan starts from, the first two active slots
        a = kNone;
        for (uint32_t i = 0; i < n && b == kNone; ++i) {
          if (node[i] < 0) continue;
          if (a == kNone) a = i; else b = i;
        }
      }
      if (a >= n || b >= n || a >= b || node[a] < 0 || node[b] < 0) a = b = kNone;  // never index beyond the arrays
      pick[0] = a;
      pick[1] = b;
    }
  }
  __syncthreads();
  const uint32_t a = pick[0], b = pick[1];
  if (a == kNone) {
    if (tid == 0) head->fault = 1;
    return;
  }
  double* Da = D + (size_t)a * n;
  const double* Db = D + (size_t)b * n;
  const double dab = Da[b];
  uint32_t bad = 0;
  for (uint32_t base = wave * 64; base < n; base += kNjUpdateThreads) {  // a wavefront takes whole chunks of 64 slots
    const uint32_t k = base + lane;
    const bool part = k < n && k != a && k != b && node[k] >= 0;
    double u = 0.0;
    if (part) {
      const double p = Da[k], q = Db[k];
      u = 0.5 * ((p + q) - dab);
      const double r = ((R[k] - p) - q) + u;
      R[k] = r;
      Da[k] = u;
      D[(size_t)k * n + a] = u;
      bad += nonfinite(u) + nonfinite(r);
    }
    row_u[k] = u;
    const unsigned long long m_part = __ballot(part);
    if (lane == 0) row_part[base >> 6] = m_part;
  }
  if (tid == kNjUpdateThreads - 1) {  // the join itself, by a thread of the last wavefront
    double la = 0.5 * dab;
    if (m > 2) la = la + (R[a] - R[b]) / (2.0 * (double)(m - 2));
    const double lb = dab - la;
    const int32_t na = node[a], nb = node[b];
    length[na] = la;
    length[nb] = lb;
    left[n + t] = na;
    right[n + t] = nb;
    bad += nonfinite(la) + nonfinite(lb);
  }
  if (bad) atomicAdd(&head->written, bad);
  __syncthreads();  // the new row a in LDS; R[a], R[b], node[a], node[b] still as before the join
  if (wave != 0) return;
  // R[a]: the running sum of the new row a over the remaining active k, ascending: a chain of dependent additions, the one part
  // of a join that no second thread can help with.  One wavefront walks the row in LDS, a chunk of 64 slots per step with the
  // next one already on its way; every lane carries the same sum.  A well-filled chunk adds all 64 lanes' values in turn (a slot
  // that takes no part holds +0, which changes no bit of a sum that started at +0), a sparse one only the slots of its mask.
  double s = 0.0;
  double v = row_u[lane];
  unsigned long long m_part = row_part[0];
  for (uint32_t c = 0; c < chunks; ++c) {
    const double v_next = row_u[(size_t)(c + 1) * 64 + lane];  // the array ends in one chunk of padding
    const unsigned long long m_next = row_part[c + 1];
    unsigned long long todo = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(m_part >> 32)) << 32) |
                              (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)m_part);
    if (__popcll(todo) >= 24) {
#pragma unroll
      for (int l = 0; l < 64; ++l) s += lane_value(v, l);
    } else {
      while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        s += lane_value(v, l);
      }
    }
    v = v_next;
    m_part = m_next;
  }
  if (lane == 0) {
    R[a] = s;
    R[b] = quiet_nan();
    node[a] = (int32_t)(n + t);
    node[b] = -1;
    if (nonfinite(s)) atomicAdd(&head->written, 1u);
    head->joins = t + 1;
  }
}

}  // namespace

int nj_launch(uint32_t n, const double* dist, void* workspace, int32_t* left, int32_t* right, double* length, hipStream_t st) {
  if (n < 2 || n > kNjMaxN || !dist || !workspace || !left || !right || !length) return DAFS_HIP_EINVAL;
  static bool optin[16] = {};
  const size_t lds = nj_update_lds_bytes(n);
  if (lds > 48 * 1024 && !lds_optin_once((const void*)k_nj_update, (int)nj_update_lds_bytes(kNjMaxN), optin)) return DAFS_HIP_ELAUNCH;
  uint8_t* w = (uint8_t*)workspace;
  nj_head* head = (nj_head*)w;
  double* D = (double*)(w + kNjHeadBytes);
  uint8_t* per_row = w + kNjHeadBytes + nj_round((size_t)n * n * 8);
  double* R = (double*)per_row;
  double* row_q = (double*)(per_row + nj_round((size_t)n * 8));
  int32_t* node = (int32_t*)(per_row + 2 * nj_round((size_t)n * 8));
  uint32_t* row_j = (uint32_t*)(per_row + 2 * nj_round((size_t)n * 8) + nj_round((size_t)n * 4));
  if (hip_check(hipMemsetAsync(head, 0, kNjHeadBytes, st))) return DAFS_HIP_ELAUNCH;
  const uint32_t per_block = kNjRowThreads / 64;
  const dim3 rows((n + per_block - 1) / per_block);
  STAGE_LAUNCH(ST_NJ_INIT, st)
  hipLaunchKernelGGL(k_nj_init, rows, dim3(kNjRowThreads), 0, st, n, dist, D, head, node, left, right, length);
  STAGE_LAUNCH(ST_NJ_ROWSUM, st)
  hipLaunchKernelGGL(k_nj_rowsum, dim3((n + kNjRowThreads - 1) / kNjRowThreads), dim3(kNjRowThreads), 0, st, n, D, head, R);
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  for (uint32_t t = 0; t + 1 < n; ++t) {
    STAGE_LAUNCH(ST_NJ_PICK, st)
    hipLaunchKernelGGL(k_nj_pick, rows, dim3(kNjRowThreads), 0, st, n, n - t, D, R, node, head, row_q, row_j);
    STAGE_LAUNCH(ST_NJ_UPDATE, st)
    hipLaunchKernelGGL(k_nj_update, dim3(1), dim3(kNjUpdateThreads), lds, st, n, t, D, R, node, head, row_q, row_j, left, right, length);
    if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  }
  return DAFS_HIP_OK;
}

}  // namespace dafs
