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
//
// The steps themselves (the working copy, the column sums, the scan of a row, the settling of the pair, the update, the branch
// lengths, the running sum of R[a], the retirement) are nj_steps.h's, shared with k_nj_batch (nj_boot.hip).  What is this
// file's own: R, node and the rows' tuples (row_q, row_j) in global memory, the counts of non-finite values added to nj_head
// as they arise, and the loop over the joins as launches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dafs_hip.h"
#include "hip_util.h"
#include "nj.h"
#include "nj_steps.h"
#include "stage.h"

namespace dafs {

namespace {

using namespace nj;

constexpr uint32_t kUpdateWaves = kNjUpdateThreads / 64;

__global__ __launch_bounds__(kNjRowThreads) void k_nj_init(uint32_t n, const double* __restrict__ dist, double* __restrict__ D, nj_head* head,
                                                           int32_t* node, int32_t* left, int32_t* right, double* length) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t row = blockIdx.x * (kNjRowThreads / 64) + (threadIdx.x >> 6);
  if (row >= n) return;
  const uint32_t bad = sym_row(n, row, lane, dist, D);
  if (bad) atomicAdd(&head->nonfinite, bad);
  if (lane == 0) leaf(n, row, node, left, right, length);
}

__global__ __launch_bounds__(kNjRowThreads) void k_nj_rowsum(uint32_t n, const double* __restrict__ D, nj_head* head, double* R) {
  const uint32_t k = blockIdx.x * kNjRowThreads + threadIdx.x;
  if (k >= n || head->nonfinite) return;  // refused: no join runs
  const double s = column_sum(n, k, D);
  R[k] = s;
  if (nonfinite(s)) atomicAdd(&head->written, 1u);
}

__global__ __launch_bounds__(kNjRowThreads) void k_nj_pick(uint32_t n, uint32_t m, const double* __restrict__ D, const double* __restrict__ R,
                                                           const int32_t* __restrict__ node, const nj_head* head, double* row_q, uint32_t* row_j) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * (kNjRowThreads / 64) + (threadIdx.x >> 6);
  if (i >= n || node[i] < 0 || head->nonfinite) return;
  best b = scan_row<4, false>(n, i, lane, others(m), D, R, best{pos_inf(), kNone});
  wave_best(b.q, b.k);
  if (lane == 0) { row_q[i] = b.q; row_j[i] = b.k; }
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
  // the best pair: the smallest active row whose minimum is the overall minimum, and that row's column
  double bv = pos_inf();
  uint32_t bi = kNone;
  for (uint32_t i = tid; i < n; i += kNjUpdateThreads) {
    if (node[i] < 0 || row_j[i] == kNone) continue;
    const double v = row_q[i];
    if (v < bv) { bv = v; bi = i; }
  }
  group_best<kUpdateWaves>(bv, bi, red_v, red_i);
  if (tid == 0) {
    const slots s = settle_pair(n, node, bi, bi < n ? row_j[bi] : kNone);
    pick[0] = s.a;
    pick[1] = s.b;
  }
  __syncthreads();
  const uint32_t a = pick[0], b = pick[1];
  if (a == kNone) {
    if (tid == 0) head->fault = 1;
    return;
  }
  const double dab = D[(size_t)a * n + b];
  uint32_t bad = update_row<kNjUpdateThreads>(n, a, b, dab, D, R, node, row_u, row_part);
  if (tid == kNjUpdateThreads - 1) bad += join_pair(n, t, n - t, a, b, dab, R, node, left, right, length);  // a thread of the last wavefront
  if (bad) atomicAdd(&head->written, bad);
  __syncthreads();  // the new row a in LDS; R[a], R[b], node[a], node[b] still as before the join
  if (wave != 0) return;
  const double s = row_sum(chunks, lane, row_u, row_part);
  if (lane == 0) {
    if (retire(n, t, a, b, s, R, node)) atomicAdd(&head->written, 1u);
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
