// dafs_amd/csrc/nj_boot.hip -- the bootstrap of the neighbour-joining tree on the device (the reference
// has no counterpart, tests/bootstrap_ref.py is the plain restatement).
//
// k_boot_pack  one thread per (replicate, row, word of 64 columns): the draws of its 64 positions (stateless: a draw is one
//              mix of the replicate's base and the position, so no draw is ever stored), the row's cells in the drawn
//              columns, and the four plane words of alistat.h (ali_pack_cell), word-major per replicate.
// k_boot_dist  the pair-count tile of k_ali_pairs<ALI_MATRIX> (alistat.hip) with a grid dimension over the replicates; the
//              tile's shape, its place in LDS, the staging and the counts are ali_tile.h's (ALI_TILE_COUNTS); only the
//              planes' base differs.  The lane that owns r < s turns its two counts into the distance of section 22 and
//              writes that one double; the count matrices are never stored.  A Jukes-Cantor value that comes within `guard`
//              of a quantisation step goes to a list that the host recomputes with its own log().
// k_nj_batch   ONE workgroup per matrix: all n - 1 joins of section 22 inside it, in the style of k_linkage_joins.  Every wait
//              is a __syncthreads(), the loop has exactly n - 1 trips, nothing polls and no workgroup knows of another.  D is
//              the matrix's working copy in global memory; R, node, the wavefronts' pick tuples and the row of the join
//              are in LDS.  Every step of a join is nj_steps.h's, the same code as nj.hip's kernels run.  What is this
//              kernel's own: a wavefront scans all its active rows i, rows and columns ascending, into one tuple, so a lane
//              keeps the first smallest (i, j) it met; one butterfly over (Q, i << 16 | j) per wavefront and one over the 16
//              wavefronts leave the smallest Q, then the smallest a, then the smallest b.  The counts of non-finite values
//              stay in registers until the last join.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/dafs_hip.h"
#include "ali_tile.h"
#include "alistat.h"
#include "call_host.h"
#include "hip_util.h"
#include "nj_boot.h"
#include "nj_steps.h"
#include "stage.h"

namespace dafs {

namespace {

using namespace nj;

constexpr uint32_t kBatchWaves = kNjBatchThreads / 64;
static_assert(kNjBatchMaxN <= 0xFFFFu, "k_nj_batch keeps a pair as i << 16 | j, and kNone must decode to a slot above every n");

__global__ __launch_bounds__(256) void k_boot_pack(boot_args a) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x, w = blockIdx.y, kk = blockIdx.z;
  if (r >= a.n) return;
  const uint64_t base = mix64(a.seed + kMixGolden * (uint64_t)(a.k0 + kk + 1));
  uint64_t word[4] = {0ull, 0ull, 0ull, 0ull};
  const uint32_t c1 = a.U - w * 64 < 64 ? a.U - w * 64 : 64;
  for (uint32_t b = 0; b < c1; ++b) {
    const uint32_t u = (uint32_t)(((mix64(base + (uint64_t)(w * 64 + b)) >> 32) * (uint64_t)a.U) >> 32);  // below U
    ali_pack_cell(a.cells[(size_t)u * a.n + r], b, word);
  }
  uint64_t* planes = a.planes + (size_t)kk * a.words * 4 * a.n;
#pragma unroll
  for (int p = 0; p < 4; ++p) planes[((size_t)w * 4 + p) * a.n + r] = word[p];
}

__global__ __launch_bounds__(ALI_TILE_THREADS) void k_boot_dist(boot_args a, uint32_t kk0) {
  extern __shared__ uint64_t lds[];  // ali_tile_shape::lds
  const uint32_t i0 = blockIdx.x * ALI_TI, j0 = blockIdx.y * ALI_TJ, kk = kk0 + blockIdx.z;
  if (!ali_tile_upper(i0, j0)) return;  // the whole workgroup leaves
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t r = i0 + wv, s = j0 + lane;
  const uint64_t* planes = a.planes + (size_t)kk * a.words * 4 * a.n;
  uint64_t* ly = ali_tile_y(lds);
  uint64_t* lx = ali_tile_x(lds, a.chunk);
  uint32_t ident = 0, comp = 0;
  ALI_TILE_COUNTS(planes, a.n, a.words, a.chunk, i0, j0, wv, lane, ly, lx, true, ident, comp);
  if (!(r < s && s < a.n)) return;
  const uint32_t mism = comp - ident;
  double d;
  if (a.model == DAFS_NJ_P) {
    d = comp ? (double)mism / (double)comp : 1.0;
  } else if (comp == 0 || 4 * (uint64_t)mism >= 3 * (uint64_t)comp) {
    d = 3.0;
  } else {
    const double kQ = 1048576.0, kCapK = 3.0 * 1048576.0;
    const double x = 1.0 - (4.0 * (double)mism) / (3.0 * (double)comp);
    const double y = -0.75 * log(x) * kQ + 0.5;
    double k = floor(y);
    // the host's log() may differ from this one in its last bits, which moves k only where y comes close to an integer
    if (y - k <= a.guard || (k + 1.0) - y <= a.guard) {
      const uint32_t at = atomicAdd(a.fix_count, 1u);
      if (at < a.fix_cap) a.fix[at] = boot_fix{kk, r, s, mism, comp};
    }
    if (!(k < kCapK)) k = kCapK;
    d = k / kQ;
  }
  a.dist[((size_t)kk * a.n + r) * a.n + s] = d;
}

__global__ __launch_bounds__(kNjBatchThreads) void k_nj_batch(uint32_t n, const double* __restrict__ dist, double* copies, size_t copy_doubles,
                                                              nj_head* heads, int32_t* left, int32_t* right, double* length) {
  extern __shared__ __align__(16) unsigned char lds_state[];  // nj_batch_lds_bytes(n)
  __shared__ double red_v[kBatchWaves];
  __shared__ uint32_t red_k[kBatchWaves];
  __shared__ uint32_t pick[2];
  __shared__ uint32_t bad_in;
  const uint32_t chunks = (n + 63) / 64;
  double* R = (double*)lds_state;                                                           // per slot; NaN once retired
  double* row_u = R + (size_t)chunks * 64;                                                  // per slot the new D(a, k), +0 where k takes no part
  unsigned long long* row_part = (unsigned long long*)(row_u + (size_t)(chunks + 1) * 64);  // per 64 slots: which take part
  int32_t* node = (int32_t*)(row_part + chunks + 1);                                        // per slot; -1 once retired
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t T = 2 * (size_t)n - 1;
  const double* in = dist + (size_t)blockIdx.x * n * n;
  double* D = copies + (size_t)blockIdx.x * copy_doubles;
  nj_head* head = heads + blockIdx.x;
  left += blockIdx.x * T;
  right += blockIdx.x * T;
  length += blockIdx.x * T;

  // the symmetric working copy from the upper triangle, the leaves, zeroed lengths (k_nj_init)
  if (tid == 0) bad_in = 0;
  __syncthreads();
  uint32_t bad = 0;
  for (uint32_t row = wave; row < n; row += kBatchWaves) bad += sym_row(n, row, lane, in, D);
  for (uint32_t i = tid; i < n; i += kNjBatchThreads) leaf(n, i, node, left, right, length);
  if (bad) atomicAdd(&bad_in, bad);
  __syncthreads();
  if (bad_in) {  // refused: no join runs (the whole workgroup leaves)
    if (tid == 0) head->nonfinite = bad_in;
    return;
  }
  // R[k]: the running sum of column k in ascending row order (k_nj_rowsum)
  uint32_t written = 0;
  for (uint32_t k = tid; k < n; k += kNjBatchThreads) {
    const double s = column_sum(n, k, D);
    R[k] = s;
    written += nonfinite(s);
  }
  __syncthreads();

  uint32_t joins = 0;
  for (uint32_t t = 0; t + 1 < n; ++t) {
    const uint32_t m = n - t;
    // the pick: a wavefront per active row, all its rows into one tuple
    const double c = others(m);
    best p{pos_inf(), kNone};
    for (uint32_t i = wave; i + 1 < n; i += kBatchWaves)
      if (node[i] >= 0) p = scan_row<2, true>(n, i, lane, c, D, R, p);
    wave_best(p.q, p.k);
    if (lane == 0) { red_v[wave] = p.q; red_k[wave] = p.k; }
    __syncthreads();
    if (wave == 0) {
      double bq = lane < kBatchWaves ? red_v[lane] : pos_inf();
      uint32_t bk = lane < kBatchWaves ? red_k[lane] : kNone;
      wave_best(bq, bk);
      if (lane == 0) {
        const slots s = settle_pair(n, node, bk >> 16, bk & 0xFFFFu);  // kNone: a = 0xFFFF, above every n of this form
        pick[0] = s.a;
        pick[1] = s.b;
      }
    }
    __syncthreads();
    const uint32_t a = pick[0], b = pick[1];
    if (a == kNone) {  // cannot happen; the join is skipped by every thread alike and the count stays short
      if (tid == 0) head->fault = 1;
      continue;
    }
    const double dab = D[(size_t)a * n + b];
    written += update_row<kNjBatchThreads>(n, a, b, dab, D, R, node, row_u, row_part);
    if (tid == kNjBatchThreads - 1) written += join_pair(n, t, m, a, b, dab, R, node, left, right, length);  // a thread of the last wavefront
    __syncthreads();  // the new row a in LDS; R[a], R[b], node[a], node[b] still as before the join
    if (wave == 0) {
      const double s = row_sum(chunks, lane, row_u, row_part);
      if (lane == 0) {
        written += retire(n, t, a, b, s, R, node);
        ++joins;
      }
    }
    __syncthreads();
  }
  if (written) atomicAdd(&head->written, written);
  if (tid == 0) head->joins = joins;
}

}  // namespace

// tests: the looped form at small sizes (the results do not depend on it)
uint32_t nj_batch_max_n() { return (uint32_t)env_uint("DAFS_NJ_BATCH_MAX_N", 0, kNjBatchMaxN - 1, kNjBatchMaxN); }

int nj_batch_launch(uint32_t n, uint32_t count, const double* dist, void* workspace, int32_t* left, int32_t* right, double* length, bool batched,
                    hipStream_t st) {
  if (n < 2 || n > kNjMaxN || !count || !dist || !workspace || !left || !right || !length) return DAFS_HIP_EINVAL;
  if (batched && n > kNjBatchMaxN) return DAFS_HIP_EINVAL;
  uint8_t* w = (uint8_t*)workspace;
  nj_head* heads = (nj_head*)w;
  uint8_t* rest = w + nj_batch_heads_bytes(count);
  const size_t T = 2 * (size_t)n - 1;
  if (batched) {
    if (hip_check(hipMemsetAsync(heads, 0, (size_t)count * sizeof(nj_head), st))) return DAFS_HIP_ELAUNCH;
    STAGE_LAUNCH(ST_NJ_BATCH, st)
    hipLaunchKernelGGL(k_nj_batch, dim3(count), dim3(kNjBatchThreads), nj_batch_lds_bytes(n), st, n, dist, (double*)rest, nj_batch_copy_bytes(n) / 8,
                       heads, left, right, length);
    return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
  }
  for (uint32_t k = 0; k < count; ++k) {
    const int rc = nj_launch(n, dist + (size_t)k * n * n, rest, left + k * T, right + k * T, length + k * T, st);
    if (rc) return rc;
    if (hip_check(hipMemcpyAsync(heads + k, rest, sizeof(nj_head), hipMemcpyDeviceToDevice, st))) return DAFS_HIP_ELAUNCH;
  }
  return DAFS_HIP_OK;
}

int boot_pack(const boot_args& a, hipStream_t st) {
  if (!a.n || !a.U || !a.count || a.count > kBootChunkReplicates || a.words > 65535) return DAFS_HIP_EINVAL;
  STAGE_LAUNCH(ST_BOOT_PACK, st) hipLaunchKernelGGL(k_boot_pack, dim3((a.n + 255) / 256, a.words, a.count), dim3(256), 0, st, a);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int boot_dist(const boot_args& a, hipStream_t st) {
  if (a.n < 2 || a.n > kNjMaxN || !a.words || !a.chunk || a.chunk > kAliMaxChunk || !a.count || a.count > kBootChunkReplicates) return DAFS_HIP_EINVAL;
  const ali_tile_shape tile = ali_tile_shape_of(a.n, a.chunk);  // <= 2^10 x 2^8 blocks
  // so many replicates per launch that it stays below kAliBandBlocks workgroups of 1024 threads: under 2^32 work-items
  const uint32_t per = kAliBandBlocks / (tile.bi * tile.bj) ? kAliBandBlocks / (tile.bi * tile.bj) : 1;
  for (uint32_t kk = 0; kk < a.count; kk += per) {
    const uint32_t z = a.count - kk < per ? a.count - kk : per;
    STAGE_LAUNCH(ST_BOOT_DIST, st) hipLaunchKernelGGL(k_boot_dist, dim3(tile.bi, tile.bj, z), dim3(ALI_TILE_THREADS), tile.lds, st, a, kk);
    if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  }
  return DAFS_HIP_OK;
}

}  // namespace dafs

#undef ALI_TILE_COUNTS
