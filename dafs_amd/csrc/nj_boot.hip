// dafs_amd/csrc/nj_boot.hip -- the bootstrap of the neighbour-joining tree on the device (the reference
// has no counterpart, tests/bootstrap_ref.py is the plain restatement).
//
// k_boot_pack  one thread per (replicate, row, word of 64 columns): the draws of its 64 positions (stateless: a draw is one
//              mix of the replicate's base and the position, so no draw is ever stored), the row's cells in the drawn
//              columns, and the four plane words of alistat.h, word-major per replicate.
// k_boot_dist  the tile of k_ali_pairs<ALI_MATRIX> (alistat.hip) with a grid dimension over the replicates: 16 wavefronts,
//              16 rows r x 64 rows s, the plane words staged in LDS, the counters in registers.  The lane that owns r < s
//              turns its two counts into the distance of section 22 and writes that one double; the count matrices are
//              never stored.  A Jukes-Cantor value that comes within `guard` of a quantisation step goes to a list that the
//              host recomputes with its own log().
// k_nj_batch   ONE workgroup per matrix: all n - 1 joins of section 22 inside it, in the style of k_linkage_joins.  Every wait
//              is a __syncthreads(), the loop has exactly n - 1 trips, nothing polls and no workgroup knows of another.  D is
//              the matrix's working copy in global memory; R, node, the wavefronts' pick tuples and the row of the join
//              are in LDS.  The pick, the update and the running sum R[a] are those of nj.hip, restated here so that nj.hip's
//              code objects stay as they are: a wavefront per active row i scans j > i with strict `<`, rows and columns
//              ascending, so a lane keeps the first smallest (i, j) it met; one butterfly over (Q, i << 16 | j) per wavefront
//              and one over the 16 wavefronts leave the smallest Q, then the smallest a, then the smallest b.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/dafs_hip.h"
#include "alistat.h"
#include "call_host.h"
#include "hip_util.h"
#include "nj_boot.h"
#include "stage.h"

namespace dafs {

namespace {

constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kBatchWaves = kNjBatchThreads / 64;
constexpr uint32_t TI = 16, TJ = 64;

__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7FF0000000000000ll); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ uint32_t nonfinite(double v) {
  return ((unsigned long long)__double_as_longlong(v) & 0x7FF0000000000000ull) == 0x7FF0000000000000ull ? 1u : 0u;
}

// (value ascending, key ascending); a NaN is never better, and (+inf, kNone) is "no candidate"
__device__ __forceinline__ bool better(double v1, uint32_t i1, double v2, uint32_t i2) { return v1 < v2 || (v1 == v2 && i1 < i2); }

__device__ __forceinline__ void wave_best(double& v, uint32_t& i) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const double ov = __shfl_xor(v, d, 64);
    const uint32_t oi = __shfl_xor(i, d, 64);
    if (better(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

__device__ __forceinline__ double lane_value(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// mix of DESIGN.md section 13
__device__ __forceinline__ uint64_t boot_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__global__ __launch_bounds__(256) void k_boot_pack(boot_args a) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x, w = blockIdx.y, kk = blockIdx.z;
  if (r >= a.n) return;
  const uint64_t base = boot_mix(a.seed + kGolden * (uint64_t)(a.k0 + kk + 1));
  uint64_t word[4] = {0ull, 0ull, 0ull, 0ull};
  const uint32_t c1 = a.U - w * 64 < 64 ? a.U - w * 64 : 64;
  for (uint32_t b = 0; b < c1; ++b) {
    const uint32_t u = (uint32_t)(((boot_mix(base + (uint64_t)(w * 64 + b)) >> 32) * (uint64_t)a.U) >> 32);  // below U
    const uint64_t v = a.cells[(size_t)u * a.n + r];
    word[ALI_LO] |= (v & 1) << b;
    word[ALI_HI] |= ((v >> 1) & 1) << b;
    word[ALI_BASE] |= (uint64_t)(v <= 3 ? 1 : 0) << b;
    word[ALI_RES] |= (uint64_t)(v <= 4 ? 1 : 0) << b;
  }
  uint64_t* planes = a.planes + (size_t)kk * a.words * 4 * a.n;
#pragma unroll
  for (int p = 0; p < 4; ++p) planes[((size_t)w * 4 + p) * a.n + r] = word[p];
}

__global__ __launch_bounds__(1024) void k_boot_dist(boot_args a, uint32_t kk0) {
  extern __shared__ uint64_t lds[];  // y[chunk][4][TJ], then x[chunk][4][TI]
  const uint32_t i0 = blockIdx.x * TI, j0 = blockIdx.y * TJ, kk = kk0 + blockIdx.z;
  if (j0 + TJ - 1 <= i0) return;  // no pair r < s in this tile (the whole workgroup leaves)
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t r = i0 + wv, s = j0 + lane;
  const uint64_t* planes = a.planes + (size_t)kk * a.words * 4 * a.n;
  uint64_t* ly = lds;
  uint64_t* lx = lds + (size_t)a.chunk * 4 * TJ;
  uint32_t ident = 0, comp = 0;
  for (uint32_t w0 = 0; w0 < a.words; w0 += a.chunk) {
    const uint32_t wc = a.words - w0 < a.chunk ? a.words - w0 : a.chunk;
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < wc * 4 * TJ; t += 1024) {
      const uint32_t row = j0 + (t & (TJ - 1)), pl = t / TJ;  // pl = w * 4 + plane
      ly[t] = row < a.n ? planes[((size_t)w0 * 4 + pl) * a.n + row] : 0ull;
    }
    for (uint32_t t = threadIdx.x; t < wc * 4 * TI; t += 1024) {
      const uint32_t row = i0 + (t & (TI - 1)), pl = t / TI;
      lx[t] = row < a.n ? planes[((size_t)w0 * 4 + pl) * a.n + row] : 0ull;
    }
    __syncthreads();
    for (uint32_t w = 0; w < wc; ++w) {
      uint64_t x[4], y[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        x[p] = lx[(w * 4 + p) * TI + wv];
        y[p] = ly[(w * 4 + p) * TJ + lane];
      }
      ident += (uint32_t)__popcll(~(x[ALI_LO] ^ y[ALI_LO]) & ~(x[ALI_HI] ^ y[ALI_HI]) & x[ALI_BASE] & y[ALI_BASE]);
      comp += (uint32_t)__popcll(x[ALI_RES] & y[ALI_RES]);
    }
  }
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
  for (uint32_t row = wave; row < n; row += kBatchWaves) {
    double* out = D + (size_t)row * n;
    for (uint32_t j = lane; j < n; j += 64) {
      double v = 0.0;
      if (j > row) {
        v = in[(size_t)row * n + j];
        bad += nonfinite(v);
      } else if (j < row) {
        v = in[(size_t)j * n + row];
      }
      out[j] = v;
    }
  }
  for (uint32_t i = tid; i < n; i += kNjBatchThreads) {
    node[i] = (int32_t)i;
    left[i] = -1;
    right[i] = -1;
    length[i] = 0.0;
    if (i + 1 < n) length[n + i] = 0.0;  // the root's stays
  }
  if (bad) atomicAdd(&bad_in, bad);
  __syncthreads();
  if (bad_in) {  // refused: no join runs (the whole workgroup leaves)
    if (tid == 0) head->nonfinite = bad_in;
    return;
  }
  // R[k]: the running sum of column k in ascending row order (k_nj_rowsum)
  uint32_t written = 0;
  for (uint32_t k = tid; k < n; k += kNjBatchThreads) {
    double s = 0.0;
#pragma unroll 8
    for (uint32_t j = 0; j < n; ++j) s += D[(size_t)j * n + k];
    R[k] = s;
    written += nonfinite(s);
  }
  __syncthreads();

  uint32_t joins = 0;
  for (uint32_t t = 0; t + 1 < n; ++t) {
    const uint32_t m = n - t;
    // the pick: a wavefront per active row
    {
      const double c = (double)(m - 2);
      double bq = pos_inf();
      uint32_t bk = kNone;
      for (uint32_t i = wave; i + 1 < n; i += kBatchWaves) {
        if (node[i] < 0) continue;
        const double* Di = D + (size_t)i * n;
        const double Ri = R[i];
#pragma unroll 2
        for (uint32_t j = i + 1 + lane; j < n; j += 64) {
          const double q = (c * Di[j] - Ri) - R[j];  // NaN at a retired j: never below anything
          if (q < bq) { bq = q; bk = (i << 16) | j; }
        }
      }
      wave_best(bq, bk);
      if (lane == 0) { red_v[wave] = bq; red_k[wave] = bk; }
    }
    __syncthreads();
    if (wave == 0) {
      double bq = lane < kBatchWaves ? red_v[lane] : pos_inf();
      uint32_t bk = lane < kBatchWaves ? red_k[lane] : kNone;
      wave_best(bq, bk);
      if (lane == 0) {
        uint32_t a = kNone, b = kNone;
        if (bk != kNone) {
          a = bk >> 16;
          b = bk & 0xFFFFu;
        } else {  // no Q below +inf: the candidate the scan starts from, the first two active slots
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
    if (a == kNone) {  // cannot happen; the join is skipped by every thread alike and the count stays short
      if (tid == 0) head->fault = 1;
      continue;
    }
    double* Da = D + (size_t)a * n;
    const double* Db = D + (size_t)b * n;
    const double dab = Da[b];
    for (uint32_t base = wave * 64; base < n; base += kNjBatchThreads) {  // a wavefront takes whole chunks of 64 slots
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
        written += nonfinite(u) + nonfinite(r);
      }
      row_u[k] = u;
      const unsigned long long m_part = __ballot(part);
      if (lane == 0) row_part[base >> 6] = m_part;
    }
    if (tid == kNjBatchThreads - 1) {  // the join itself, by a thread of the last wavefront
      double la = 0.5 * dab;
      if (m > 2) la = la + (R[a] - R[b]) / (2.0 * (double)(m - 2));
      const double lb = dab - la;
      const int32_t na = node[a], nb = node[b];
      length[na] = la;
      length[nb] = lb;
      left[n + t] = na;
      right[n + t] = nb;
      written += nonfinite(la) + nonfinite(lb);
    }
    __syncthreads();  // the new row a in LDS; R[a], R[b], node[a], node[b] still as before the join
    if (wave == 0) {
      // R[a]: the running sum of the new row a over the remaining active k, ascending (see k_nj_update)
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
        written += nonfinite(s);
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
  const uint32_t bi = (a.n + TI - 1) / TI, bj = (a.n + TJ - 1) / TJ;  // <= 2^10 x 2^8
  const size_t lds = (size_t)a.chunk * 4 * (TI + TJ) * sizeof(uint64_t);
  // so many replicates per launch that it stays below kAliBandBlocks workgroups of 1024 threads: under 2^32 work-items
  const uint32_t per = kAliBandBlocks / (bi * bj) ? kAliBandBlocks / (bi * bj) : 1;
  for (uint32_t kk = 0; kk < a.count; kk += per) {
    const uint32_t z = a.count - kk < per ? a.count - kk : per;
    STAGE_LAUNCH(ST_BOOT_DIST, st) hipLaunchKernelGGL(k_boot_dist, dim3(bi, bj, z), dim3(1024), lds, st, a, kk);
    if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  }
  return DAFS_HIP_OK;
}

}  // namespace dafs
