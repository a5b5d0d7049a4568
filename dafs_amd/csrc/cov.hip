// dafs_amd/csrc/cov.hip -- covariation statistics of an alignment's columns (dafs_hip_alignment_covariation, capi_cov.cpp;
// definitions in DESIGN.md section 13).
//
// The alignment is held as bit planes, one n-bit plane per column and base (cov.h).  The joint count n_ab of two columns is
// the population count of the AND of two planes, the G statistic Gq an exact int64 from a table of fixed-point logarithms.
// Everything that is added across threads is an integer (Gq into the column sums, the null's tail counters) or a maximum /
// minimum (the best partner), so the atomics and the tiling change no bit.
//
// k_cov_pairs: a workgroup of 16 wavefronts takes a tile of 16 columns c1 x 64 columns c2 of the upper triangle; wavefront v
// owns c1 = i0 + v, lane l owns c2 = j0 + l, so a lane owns one column pair and keeps its 16 counts in registers.  The planes
// of both column blocks are staged in LDS in chunks of `chunk` words (32 rows each): the c2 words word-major, so the lanes
// read consecutive banks, the c1 words a broadcast.
//
// A null alignment comes from k_cov_shuffle (every column permuted on its own) or from k_cov_fitch, once, and k_cov_draw +
// k_cov_evolve per alignment (the substitutions of every branch of a tree, moved to other columns); the pair passes do not
// care which.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dafs_hip.h"
#include "cov.h"
#include "hip_util.h"
#include "mix64.h"
#include "stage.h"

namespace dafs {

constexpr uint32_t TI = 16, TJ = 64;

// Gq of one column pair from its counts cnt[a * 4 + b]; *rows = m
__device__ __forceinline__ long long cov_gq(const uint32_t* cnt, const int64_t* __restrict__ lnq, uint32_t* rows) {
  uint32_t r[4], s[4], m = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    r[a] = cnt[a * 4] + cnt[a * 4 + 1] + cnt[a * 4 + 2] + cnt[a * 4 + 3];
    s[a] = cnt[a] + cnt[4 + a] + cnt[8 + a] + cnt[12 + a];
    m += r[a];
  }
  *rows = m;
  long long lr[4], ls[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) { lr[a] = lnq[r[a]]; ls[a] = lnq[s[a]]; }
  const long long lm = lnq[m];
  long long g = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t k = cnt[a * 4 + b];
      if (k) g += (long long)k * (lnq[k] + lm - lr[a] - ls[b]);
    }
  return 2 * g;
}

// S of one pair: the casts and operations of the definition, in its order
__device__ __forceinline__ double cov_score(long long g, long long r1, long long r2, long long t, double ratio) {
  double apc = 0.0;
  if (t != 0) apc = (double)r1 * (double)r2 / (double)t * ratio;
  return ((double)g - apc) / 65536.0;  // never -0.0: (double)g is not, so the difference is not
}

// order-preserving key of a finite double: a < b  <=>  key(a) < key(b); every key is above 0
__device__ __forceinline__ unsigned long long cov_key(double s) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

template <int PASS>
__global__ __launch_bounds__(1024) void k_cov_pairs(cov_args a, uint32_t j_block0) {
  extern __shared__ uint32_t lds[];  // y[chunk][4][TJ], then x[chunk][4][TI]
  __shared__ unsigned long long red_i[TI], red_j[TJ];
  const uint32_t i0 = blockIdx.x * TI, j0 = (j_block0 + blockIdx.y) * TJ;
  if (j0 + TJ - 1 <= i0) return;  // no pair c1 < c2 in this tile (the whole workgroup leaves)
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t c1 = i0 + wv, c2 = j0 + lane;
  uint32_t* ly = lds;
  uint32_t* lx = lds + (size_t)a.chunk * 4 * TJ;
  if (PASS == COV_SUMS || PASS == COV_BEST) {
    if (threadIdx.x < TI) red_i[threadIdx.x] = 0;
    if (threadIdx.x < TJ) red_j[threadIdx.x] = 0;
  }
  uint32_t cnt[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) cnt[k] = 0;
  for (uint32_t w0 = 0; w0 < a.words; w0 += a.chunk) {
    const uint32_t wc = a.words - w0 < a.chunk ? a.words - w0 : a.chunk;
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < wc * 4 * TJ; t += 1024) {
      const uint32_t col = j0 + (t & (TJ - 1)), pl = t / TJ;  // pl = w * 4 + base
      ly[t] = col < a.len ? a.planes[((size_t)w0 * 4 + pl) * a.len + col] : 0u;
    }
    for (uint32_t t = threadIdx.x; t < wc * 4 * TI; t += 1024) {
      const uint32_t col = i0 + (t & (TI - 1)), pl = t / TI;
      lx[t] = col < a.len ? a.planes[((size_t)w0 * 4 + pl) * a.len + col] : 0u;
    }
    __syncthreads();
    for (uint32_t w = 0; w < wc; ++w) {
      uint32_t x[4], y[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        x[b] = lx[(w * 4 + b) * TI + wv];
        y[b] = ly[(w * 4 + b) * TJ + lane];
      }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) cnt[p * 4 + q] += (uint32_t)__popc(x[p] & y[q]);
    }
  }
  const bool valid = c1 < c2 && c2 < a.len;
  long long g = 0;
  uint32_t rows;
  if (valid) g = cov_gq(cnt, a.lnq, &rows);

  if (PASS == COV_SUMS) {
    if (valid) {
      if (a.g) {
        a.g[(size_t)c1 * a.len + c2] = g;
        a.g[(size_t)c2 * a.len + c1] = g;
      }
      if (g) {
        atomicAdd(&red_i[wv], (unsigned long long)g);
        atomicAdd(&red_j[lane], (unsigned long long)g);
      }
    }
    __syncthreads();
    if (threadIdx.x < TI && i0 + threadIdx.x < a.len && red_i[threadIdx.x]) atomicAdd(&a.col_sum[i0 + threadIdx.x], red_i[threadIdx.x]);
    if (threadIdx.x >= 64 && threadIdx.x < 64 + TJ) {
      const uint32_t t = threadIdx.x - 64;
      if (j0 + t < a.len && red_j[t]) atomicAdd(&a.col_sum[j0 + t], red_j[t]);
    }
    return;
  }

  double s = 0.0;
  if (valid) s = cov_score(g, (long long)a.col_sum[c1], (long long)a.col_sum[c2], *a.total, a.ratio);
  if (PASS == COV_BEST) {
    if (valid) {
      const unsigned long long k = cov_key(s);
      atomicMax(&red_i[wv], k);
      atomicMax(&red_j[lane], k);
    }
    __syncthreads();
    if (threadIdx.x < TI && red_i[threadIdx.x]) atomicMax(&a.best_key[i0 + threadIdx.x], red_i[threadIdx.x]);
    if (threadIdx.x >= 64 && threadIdx.x < 64 + TJ) {
      const uint32_t t = threadIdx.x - 64;
      if (red_j[t]) atomicMax(&a.best_key[j0 + t], red_j[t]);  // a key was written for columns below len only
    }
  } else if (PASS == COV_ARG) {
    if (valid) {
      const unsigned long long k = cov_key(s);
      if (k == a.best_key[c1]) atomicMin(&a.best[c1], c2);
      if (k == a.best_key[c2]) atomicMin(&a.best[c2], c1);
    }
  } else {  // COV_NULL: the last candidate that s reaches counts it
    if (valid && s >= a.cand[0]) {
      uint32_t lo = 0, hi = a.ncand;  // cand[lo] <= s < cand[hi]
      while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.cand[mid] <= s) lo = mid; else hi = mid;
      }
      atomicAdd(&a.tail[(size_t)(lane & (a.copies - 1)) * a.ncand + lo], 1ull);
    }
  }
}

// one thread per (column, word): the four words of its 32 rows
__global__ __launch_bounds__(256) void k_cov_pack(const uint8_t* __restrict__ code, uint32_t n, uint32_t len, uint32_t* __restrict__ planes) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x, w = blockIdx.y;
  if (c >= len) return;
  uint32_t word[4] = {0u, 0u, 0u, 0u};
  const uint32_t r1 = n - w * 32 < 32 ? n - w * 32 : 32;
  for (uint32_t b = 0; b < r1; ++b) {
    const uint32_t v = code[(size_t)(w * 32 + b) * len + c];
#pragma unroll
    for (int q = 0; q < 4; ++q) word[q] |= (v == (uint32_t)q ? 1u : 0u) << b;
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) planes[((size_t)w * 4 + q) * len + c] = word[q];
}

// one thread per column: the Fisher-Yates of that column on the codes themselves (swapping p[i], p[j] swaps the codes at
// rows i and j).  The generator is counter-based: every draw depends on (base, c, i) alone.
__global__ __launch_bounds__(256) void k_cov_shuffle(const uint8_t* __restrict__ code, uint8_t* __restrict__ out, uint32_t n, uint32_t len,
                                                     uint64_t base) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= len) return;
  for (uint32_t r = 0; r < n; ++r) out[(size_t)r * len + c] = code[(size_t)r * len + c];
  for (uint32_t i = n - 1; i >= 1; --i) {
    const uint64_t u = mix64(base + (((uint64_t)c << 32) | i));
    const uint32_t j = (uint32_t)(((u >> 32) * (uint64_t)(i + 1)) >> 32);  // j <= i
    const uint8_t vi = out[(size_t)i * len + c], vj = out[(size_t)j * len + c];
    out[(size_t)i * len + c] = vj;
    out[(size_t)j * len + c] = vi;
  }
}

// ---- the null by evolution along a tree.  Both kernels keep one byte per (node, column) in a
// scratch laid out [node][column]: at every node the lanes of a wavefront touch 64 adjacent bytes, and a thread reads
// only cells of its own column, which it wrote itself.

// one thread per column: Fitch sets leaves-up, then states and change records root-down
__global__ __launch_bounds__(kCovTreeThreads) void k_cov_fitch(const uint8_t* __restrict__ code, const int32_t* __restrict__ left,
                                                               const int32_t* __restrict__ right, const int32_t* __restrict__ parent, uint32_t n,
                                                               uint32_t len, uint8_t* node, uint8_t* __restrict__ chg) {
  const uint32_t c = blockIdx.x * kCovTreeThreads + threadIdx.x;
  if (c >= len) return;
  const uint32_t root = 2 * n - 2;
  for (uint32_t r = 0; r < n; ++r) {
    const uint32_t v = code[(size_t)r * len + c];
    node[(size_t)r * len + c] = (uint8_t)(v < 4 ? 1u << v : 15u);
  }
  for (uint32_t v = n; v <= root; ++v) {
    const uint32_t a = node[(size_t)left[v] * len + c], b = node[(size_t)right[v] * len + c];
    node[(size_t)v * len + c] = (uint8_t)((a & b) ? (a & b) : (a | b));
  }
  // a set is never empty, so __ffs is at least 1; a state overwrites its node's set once the set has been read
  node[(size_t)root * len + c] = (uint8_t)(__ffs((int)node[(size_t)root * len + c]) - 1);
  chg[(size_t)root * len + c] = 0;
  for (uint32_t v = root; v-- > 0;) {
    const uint32_t p = node[(size_t)parent[v] * len + c], s = node[(size_t)v * len + c];
    const uint32_t state = ((s >> p) & 1u) ? p : (uint32_t)__ffs((int)s) - 1u;
    node[(size_t)v * len + c] = (uint8_t)state;
    chg[(size_t)v * len + c] = (uint8_t)(state == p ? 0u : 1u + 4u * p + state);
  }
}

// F: four Feistel rounds on the two h-bit halves of x, a bijection of [0, 4^h)
__device__ __forceinline__ uint32_t cov_feistel(uint64_t key, uint32_t h, uint32_t mask, uint32_t x) {
  uint32_t L = x >> h, R = x & mask;
#pragma unroll
  for (uint64_t r = 1; r <= 4; ++r) {
    const uint32_t t = L ^ ((uint32_t)mix64(key + kMixGolden * r + R) & mask);
    L = R;
    R = t;
  }
  return (L << h) | R;
}

// pi(key, len, c): F's cycle walked from c until it is back below len.  At most walk = 4^h - len + 1 applications get
// there, and that is the trip count: nothing here can spin.
__device__ __forceinline__ uint32_t cov_pi(uint64_t key, uint32_t len, uint32_t h, uint32_t walk, uint32_t c) {
  const uint32_t mask = (1u << h) - 1u;
  uint32_t x = cov_feistel(key, h, mask, c);
  for (uint32_t t = 1; t < walk && x >= len; ++t) x = cov_feistel(key, h, mask, x);
  return x < len ? x : c;  // always x: the index of a load stays inside the row whatever happens
}

// one thread per (branch, column) of one null alignment: the change record that branch v = v0 + blockIdx.y brings to
// column c, drawn by pi, into the branch's row of `node`.  Every draw depends on (base, v, c) alone, so the grid fills the
// device however short the alignment is; the root (no branch) keeps its row, state(root) from k_cov_fitch.
__global__ __launch_bounds__(kCovTreeThreads) void k_cov_draw(const uint8_t* __restrict__ chg, uint32_t len, uint32_t h, uint32_t walk,
                                                              uint64_t base, uint32_t v0, uint8_t* __restrict__ node) {
  const uint32_t c = blockIdx.x * kCovTreeThreads + threadIdx.x, v = v0 + blockIdx.y;
  if (c >= len) return;
  const uint64_t key = mix64(base ^ ((uint64_t)(v + 1) << 32));  // uniform per workgroup
  node[(size_t)v * len + c] = chg[(size_t)v * len + cov_pi(key, len, h, walk, c)];
}

// one thread per column, after k_cov_draw: root-down, the state of every node from its parent's and its drawn record.  The
// states of the joins (a leaf is nobody's parent) are the one chain of dependent reads: with LDS they live in the
// workgroup's LDS as [join][lane], else each takes the place of the join's record in `node` once that has been read.  A
// node's record and a leaf's own code do not depend on that chain and are fetched one node ahead.
template <bool LDS>
__global__ __launch_bounds__(kCovTreeThreads) void k_cov_evolve(const uint8_t* __restrict__ code, const int32_t* __restrict__ parent, uint32_t n,
                                                                uint32_t len, uint8_t* node, uint8_t* __restrict__ out) {
  extern __shared__ uint8_t ns_lds[];
  const uint32_t c = blockIdx.x * kCovTreeThreads + threadIdx.x;
  if (c >= len) return;
  const uint32_t root = 2 * n - 2;
  auto at = [&](uint32_t v) {  // the state of join v in this column (n <= v <= root)
    return LDS ? ns_lds + (size_t)(v - n) * kCovTreeThreads + threadIdx.x : node + (size_t)v * len + c;
  };
  if (LDS) *at(root) = node[(size_t)root * len + c];
  uint32_t rec_next = node[(size_t)(root - 1) * len + c], cell_next = root - 1 < n ? code[(size_t)(root - 1) * len + c] : 0u;  // n >= 2
  for (uint32_t v = root; v-- > 0;) {
    const uint32_t rec = rec_next, cell = cell_next;
    if (v) {
      rec_next = node[(size_t)(v - 1) * len + c];
      cell_next = v - 1 < n ? code[(size_t)(v - 1) * len + c] : 0u;
    }
    const uint32_t p = *at((uint32_t)parent[v]);  // a parent is a join
    uint32_t s = p;
    if (rec) {
      const uint32_t a = ((rec - 1) >> 2) & 3u, b = (rec - 1) & 3u;
      s = b != p ? b : a;
    }
    if (v >= n) *at(v) = (uint8_t)s;
    else out[(size_t)v * len + c] = cell == 4 ? (uint8_t)4 : (uint8_t)s;
  }
}

__global__ __launch_bounds__(1024) void k_cov_total(const unsigned long long* __restrict__ col_sum, uint32_t len, long long* total) {
  __shared__ unsigned long long acc;
  if (threadIdx.x == 0) acc = 0;
  __syncthreads();
  unsigned long long s = 0;
  for (uint32_t c = threadIdx.x; c < len; c += 1024) s += col_sum[c];
  if (s) atomicAdd(&acc, s);
  __syncthreads();
  if (threadIdx.x == 0) *total = (long long)acc;
}

// one thread per column: the consensus pair that starts there
__global__ __launch_bounds__(256) void k_cov_ss(cov_args a, cov_ss_args s) {
  const uint32_t c1 = blockIdx.x * 256 + threadIdx.x;
  if (c1 >= a.len) return;
  const uint32_t c2 = s.ss[c1];
  double score = 0.0;
  uint32_t rows = 0, canonical = 0, types = 0;
  if (c2 != DAFS_HIP_NONE) {
    uint32_t cnt[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) cnt[k] = 0;
    for (uint32_t w = 0; w < a.words; ++w) {
      uint32_t x[4], y[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        x[b] = a.planes[((size_t)w * 4 + b) * a.len + c1];
        y[b] = a.planes[((size_t)w * 4 + b) * a.len + c2];
      }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) cnt[p * 4 + q] += (uint32_t)__popc(x[p] & y[q]);
    }
    const long long g = cov_gq(cnt, a.lnq, &rows);
    score = cov_score(g, (long long)a.col_sum[c1], (long long)a.col_sum[c2], *a.total, a.ratio);
    const uint32_t six[6] = {cnt[0 * 4 + 3], cnt[3 * 4 + 0], cnt[2 * 4 + 1], cnt[1 * 4 + 2], cnt[2 * 4 + 3], cnt[3 * 4 + 2]};  // AU UA GC CG GU UG
#pragma unroll
    for (int k = 0; k < 6; ++k) { canonical += six[k]; types += six[k] ? 1u : 0u; }
  }
  s.score[c1] = score;
  s.rows[c1] = rows;
  s.canonical[c1] = canonical;
  s.types[c1] = types;
}

int cov_pack(const uint8_t* code, uint32_t n, uint32_t len, uint32_t* planes, hipStream_t st) {
  const uint32_t words = (n + 31) / 32;
  for (uint32_t w0 = 0; w0 < words; w0 += 65535) {  // grid.y holds 65535 at most
    const uint32_t wn = words - w0 < 65535 ? words - w0 : 65535;
    STAGE_LAUNCH(ST_COV_PACK, st)
    hipLaunchKernelGGL(k_cov_pack, dim3((len + 255) / 256, wn), dim3(256), 0, st, code + (size_t)w0 * 32 * len, n - w0 * 32, len,
                       planes + (size_t)w0 * 4 * len);
    if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  }
  return DAFS_HIP_OK;
}

int cov_shuffle(const uint8_t* code, uint8_t* out, uint32_t n, uint32_t len, uint64_t base, hipStream_t st) {
  STAGE_LAUNCH(ST_COV_SHUFFLE, st) hipLaunchKernelGGL(k_cov_shuffle, dim3((len + 255) / 256), dim3(256), 0, st, code, out, n, len, base);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int cov_fitch(const uint8_t* code, const cov_tree& t, uint32_t n, uint32_t len, uint8_t* node, uint8_t* chg, hipStream_t st) {
  STAGE_LAUNCH(ST_COV_FITCH, st)
  hipLaunchKernelGGL(k_cov_fitch, dim3((len + kCovTreeThreads - 1) / kCovTreeThreads), dim3(kCovTreeThreads), 0, st, code, t.left, t.right,
                     t.parent, n, len, node, chg);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int cov_evolve(const uint8_t* code, const uint8_t* chg, const cov_tree& t, uint32_t n, uint32_t len, uint64_t base, uint8_t* node,
               uint8_t* out, bool lds, hipStream_t st) {
  if (n < 2 || (lds && !cov_evolve_fits_lds(n))) return DAFS_HIP_EINVAL;
  uint32_t h = 1;
  while (((uint64_t)1 << (2 * h)) < len) ++h;
  const uint32_t walk = (uint32_t)(((uint64_t)1 << (2 * h)) - len + 1), cols = (len + kCovTreeThreads - 1) / kCovTreeThreads;
  for (uint32_t v0 = 0; v0 < 2 * n - 2; v0 += 65535) {  // grid.y holds 65535 at most
    const uint32_t vn = 2 * n - 2 - v0 < 65535 ? 2 * n - 2 - v0 : 65535;
    STAGE_LAUNCH(ST_COV_DRAW, st) hipLaunchKernelGGL(k_cov_draw, dim3(cols, vn), dim3(kCovTreeThreads), 0, st, chg, len, h, walk, base, v0, node);
    if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  }
  STAGE_LAUNCH(ST_COV_EVOLVE, st) {
    if (lds)
      hipLaunchKernelGGL(k_cov_evolve<true>, dim3(cols), dim3(kCovTreeThreads), (size_t)(n - 1) * kCovTreeThreads, st, code, t.parent, n, len, node,
                         out);
    else
      hipLaunchKernelGGL(k_cov_evolve<false>, dim3(cols), dim3(kCovTreeThreads), 0, st, code, t.parent, n, len, node, out);
  }
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int cov_pairs(cov_pass pass, const cov_args& a, hipStream_t st) {
  if (a.len < 2 || !a.chunk || a.chunk > kCovMaxChunk) return DAFS_HIP_EINVAL;
  const uint32_t bi = (a.len + TI - 1) / TI, bj = (a.len + TJ - 1) / TJ;
  const size_t lds = (size_t)a.chunk * 4 * (TI + TJ) * sizeof(uint32_t);
  static const int ids[4] = {ST_COV_SUMS, ST_COV_BEST, ST_COV_ARG, ST_COV_NULL};
  for (uint32_t j = 0; j < bj; j += 65535) {
    const dim3 grid(bi, bj - j < 65535 ? bj - j : 65535);
    STAGE_LAUNCH(ids[pass], st) switch (pass) {
      case COV_SUMS: hipLaunchKernelGGL(k_cov_pairs<COV_SUMS>, grid, dim3(1024), lds, st, a, j); break;
      case COV_BEST: hipLaunchKernelGGL(k_cov_pairs<COV_BEST>, grid, dim3(1024), lds, st, a, j); break;
      case COV_ARG: hipLaunchKernelGGL(k_cov_pairs<COV_ARG>, grid, dim3(1024), lds, st, a, j); break;
      default: hipLaunchKernelGGL(k_cov_pairs<COV_NULL>, grid, dim3(1024), lds, st, a, j); break;
    }
    if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  }
  return DAFS_HIP_OK;
}

int cov_total(const unsigned long long* col_sum, uint32_t len, long long* total, hipStream_t st) {
  STAGE_LAUNCH(ST_COV_TOTAL, st) hipLaunchKernelGGL(k_cov_total, dim3(1), dim3(1024), 0, st, col_sum, len, total);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int cov_ss(const cov_args& a, const cov_ss_args& s, hipStream_t st) {
  STAGE_LAUNCH(ST_COV_SS, st) hipLaunchKernelGGL(k_cov_ss, dim3((a.len + 255) / 256), dim3(256), 0, st, a, s);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

}  // namespace dafs
