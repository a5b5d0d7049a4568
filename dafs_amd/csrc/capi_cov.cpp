// dafs_amd/csrc/capi_cov.cpp -- dafs_hip_alignment_covariation: how far the sequences of an alignment support its column pairs
// (cov.hip; definitions in DESIGN.md section 13).  The reference has no counterpart.  The call reads the alignment's codes and
// the structure alone, none of the context's stores, so it annotates any alignment.
//
// Host work: the checks, the table of fixed-point logarithms, the order of the passes, the sorted candidate scores of the
// null and the suffix sum that turns its bucket counters into tails.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <limits>
#include <vector>

#include "../../include/dafs_hip.h"
#include "cov.h"
#include "ctx.h"
#include "hip_util.h"

using namespace dafs;

namespace {

uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

double key_to_double(unsigned long long k) {  // inverse of cov_key (cov.hip)
  const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  double d;
  memcpy(&d, &b, 8);
  return d;
}

struct dev_mem {  // the Gq matrix of one call: not kept in the context
  void* p = nullptr;
  ~dev_mem() { if (p) (void)hipFree(p); }
};

// Every return waits for the stream: the queued copies and kernels read and write the caller's buffers and this call's
// vectors, which must not die under them when an error ends the call early.
struct stream_drain {
  hipStream_t st;
  ~stream_drain() { (void)hipStreamSynchronize(st); }
};

}  // namespace

extern "C" int dafs_hip_alignment_covariation(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint8_t* code, const uint32_t* ss,
                                              uint32_t shuffles, uint64_t seed, int64_t* col_sum, uint32_t* best, double* best_score,
                                              double* best_e, double* pair_score, double* pair_e, uint32_t* pair_rows,
                                              uint32_t* pair_canonical, uint32_t* pair_types, int64_t* total, int64_t* g) {
  if (!c || !n || !len || !code) return DAFS_HIP_EINVAL;
  if (n > (1u << 20) || (double)n * (double)len * (double)len > 35184372088832.0) return DAFS_HIP_EINVAL;  // 2^45: T fits an int64
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  for (size_t k = 0; k < (size_t)n * len; ++k)
    if (code[k] > 4) return DAFS_HIP_EINVAL;
  std::vector<uint32_t> lefts;
  if (ss) {  // left column -> right column, each column in at most one pair (as dafs_hip_alignment_reliability)
    std::vector<uint8_t> used(len, 0);
    for (uint32_t col = 0; col < len; ++col) {
      const uint32_t p = ss[col];
      if (p == DAFS_HIP_NONE) continue;
      if (p <= col || p >= len || used[col] || used[p]) return DAFS_HIP_EINVAL;
      used[col] = used[p] = 1;
      lefts.push_back(col);
    }
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  const double e0 = shuffles ? 0.0 : nan;
  // everything 0, no partners, E = 0 (NaN without shuffles); the statistics overwrite it below
  if (col_sum) std::fill(col_sum, col_sum + len, (int64_t)0);
  if (best) std::fill(best, best + len, DAFS_HIP_NONE);
  if (best_score) std::fill(best_score, best_score + len, 0.0);
  if (best_e) std::fill(best_e, best_e + len, e0);
  if (pair_score) std::fill(pair_score, pair_score + len, 0.0);
  if (pair_e) {
    std::fill(pair_e, pair_e + len, 0.0);
    for (uint32_t l : lefts) pair_e[l] = e0;
  }
  if (pair_rows) std::fill(pair_rows, pair_rows + len, 0u);
  if (pair_canonical) std::fill(pair_canonical, pair_canonical + len, 0u);
  if (pair_types) std::fill(pair_types, pair_types + len, 0u);
  if (total) *total = 0;
  if (g) std::fill(g, g + (size_t)len * len, (int64_t)0);
  if (len < 2 || n < 2) return DAFS_HIP_OK;  // no launch

  std::vector<int64_t> lnq((size_t)n + 1, 0);
  for (uint32_t k = 1; k <= n; ++k) lnq[k] = (int64_t)floor(log((double)k) * 65536 + 0.5);
  const uint32_t words = (n + 31) / 32;
  uint32_t chunk = std::min(words, kCovMaxChunk);
  if (const char* e = getenv("DAFS_COV_CHUNK_WORDS")) {  // tests: a smaller LDS stage (the results do not depend on it)
    const long v = strtol(e, nullptr, 10);
    if (v >= 1 && v <= (long)kCovMaxChunk) chunk = std::min(words, (uint32_t)v);
  }
  const uint32_t ncand = len + (uint32_t)lefts.size();
  uint32_t copies = 64;
  while (copies > 1 && (size_t)copies * ncand * 8 > ((size_t)64 << 20)) copies /= 2;

  // device workspace, carved from c->work
  size_t used = 0;
  auto take = [&](size_t bytes) { const size_t at = used; used += (bytes + 255) & ~(size_t)255; return at; };
  const size_t o_code = take((size_t)n * len), o_shuf = take(shuffles ? (size_t)n * len : 0), o_planes = take((size_t)words * 4 * len * 4);
  const size_t o_lnq = take(((size_t)n + 1) * 8), o_sum = take((size_t)len * 8), o_tot = take(8), o_key = take((size_t)len * 8);
  const size_t o_best = take((size_t)len * 4), o_ss = take((size_t)len * 4), o_ps = take((size_t)len * 8), o_pr = take((size_t)len * 4 * 3);
  const size_t o_cand = take((size_t)ncand * 8), o_tail = take(shuffles ? (size_t)copies * ncand * 8 : 0);
  int rc;
  if ((rc = c->work.reserve(used + 256))) return rc;
  uint8_t* w = c->work.ptr;
  dev_mem gm;
  if (g && hip_check(hipMalloc(&gm.p, (size_t)len * len * 8))) return DAFS_HIP_ENOMEM;
  hipStream_t st = c->stream;
  std::vector<unsigned long long> key(len), tail(shuffles ? (size_t)copies * ncand : 0);
  std::vector<double> bs(len), ps(len, 0.0), cand;
  int64_t tot = 0;
  stream_drain drain{st};  // declared after every host buffer the stream touches, so it waits before they go
  auto up = [&](size_t off, const void* src, size_t bytes) { return bytes && hip_check(hipMemcpyAsync(w + off, src, bytes, hipMemcpyHostToDevice, st)); };
  auto down = [&](void* dst, size_t off, size_t bytes) { return hip_check(hipMemcpyAsync(dst, w + off, bytes, hipMemcpyDeviceToHost, st)); };
  auto zero = [&](size_t off, int v, size_t bytes) { return hip_check(hipMemsetAsync(w + off, v, bytes, st)); };

  cov_args a;
  memset(&a, 0, sizeof a);
  a.planes = (const uint32_t*)(w + o_planes);
  a.lnq = (const int64_t*)(w + o_lnq);
  a.col_sum = (unsigned long long*)(w + o_sum);
  a.total = (const long long*)(w + o_tot);
  a.g = (long long*)gm.p;
  a.best_key = (unsigned long long*)(w + o_key);
  a.best = (uint32_t*)(w + o_best);
  a.cand = (const double*)(w + o_cand);
  a.tail = (unsigned long long*)(w + o_tail);
  a.ratio = (double)len / (double)(len - 1);
  a.n = n; a.len = len; a.words = words; a.chunk = chunk; a.ncand = ncand; a.copies = copies;
  cov_ss_args sa;
  sa.ss = (const uint32_t*)(w + o_ss);
  sa.score = (double*)(w + o_ps);
  sa.rows = (uint32_t*)(w + o_pr);
  sa.canonical = sa.rows + len;
  sa.types = sa.canonical + len;

  // the alignment itself: column sums, total, best partners, consensus pairs
  if (up(o_code, code, (size_t)n * len) || up(o_lnq, lnq.data(), lnq.size() * 8) || (ss && up(o_ss, ss, (size_t)len * 4))) return DAFS_HIP_ELAUNCH;
  if (zero(o_sum, 0, (size_t)len * 8) || zero(o_key, 0, (size_t)len * 8) || zero(o_best, 0xFF, (size_t)len * 4)) return DAFS_HIP_ELAUNCH;
  if (gm.p && hip_check(hipMemsetAsync(gm.p, 0, (size_t)len * len * 8, st))) return DAFS_HIP_ELAUNCH;
  if ((rc = cov_pack(w + o_code, n, len, (uint32_t*)(w + o_planes), st))) return rc;
  if ((rc = cov_pairs(COV_SUMS, a, st))) return rc;
  if ((rc = cov_total(a.col_sum, len, (long long*)(w + o_tot), st))) return rc;
  if ((rc = cov_pairs(COV_BEST, a, st))) return rc;
  if ((rc = cov_pairs(COV_ARG, a, st))) return rc;
  if (ss && (rc = cov_ss(a, sa, st))) return rc;
  if (down(key.data(), o_key, (size_t)len * 8) || down(&tot, o_tot, 8)) return DAFS_HIP_ELAUNCH;
  if (ss && down(ps.data(), o_ps, (size_t)len * 8)) return DAFS_HIP_ELAUNCH;
  if (col_sum && down(col_sum, o_sum, (size_t)len * 8)) return DAFS_HIP_ELAUNCH;
  if (best && down(best, o_best, (size_t)len * 4)) return DAFS_HIP_ELAUNCH;
  if (ss && pair_rows && down(pair_rows, o_pr, (size_t)len * 4)) return DAFS_HIP_ELAUNCH;
  if (ss && pair_canonical && down(pair_canonical, o_pr + (size_t)len * 4, (size_t)len * 4)) return DAFS_HIP_ELAUNCH;
  if (ss && pair_types && down(pair_types, o_pr + (size_t)len * 8, (size_t)len * 4)) return DAFS_HIP_ELAUNCH;
  if (g && hip_check(hipMemcpyAsync(g, gm.p, (size_t)len * len * 8, hipMemcpyDeviceToHost, st))) return DAFS_HIP_ELAUNCH;
  if (hip_check(hipStreamSynchronize(st))) return DAFS_HIP_ELAUNCH;
  for (uint32_t col = 0; col < len; ++col) bs[col] = key_to_double(key[col]);  // len >= 2: every column has a partner
  if (best_score) std::copy(bs.begin(), bs.end(), best_score);
  if (pair_score) std::copy(ps.begin(), ps.end(), pair_score);
  if (total) *total = tot;
  if (!shuffles || (!best_e && !pair_e)) return DAFS_HIP_OK;

  // the null: per shuffle its own column sums and total, then every score that reaches the smallest candidate is counted
  // at the last candidate it reaches; a suffix sum gives the tails
  cand = bs;
  for (uint32_t l : lefts) cand.push_back(ps[l]);
  std::sort(cand.begin(), cand.end());
  if (up(o_cand, cand.data(), (size_t)ncand * 8) || zero(o_tail, 0, (size_t)copies * ncand * 8)) return DAFS_HIP_ELAUNCH;
  for (uint32_t k = 0; k < shuffles; ++k) {
    const uint64_t base = mix64(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)k + 1));
    if ((rc = cov_shuffle(w + o_code, w + o_shuf, n, len, base, st))) return rc;
    if ((rc = cov_pack(w + o_shuf, n, len, (uint32_t*)(w + o_planes), st))) return rc;
    if (zero(o_sum, 0, (size_t)len * 8)) return DAFS_HIP_ELAUNCH;
    cov_args b = a;
    b.g = nullptr;
    if ((rc = cov_pairs(COV_SUMS, b, st))) return rc;
    if ((rc = cov_total(b.col_sum, len, (long long*)(w + o_tot), st))) return rc;
    if ((rc = cov_pairs(COV_NULL, b, st))) return rc;
  }
  if (down(tail.data(), o_tail, tail.size() * 8)) return DAFS_HIP_ELAUNCH;
  if (hip_check(hipStreamSynchronize(st))) return DAFS_HIP_ELAUNCH;
  std::vector<unsigned long long> reach(ncand + 1, 0);  // reach[i]: null scores >= cand[i]
  for (uint32_t i = ncand; i-- > 0;) {
    unsigned long long s = 0;
    for (uint32_t q = 0; q < copies; ++q) s += tail[(size_t)q * ncand + i];
    reach[i] = reach[i + 1] + s;
  }
  auto e_of = [&](double s) {
    const size_t i = (size_t)(std::lower_bound(cand.begin(), cand.end(), s) - cand.begin());  // the first candidate equal to s
    return (double)reach[i] / (double)shuffles;
  };
  if (best_e)
    for (uint32_t col = 0; col < len; ++col) best_e[col] = e_of(bs[col]);
  if (pair_e)
    for (uint32_t l : lefts) pair_e[l] = e_of(ps[l]);
  return DAFS_HIP_OK;
}
