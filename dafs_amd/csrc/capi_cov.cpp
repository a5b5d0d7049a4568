// dafs_amd/csrc/capi_cov.cpp -- dafs_hip_alignment_covariation[_null]: how far the sequences of an alignment support its column
// pairs (cov.hip; definitions in DESIGN.md section 13), and dafs_hip_covariation_null_alignment: one alignment of its null.  The
// reference has no counterpart.  The calls read the alignment's codes and the structure alone, none of the context's stores, so
// they annotate any alignment.
//
// Host work: the checks, the table of fixed-point logarithms, the order of the passes, the sorted candidate scores of the
// null and the suffix sum that turns its bucket counters into tails; for the tree null the checks of the caller's tree and its
// parents, or the default tree: the identity matrices of dafs_hip_alignment_identity, divided on the host, joined by
// dafs_hip_linkage_tree under the average rule (both through host memory, so n <= 32768 there).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <limits>
#include <vector>

#include "../../include/dafs_hip.h"
#include "call_frame.h"
#include "call_host.h"
#include "cov.h"

using namespace dafs;

namespace {

double key_to_double(unsigned long long k) {  // inverse of cov_key (cov.hip)
  const unsigned long long b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  double d;
  memcpy(&d, &b, 8);
  return d;
}

// what the arguments say about the null, before anything is read through them
int null_args_check(int null, const int32_t* tree_left, const int32_t* tree_right) {
  if (null != DAFS_COV_NULL_SHUFFLE && null != DAFS_COV_NULL_TREE) return refuse("covariation: unknown null");
  if (null == DAFS_COV_NULL_SHUFFLE && (tree_left || tree_right)) return refuse("covariation: the shuffle null takes no tree");
  if (!tree_left != !tree_right) return refuse("covariation: a tree needs both of its arrays");
  return DAFS_HIP_OK;
}

// tree = left, right, parent of the 2n-1 nodes, one after the other.  The caller's arrays pass the checks of
// dafs_host_cluster_cut; without them it is the default tree of DESIGN.md section 13.
int tree_of(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint8_t* code, const int32_t* tree_left, const int32_t* tree_right,
            std::vector<int32_t>& tree) {
  const size_t T = 2 * (size_t)n - 1;
  tree.assign(3 * T, -1);
  int32_t *left = tree.data(), *right = left + T, *parent = right + T;
  if (tree_left) {
    std::copy(tree_left, tree_left + T, left);
    std::copy(tree_right, tree_right + T, right);
  } else {
    if (n > 32768) return refuse("covariation: the default tree takes at most 32768 rows (pass a tree)");
    std::vector<uint8_t> cell((size_t)n * len);
    for (uint32_t r = 0; r < n; ++r) {
      bool any = false;
      for (uint32_t col = 0; col < len; ++col) {
        const uint8_t v = code[(size_t)r * len + col];
        cell[(size_t)r * len + col] = v == 4 ? 5 : v;  // the gap code of dafs_hip_alignment_identity: matches and aligns with nothing
        any = any || v < 4;
      }
      if (!any) return refuse("covariation: the default tree needs a base in every row");
    }
    std::vector<uint32_t> ident((size_t)n * n), both((size_t)n * n);
    int rc = dafs_hip_alignment_identity(c, n, len, cell.data(), nullptr, nullptr, 0.0, nullptr, ident.data(), both.data(), nullptr, nullptr,
                                         nullptr, nullptr);
    if (rc) return rc;
    std::vector<float> sim((size_t)n * n, 0.0f), score(T);
    for (uint32_t r = 0; r < n; ++r)
      for (uint32_t s = r + 1; s < n; ++s) {
        const size_t at = (size_t)r * n + s;
        sim[at] = both[at] ? (float)((double)ident[at] / (double)both[at]) : 0.0f;
      }
    if ((rc = dafs_hip_linkage_tree(c, DAFS_LINKAGE_AVERAGE, n, sim.data(), score.data(), left, right))) return rc;
  }
  for (size_t i = 0; i < T; ++i) {
    if (i < n) {
      if (left[i] != -1 || right[i] != -1) return refuse("covariation: malformed tree (a leaf with a child)");
      continue;
    }
    if (left[i] == right[i]) return refuse("covariation: malformed tree (a join of a node with itself)");
    for (const int64_t ch : {(int64_t)left[i], (int64_t)right[i]}) {
      if (ch < 0 || ch >= (int64_t)i) return refuse("covariation: malformed tree (a child that is not an earlier node)");
      if (parent[ch] != -1) return refuse("covariation: malformed tree (a node that is a child twice)");
      parent[ch] = (int32_t)i;
    }
  }
  return DAFS_HIP_OK;  // 2n - 2 child slots hold distinct nodes below the root: every node but the root has its parent
}

int input_check(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint8_t* code) {
  if (!c || !n || !len || !code) return DAFS_HIP_EINVAL;
  if (n > (1u << 20) || (double)n * (double)len * (double)len > 35184372088832.0) return DAFS_HIP_EINVAL;  // 2^45: T fits an int64
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  for (size_t k = 0; k < (size_t)n * len; ++k)
    if (code[k] > 4) return DAFS_HIP_EINVAL;
  return DAFS_HIP_OK;
}

// DAFS_COV_TREE_LDS=0 (read per call): k_cov_evolve keeps the joins' states in global memory at every n (tests reach that
// form at a small n)
bool evolve_in_lds(uint32_t n) { return !env_off("DAFS_COV_TREE_LDS") && cov_evolve_fits_lds(n); }

uint64_t null_base(uint64_t seed, uint32_t k) { return mix64(seed + kMixGolden * ((uint64_t)k + 1)); }

}  // namespace

extern "C" int dafs_hip_alignment_covariation(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint8_t* code, const uint32_t* ss,
                                              uint32_t shuffles, uint64_t seed, int64_t* col_sum, uint32_t* best, double* best_score,
                                              double* best_e, double* pair_score, double* pair_e, uint32_t* pair_rows,
                                              uint32_t* pair_canonical, uint32_t* pair_types, int64_t* total, int64_t* g) {
  return dafs_hip_alignment_covariation_null(c, n, len, code, ss, shuffles, seed, DAFS_COV_NULL_SHUFFLE, nullptr, nullptr, col_sum, best,
                                             best_score, best_e, pair_score, pair_e, pair_rows, pair_canonical, pair_types, total, g);
}

extern "C" int dafs_hip_covariation_null_alignment(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint8_t* code, int null,
                                                   const int32_t* tree_left, const int32_t* tree_right, uint64_t seed, uint32_t k,
                                                   uint8_t* out_code) {
  int rc;
  if ((rc = null_args_check(null, tree_left, tree_right))) return rc;
  if (!out_code) return DAFS_HIP_EINVAL;
  if ((rc = input_check(c, n, len, code))) return rc;
  const bool by_tree = null == DAFS_COV_NULL_TREE;
  std::vector<int32_t> tree;
  if (by_tree && (tree_left || n >= 2) && (rc = tree_of(c, n, len, code, tree_left, tree_right, tree))) return rc;
  if (n < 2) {  // one row: nothing to permute, no branch to change on; no launch
    std::copy(code, code + len, out_code);
    return DAFS_HIP_OK;
  }
  const size_t cells = (size_t)n * len, T = 2 * (size_t)n - 1;
  carve cv;
  const size_t o_code = cv.take(cells), o_out = cv.take(cells), o_node = cv.take(by_tree ? T * len : 0), o_chg = cv.take(by_tree ? T * len : 0);
  const size_t o_tree = cv.take(by_tree ? 3 * T * 4 : 0);
  if ((rc = c->work.reserve(cv.reserve_bytes()))) return rc;
  uint8_t* w = c->work.ptr;
  call_frame f(c);
  hipStream_t st = f.st;
  if (f.up(w + o_code, code, cells)) return DAFS_HIP_ELAUNCH;
  if (by_tree) {
    if (f.up(w + o_tree, tree.data(), 3 * T * 4)) return DAFS_HIP_ELAUNCH;
    const int32_t* d_tree = (const int32_t*)(w + o_tree);
    const cov_tree t = {d_tree, d_tree + T, d_tree + 2 * T};
    if ((rc = cov_fitch(w + o_code, t, n, len, w + o_node, w + o_chg, st))) return rc;
    if ((rc = cov_evolve(w + o_code, w + o_chg, t, n, len, null_base(seed, k), w + o_node, w + o_out, evolve_in_lds(n), st))) return rc;
  } else if ((rc = cov_shuffle(w + o_code, w + o_out, n, len, null_base(seed, k), st))) {
    return rc;
  }
  if (f.down(out_code, w + o_out, cells)) return DAFS_HIP_ELAUNCH;
  return f.finish();
}

extern "C" int dafs_hip_alignment_covariation_null(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint8_t* code, const uint32_t* ss,
                                                   uint32_t shuffles, uint64_t seed, int null, const int32_t* tree_left,
                                                   const int32_t* tree_right, int64_t* col_sum, uint32_t* best, double* best_score,
                                                   double* best_e, double* pair_score, double* pair_e, uint32_t* pair_rows,
                                                   uint32_t* pair_canonical, uint32_t* pair_types, int64_t* total, int64_t* g) {
  int rc;
  if ((rc = null_args_check(null, tree_left, tree_right))) return rc;
  if ((rc = input_check(c, n, len, code))) return rc;
  std::vector<uint32_t> lefts;
  if (ss) {  // as dafs_hip_alignment_reliability takes it; lefts: the left columns of its pairs
    std::vector<uint8_t> used;
    if (!structure_ok(ss, len, used)) return DAFS_HIP_EINVAL;
    for (uint32_t col = 0; col < len; ++col)
      if (ss[col] != DAFS_HIP_NONE) lefts.push_back(col);
  }
  // the tree null's tree, before any output is written: the caller's is checked whenever it is there, the default one is
  // built only where the new kernels will run (n >= 2, len >= 2, a null that somebody reads)
  const bool by_tree = null == DAFS_COV_NULL_TREE && n >= 2 && len >= 2 && shuffles && (best_e || pair_e);
  std::vector<int32_t> tree;
  if ((tree_left || by_tree) && (rc = tree_of(c, n, len, code, tree_left, tree_right, tree))) return rc;
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
  // tests: a smaller LDS stage (the results do not depend on it)
  const uint32_t chunk = std::min(words, (uint32_t)env_uint("DAFS_COV_CHUNK_WORDS", 1, kCovMaxChunk, kCovMaxChunk));
  const uint32_t ncand = len + (uint32_t)lefts.size();
  uint32_t copies = 64;
  while (copies > 1 && (size_t)copies * ncand * 8 > ((size_t)64 << 20)) copies /= 2;

  carve cv;  // device workspace, carved from c->work
  const size_t o_code = cv.take((size_t)n * len), o_shuf = cv.take(shuffles ? (size_t)n * len : 0), o_planes = cv.take((size_t)words * 4 * len * 4);
  const size_t o_lnq = cv.take(((size_t)n + 1) * 8), o_sum = cv.take((size_t)len * 8), o_tot = cv.take(8), o_key = cv.take((size_t)len * 8);
  const size_t o_best = cv.take((size_t)len * 4), o_ss = cv.take((size_t)len * 4), o_ps = cv.take((size_t)len * 8);
  const size_t o_pr = cv.take((size_t)len * 4 * 3);
  const size_t o_cand = cv.take((size_t)ncand * 8), o_tail = cv.take(shuffles ? (size_t)copies * ncand * 8 : 0);
  const size_t T = 2 * (size_t)n - 1;  // the tree null: Fitch's scratch, the change records, left / right / parent
  const size_t o_node = cv.take(by_tree ? T * len : 0), o_chg = cv.take(by_tree ? T * len : 0), o_tree = cv.take(by_tree ? 3 * T * 4 : 0);
  if ((rc = c->work.reserve(cv.reserve_bytes()))) return rc;
  uint8_t* w = c->work.ptr;
  std::vector<unsigned long long> key(len), tail(shuffles ? (size_t)copies * ncand : 0);
  std::vector<double> bs(len), ps(len, 0.0), cand;
  int64_t tot = 0;
  call_frame f(c);
  hipStream_t st = f.st;
  void* gm = nullptr;  // the Gq matrix of one call: not kept in the context
  if (g && !(gm = f.alloc((size_t)len * len * 8))) return DAFS_HIP_ENOMEM;

  cov_args a;
  memset(&a, 0, sizeof a);
  a.planes = (const uint32_t*)(w + o_planes);
  a.lnq = (const int64_t*)(w + o_lnq);
  a.col_sum = (unsigned long long*)(w + o_sum);
  a.total = (const long long*)(w + o_tot);
  a.g = (long long*)gm;
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
  if (f.up(w + o_code, code, (size_t)n * len) || f.up(w + o_lnq, lnq.data(), lnq.size() * 8) || (ss && f.up(w + o_ss, ss, (size_t)len * 4)))
    return DAFS_HIP_ELAUNCH;
  if (f.fill(w + o_sum, 0, (size_t)len * 8) || f.fill(w + o_key, 0, (size_t)len * 8) || f.fill(w + o_best, 0xFF, (size_t)len * 4)) return DAFS_HIP_ELAUNCH;
  if (gm && f.fill(gm, 0, (size_t)len * len * 8)) return DAFS_HIP_ELAUNCH;
  if ((rc = cov_pack(w + o_code, n, len, (uint32_t*)(w + o_planes), st))) return rc;
  if ((rc = cov_pairs(COV_SUMS, a, st))) return rc;
  if ((rc = cov_total(a.col_sum, len, (long long*)(w + o_tot), st))) return rc;
  if ((rc = cov_pairs(COV_BEST, a, st))) return rc;
  if ((rc = cov_pairs(COV_ARG, a, st))) return rc;
  if (ss && (rc = cov_ss(a, sa, st))) return rc;
  if (f.down(key.data(), w + o_key, (size_t)len * 8) || f.down(&tot, w + o_tot, 8)) return DAFS_HIP_ELAUNCH;
  if (ss && f.down(ps.data(), w + o_ps, (size_t)len * 8)) return DAFS_HIP_ELAUNCH;
  // what the caller asked for goes into its memory directly
  if (f.down(col_sum, w + o_sum, (size_t)len * 8) || f.down(best, w + o_best, (size_t)len * 4)) return DAFS_HIP_ELAUNCH;
  if (ss && (f.down(pair_rows, w + o_pr, (size_t)len * 4) || f.down(pair_canonical, w + o_pr + (size_t)len * 4, (size_t)len * 4) ||
             f.down(pair_types, w + o_pr + (size_t)len * 8, (size_t)len * 4)))
    return DAFS_HIP_ELAUNCH;
  if (f.down(g, gm, (size_t)len * len * 8)) return DAFS_HIP_ELAUNCH;
  if ((rc = f.finish())) return rc;
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
  if (f.up(w + o_cand, cand.data(), (size_t)ncand * 8) || f.fill(w + o_tail, 0, (size_t)copies * ncand * 8)) return DAFS_HIP_ELAUNCH;
  const int32_t* d_tree = (const int32_t*)(w + o_tree);
  const cov_tree t = {d_tree, d_tree + T, d_tree + 2 * T};
  const bool in_lds = by_tree && evolve_in_lds(n);
  if (by_tree) {  // once per call: the change records of every branch
    if (f.up(w + o_tree, tree.data(), 3 * T * 4)) return DAFS_HIP_ELAUNCH;
    if ((rc = cov_fitch(w + o_code, t, n, len, w + o_node, w + o_chg, st))) return rc;
  }
  for (uint32_t k = 0; k < shuffles; ++k) {
    const uint64_t base = null_base(seed, k);
    if (by_tree) rc = cov_evolve(w + o_code, w + o_chg, t, n, len, base, w + o_node, w + o_shuf, in_lds, st);
    else rc = cov_shuffle(w + o_code, w + o_shuf, n, len, base, st);
    if (rc) return rc;
    if ((rc = cov_pack(w + o_shuf, n, len, (uint32_t*)(w + o_planes), st))) return rc;
    if (f.fill(w + o_sum, 0, (size_t)len * 8)) return DAFS_HIP_ELAUNCH;
    cov_args b = a;
    b.g = nullptr;
    if ((rc = cov_pairs(COV_SUMS, b, st))) return rc;
    if ((rc = cov_total(b.col_sum, len, (long long*)(w + o_tot), st))) return rc;
    if ((rc = cov_pairs(COV_NULL, b, st))) return rc;
  }
  if (f.down(tail.data(), w + o_tail, tail.size() * 8)) return DAFS_HIP_ELAUNCH;
  if ((rc = f.finish())) return rc;
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
