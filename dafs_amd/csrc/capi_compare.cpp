// dafs_amd/csrc/capi_compare.cpp -- dafs_hip_alignment_compare: how far two alignments of the same sequences agree
// (compare.hip; definitions in DESIGN.md section 19).  The reference has no counterpart.  The call reads the two alignments'
// cells alone, none of the context's stores, so it compares any two alignments, also on a context without sequences.
//
// Host work: the checks (everything is refused before the first launch), the structures in their left-column form, the order
// of the kernels, the totals (integer sums of the row sums) and every quotient.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "../../include/dafs_hip.h"
#include "call_frame.h"
#include "call_host.h"
#include "compare.h"

using namespace dafs;

namespace {

// ss (either form) -> the partner at the left column of a pair, DAFS_HIP_NONE elsewhere; false for a bad structure
bool left_form(const uint32_t* ss, uint32_t len, std::vector<uint32_t>& left) {
  left.assign(len, DAFS_HIP_NONE);
  std::vector<uint8_t> taken(len, 0);
  for (uint32_t c = 0; c < len; ++c) {
    const uint32_t d = ss[c];
    if (d == DAFS_HIP_NONE) continue;
    if (d >= len || d == c) return false;
    if (d < c) {  // the right column of the symmetric form
      if (ss[d] != c) return false;
      continue;
    }
    if (taken[c] || taken[d]) return false;
    taken[c] = taken[d] = 1;
    left[c] = d;
  }
  return true;
}

double quotient(uint64_t a, uint64_t b) { return b ? (double)a / (double)b : std::numeric_limits<double>::quiet_NaN(); }

}  // namespace

extern "C" int dafs_hip_alignment_compare(dafs_hip_ctx* c, uint32_t n, uint32_t len_r, uint32_t len_t, const uint8_t* cell_r,
                                          const uint8_t* cell_t, const uint8_t* use_r, const uint8_t* use_t, const uint32_t* ss_r,
                                          const uint32_t* ss_t, const uint8_t* pp, const dafs_compare_out* out) {
  if (!c || !out || !cell_r || !cell_t) return refuse("alignment_compare: a missing argument");
  if (n < 2 || n > kCmpMaxRows) return refuse("alignment_compare: it takes 2 to 2^20 rows");
  if (!len_r || !len_t || len_r > kCmpMaxLen || len_t > kCmpMaxLen) return refuse("alignment_compare: it takes 1 to 2^20 columns");
  if ((uint64_t)len_r * len_t > kCmpMaxCells) return refuse("alignment_compare: the product of the two lengths is above 2^30");
  const dafs_compare_out& o = *out;
  const bool want_pairs = o.pair_shared || o.pair_refp || o.pair_testp;
  const bool want_ss = o.tp || o.nref || o.ntest || o.ss_total;
  const bool want_rows = o.shared || o.refp || o.testp || o.sps || o.ppv || o.total || o.score || o.pp_count;
  const bool want_cols = o.colref || o.colshared || o.reproduced || o.tc || o.score;
  const bool want_count = want_rows || want_cols || o.k || o.m;
  if (want_pairs && n > kCmpMatrixRows) return refuse("alignment_compare: the pair matrices take 16384 rows at most");
  if (want_ss && (!ss_r || !ss_t)) return refuse("alignment_compare: the structure part needs both structures");
  if (o.pp_count && !pp) return refuse("alignment_compare: the PP part needs pp");
  // the rows: codes, and the same residues in both alignments
  for (uint32_t r = 0; r < n; ++r) {
    const uint8_t* x = cell_r + (size_t)r * len_r;
    const uint8_t* y = cell_t + (size_t)r * len_t;
    uint32_t i = 0, j = 0;
    bool same = true;
    for (;;) {
      while (i < len_r && x[i] == 5) ++i;
      while (j < len_t && y[j] == 5) ++j;
      if (i < len_r && x[i] > 5) return refuse("alignment_compare: a cell code above 5");
      if (j < len_t && y[j] > 5) return refuse("alignment_compare: a cell code above 5");
      if (i == len_r || j == len_t) {
        if (i != len_r || j != len_t) same = false;
        break;
      }
      if (x[i] != y[j]) same = false;
      ++i;
      ++j;
    }
    for (; i < len_r; ++i) if (x[i] > 5) return refuse("alignment_compare: a cell code above 5");  // a difference does not hide a bad code
    for (; j < len_t; ++j) if (y[j] > 5) return refuse("alignment_compare: a cell code above 5");
    if (!same) {
      char msg[96];
      snprintf(msg, sizeof msg, "alignment_compare: row %u holds different residues in the two alignments", r + 1);
      set_last_error(msg);
      return DAFS_HIP_EINVAL;
    }
  }
  if (pp)
    for (size_t i = 0; i < (size_t)n * len_t; ++i)
      if (pp[i] >= kCmpClasses && pp[i] != 255) return refuse("alignment_compare: a PP class is 0..10, or 255 for none");
  std::vector<uint32_t> left_r, left_t;
  if (want_ss && (!left_form(ss_r, len_r, left_r) || !left_form(ss_t, len_t, left_t)))
    return refuse("alignment_compare: a structure has a partner beyond its length, a column in two pairs or a one-sided right column");
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;

  // tests: a smaller LDS stage (the results do not depend on it)
  const uint32_t chunk = (uint32_t)env_uint("DAFS_CMP_CHUNK_COLS", 1, kCmpMaxChunk, kCmpMaxChunk);
  // tests: several launches per pass at small sizes
  const uint32_t band_blocks = (uint32_t)env_uint("DAFS_CMP_BAND_BLOCKS", 1, kCmpBandBlocks, kCmpBandBlocks);

  carve cv;  // device workspace, carved from c->work; the dense cnt and the pair matrices are this call's own
  const size_t nr = (size_t)n * len_r, nt = (size_t)n * len_t;
  const size_t o_cell_r = cv.take(nr), o_cell_t = cv.take(nt), o_use_r = cv.take(use_r ? len_r : 0), o_use_t = cv.take(use_t ? len_t : 0);
  const size_t o_ss_r = cv.take(want_ss ? (size_t)len_r * 4 : 0), o_ss_t = cv.take(want_ss ? (size_t)len_t * 4 : 0);
  const size_t o_pp = cv.take(o.pp_count ? nt : 0);
  const size_t o_nres = cv.take((size_t)n * 4), o_col_r = cv.take(nr * 4), o_col_t = cv.take(nt * 4), o_idx_r = cv.take(nr * 4);
  const size_t o_key = cv.take(nr * 4), o_occ = cv.take(o.pair_testp ? nt * 4 : 0);
  const size_t o_k = cv.take((size_t)len_r * 4), o_m = cv.take((size_t)len_t * 4);
  const size_t o_row = cv.take((size_t)3 * n * 8), o_bins = cv.take((size_t)3 * kCmpClasses * 8);
  const size_t o_colref = cv.take((size_t)len_r * 8), o_colshared = cv.take((size_t)len_r * 8), o_rep = cv.take(len_r);
  const size_t o_ss_row = cv.take(want_ss ? (size_t)3 * n * 8 : 0);
  int rc;
  if ((rc = c->work.reserve(cv.reserve_bytes()))) return rc;
  uint8_t* w = c->work.ptr;
  std::vector<uint32_t> h_nres(n), h_k(len_r), h_m(len_t);
  std::vector<uint64_t> h_row((size_t)3 * n), h_bins(3 * kCmpClasses), h_colref(len_r), h_colshared(len_r), h_ss((size_t)3 * n);
  std::vector<uint8_t> h_rep(len_r);
  call_frame f(c);
  hipStream_t st = f.st;
  void *mc = nullptr, *ms = nullptr, *mp = nullptr, *mt = nullptr;
  if (want_count && !(mc = f.alloc((size_t)len_r * len_t * 4))) return DAFS_HIP_ENOMEM;
  if (want_pairs) {  // the shared pass counts refp too: its matrix is there whenever either is asked for
    if ((o.pair_shared || o.pair_refp) && (!(ms = f.alloc((size_t)n * n * 4)) || !(mp = f.alloc((size_t)n * n * 4)))) return DAFS_HIP_ENOMEM;
    if (o.pair_testp && !(mt = f.alloc((size_t)n * n * 4))) return DAFS_HIP_ENOMEM;
  }

  cmp_args a;
  memset(&a, 0, sizeof a);
  a.cell_r = w + o_cell_r;
  a.cell_t = w + o_cell_t;
  a.use_r = use_r ? w + o_use_r : nullptr;
  a.use_t = use_t ? w + o_use_t : nullptr;
  a.ss_r = want_ss ? (const uint32_t*)(w + o_ss_r) : nullptr;
  a.ss_t = want_ss ? (const uint32_t*)(w + o_ss_t) : nullptr;
  a.pp = o.pp_count ? w + o_pp : nullptr;
  a.n = n; a.len_r = len_r; a.len_t = len_t;
  a.nres = (uint32_t*)(w + o_nres);
  a.col_r = (uint32_t*)(w + o_col_r);
  a.col_t = (uint32_t*)(w + o_col_t);
  a.idx_r = (uint32_t*)(w + o_idx_r);
  a.key = (uint32_t*)(w + o_key);
  a.occ_t = o.pair_testp ? (uint32_t*)(w + o_occ) : nullptr;
  a.k = (uint32_t*)(w + o_k);
  a.m = (uint32_t*)(w + o_m);
  a.cnt = (uint32_t*)mc;
  a.row = (unsigned long long*)(w + o_row);
  a.bins = (unsigned long long*)(w + o_bins);
  a.colref = (unsigned long long*)(w + o_colref);
  a.colshared = (unsigned long long*)(w + o_colshared);
  a.reproduced = w + o_rep;
  a.ss_row = want_ss ? (unsigned long long*)(w + o_ss_row) : nullptr;

  if (f.up(w + o_cell_r, cell_r, nr) || f.up(w + o_cell_t, cell_t, nt) || f.up(w + o_use_r, use_r, use_r ? len_r : 0) ||
      f.up(w + o_use_t, use_t, use_t ? len_t : 0) || f.up(w + o_pp, pp, o.pp_count ? nt : 0))
    return DAFS_HIP_ELAUNCH;
  if (want_ss && (f.up(w + o_ss_r, left_r.data(), (size_t)len_r * 4) || f.up(w + o_ss_t, left_t.data(), (size_t)len_t * 4))) return DAFS_HIP_ELAUNCH;
  if ((rc = cmp_map(a, st))) return rc;
  if (f.down(h_nres.data(), a.nres, (size_t)n * 4)) return DAFS_HIP_ELAUNCH;
  if (want_count) {
    if ((rc = cmp_count(a, st))) return rc;
    if (f.down(h_k.data(), a.k, (size_t)len_r * 4) || f.down(h_m.data(), a.m, (size_t)len_t * 4)) return DAFS_HIP_ELAUNCH;
  }
  if (want_rows) {
    if ((rc = cmp_residue(a, st))) return rc;
    if (f.down(h_row.data(), a.row, (size_t)3 * n * 8) || f.down(h_bins.data(), a.bins, (size_t)3 * kCmpClasses * 8)) return DAFS_HIP_ELAUNCH;
  }
  if (want_cols) {
    if ((rc = cmp_columns(a, st))) return rc;
    if (f.down(h_colref.data(), a.colref, (size_t)len_r * 8) || f.down(h_colshared.data(), a.colshared, (size_t)len_r * 8) ||
        f.down(h_rep.data(), a.reproduced, len_r))
      return DAFS_HIP_ELAUNCH;
  }
  if (want_ss) {
    if ((rc = cmp_ss(a, st))) return rc;
    if (f.down(h_ss.data(), a.ss_row, (size_t)3 * n * 8)) return DAFS_HIP_ELAUNCH;
  }
  if (want_pairs) {
    const size_t bytes = (size_t)n * n * 4;
    if (ms) {
      if (f.fill(ms, 0, bytes) || f.fill(mp, 0, bytes)) return DAFS_HIP_ELAUNCH;  // the diagonal
      if ((rc = cmp_pairs(a.key, n, len_r, chunk, band_blocks, (uint32_t*)mp, (uint32_t*)ms, st))) return rc;
    }
    if (mt) {
      if (f.fill(mt, 0, bytes)) return DAFS_HIP_ELAUNCH;
      if ((rc = cmp_pairs(a.occ_t, n, len_t, chunk, band_blocks, (uint32_t*)mt, nullptr, st))) return rc;
    }
    // the large outputs go to the caller directly
    if (f.down(o.pair_shared, ms, bytes) || f.down(o.pair_refp, mp, bytes) || f.down(o.pair_testp, mt, bytes)) return DAFS_HIP_ELAUNCH;
  }
  if ((rc = f.finish())) return rc;

  if (o.residues) std::copy(h_nres.begin(), h_nres.end(), o.residues);
  if (o.k) std::copy(h_k.begin(), h_k.end(), o.k);
  if (o.m) std::copy(h_m.begin(), h_m.end(), o.m);
  if (want_rows) {
    uint64_t tot[3] = {0, 0, 0};
    for (uint32_t r = 0; r < n; ++r) {
      const uint64_t sh = h_row[r], rp = h_row[(size_t)n + r], tp = h_row[(size_t)2 * n + r];
      tot[0] += sh; tot[1] += rp; tot[2] += tp;
      if (o.shared) o.shared[r] = sh;
      if (o.refp) o.refp[r] = rp;
      if (o.testp) o.testp[r] = tp;
      if (o.sps) o.sps[r] = quotient(sh, rp);
      if (o.ppv) o.ppv[r] = quotient(sh, tp);
    }
    for (uint64_t& t : tot) t /= 2;  // every pair was counted from both of its rows
    if (o.total) std::copy(tot, tot + 3, o.total);
    if (o.score) {
      o.score[0] = quotient(tot[0], tot[1]);
      o.score[1] = quotient(tot[0], tot[2]);
    }
    if (o.pp_count) std::copy(h_bins.begin(), h_bins.end(), o.pp_count);
  }
  if (want_cols) {
    uint64_t tc[2] = {0, 0};
    for (uint32_t col = 0; col < len_r; ++col) {
      tc[0] += h_rep[col] ? 1 : 0;
      tc[1] += h_k[col] >= 2 ? 1 : 0;
    }
    if (o.colref) std::copy(h_colref.begin(), h_colref.end(), o.colref);
    if (o.colshared) std::copy(h_colshared.begin(), h_colshared.end(), o.colshared);
    if (o.reproduced) std::copy(h_rep.begin(), h_rep.end(), o.reproduced);
    if (o.tc) std::copy(tc, tc + 2, o.tc);
    if (o.score) o.score[2] = quotient(tc[0], tc[1]);
  }
  if (want_ss) {
    uint64_t tot[3] = {0, 0, 0};
    for (uint32_t r = 0; r < n; ++r)
      for (int q = 0; q < 3; ++q) tot[q] += h_ss[(size_t)q * n + r];
    if (o.tp) std::copy(h_ss.begin(), h_ss.begin() + n, o.tp);
    if (o.nref) std::copy(h_ss.begin() + n, h_ss.begin() + 2 * (size_t)n, o.nref);
    if (o.ntest) std::copy(h_ss.begin() + 2 * (size_t)n, h_ss.end(), o.ntest);
    if (o.ss_total) std::copy(tot, tot + 3, o.ss_total);
  }
  return DAFS_HIP_OK;
}
