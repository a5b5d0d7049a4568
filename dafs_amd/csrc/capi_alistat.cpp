// dafs_amd/csrc/capi_alistat.cpp -- dafs_hip_alignment_identity, dafs_hip_alignment_weights, dafs_host_nr_select: how similar
// the rows of an alignment are to one another (alistat.hip; definitions in DESIGN.md section 18).  The reference has no
// counterpart.  The device calls read the alignment's cells alone, none of the context's stores, so they describe any
// alignment, also on a context without sequences.
//
// Host work: the checks (everything is refused before the first launch), the order of the passes, the diagonal of the
// matrices, unpacking the nearest rows, and the last two steps of the weights (U and the scaling).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/dafs_hip.h"
#include "alistat.h"
#include "call_frame.h"
#include "call_host.h"

using namespace dafs;

namespace {

// the checks both calls share: sizes, codes, and a residue in the used columns of every row
bool cells_ok(uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use) {
  if (!n || !len || !cell || n > kAliMaxRows || len > kAliMaxLen) return false;
  for (uint32_t r = 0; r < n; ++r) {
    const uint8_t* row = cell + (size_t)r * len;
    bool residue = false;
    for (uint32_t c = 0; c < len; ++c) {
      if (row[c] > 5) return false;
      if (row[c] <= 4 && (!use || use[c])) residue = true;
    }
    if (!residue) return false;
  }
  return true;
}

}  // namespace

extern "C" int dafs_hip_alignment_identity(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use,
                                           const uint8_t* cand, double nr_threshold, uint32_t* res, uint32_t* ident, uint32_t* aligned,
                                           uint32_t* nearest, uint32_t* nearest_ident, uint32_t* nearest_den, uint32_t* red) {
  if (!c || !cells_ok(n, len, cell, use)) return DAFS_HIP_EINVAL;
  if (!(nr_threshold >= 0.0 && nr_threshold <= 1.0)) return DAFS_HIP_EINVAL;  // a NaN too
  const bool want_red = red && nr_threshold > 0.0, want_near = nearest || nearest_ident || nearest_den;
  if ((ident || aligned) && n > 32768) return DAFS_HIP_EINVAL;
  if (want_red && n > 65536) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;

  const uint32_t words = (len + 63) / 64, redw = (n + 31) / 32;
  // tests: a smaller LDS stage (the results do not depend on it)
  const uint32_t chunk = std::min(words, (uint32_t)env_uint("DAFS_ALI_CHUNK_WORDS", 1, kAliMaxChunk, kAliMaxChunk));
  // tests: several launches per pass at small sizes
  const uint32_t band_blocks = (uint32_t)env_uint("DAFS_ALI_BAND_BLOCKS", 1, kAliBandBlocks, kAliBandBlocks);

  carve cv;  // device workspace, carved from c->work
  const size_t o_cell = cv.take((size_t)n * len), o_use = cv.take(use ? len : 0), o_cand = cv.take(cand ? n : 0);
  const size_t o_planes = cv.take((size_t)words * 4 * n * 8), o_res = cv.take((size_t)n * 4), o_base = cv.take((size_t)n * 4);
  const size_t o_best = cv.take((size_t)n * 8), o_ni = cv.take((size_t)n * 4), o_nd = cv.take((size_t)n * 4);
  int rc;
  if ((rc = c->work.reserve(cv.reserve_bytes()))) return rc;
  uint8_t* w = c->work.ptr;
  std::vector<uint32_t> h_res(n), h_base(n), h_ni(n, 0), h_nd(n, 0);
  std::vector<unsigned long long> h_best(n, 0);
  call_frame f(c);
  hipStream_t st = f.st;
  void *mi = nullptr, *ma = nullptr, *mr = nullptr;  // the matrices of one call: not kept in the context
  if (n > 1) {
    if (ident && !(mi = f.alloc((size_t)n * n * 4))) return DAFS_HIP_ENOMEM;
    if (aligned && !(ma = f.alloc((size_t)n * n * 4))) return DAFS_HIP_ENOMEM;
    if (want_red && !(mr = f.alloc((size_t)n * redw * 4))) return DAFS_HIP_ENOMEM;
  }

  ali_args a;
  memset(&a, 0, sizeof a);
  a.planes = (const uint64_t*)(w + o_planes);
  a.res = (const uint32_t*)(w + o_res);
  a.cand = cand ? w + o_cand : nullptr;
  a.ident = (uint32_t*)mi;
  a.aligned = (uint32_t*)ma;
  a.best = (unsigned long long*)(w + o_best);
  a.red = (uint32_t*)mr;
  a.threshold = nr_threshold;
  a.n = n; a.words = words; a.chunk = chunk; a.redw = redw; a.band_blocks = band_blocks;

  if (f.up(w + o_cell, cell, (size_t)n * len) || f.up(w + o_use, use, use ? len : 0) || f.up(w + o_cand, cand, cand ? n : 0)) return DAFS_HIP_ELAUNCH;
  if (f.fill(w + o_res, 0, (size_t)n * 4) || f.fill(w + o_base, 0, (size_t)n * 4) || f.fill(w + o_best, 0, (size_t)n * 8)) return DAFS_HIP_ELAUNCH;
  if ((rc = ali_pack(w + o_cell, use ? w + o_use : nullptr, n, len, (uint64_t*)(w + o_planes), (uint32_t*)(w + o_res), (uint32_t*)(w + o_base), st)))
    return rc;
  if (n > 1) {
    if ((mi || ma) && (rc = ali_pairs(ALI_MATRIX, a, st))) return rc;
    if (want_near) {
      if ((rc = ali_pairs(ALI_NEAREST, a, st))) return rc;
      if ((rc = ali_nearest_counts(a, (uint32_t*)(w + o_ni), (uint32_t*)(w + o_nd), st))) return rc;
      if (f.down(h_best.data(), w + o_best, (size_t)n * 8) || f.down(h_ni.data(), w + o_ni, (size_t)n * 4) || f.down(h_nd.data(), w + o_nd, (size_t)n * 4))
        return DAFS_HIP_ELAUNCH;
    }
    if (want_red && (rc = ali_pairs(ALI_RED, a, st))) return rc;
  }
  if (f.down(h_res.data(), w + o_res, (size_t)n * 4) || f.down(h_base.data(), w + o_base, (size_t)n * 4)) return DAFS_HIP_ELAUNCH;
  // the large outputs go to the caller directly; their diagonal is written after the wait
  if (mi && f.down(ident, mi, (size_t)n * n * 4)) return DAFS_HIP_ELAUNCH;
  if (ma && f.down(aligned, ma, (size_t)n * n * 4)) return DAFS_HIP_ELAUNCH;
  if (mr && f.down(red, mr, (size_t)n * redw * 4)) return DAFS_HIP_ELAUNCH;
  if ((rc = f.finish())) return rc;

  if (res) std::copy(h_res.begin(), h_res.end(), res);
  for (uint32_t r = 0; r < n; ++r) {
    if (ident) ident[(size_t)r * n + r] = h_base[r];
    if (aligned) aligned[(size_t)r * n + r] = h_res[r];
    const uint32_t s = h_best[r] ? ali_best_row(h_best[r]) : DAFS_HIP_NONE;
    if (nearest) nearest[r] = s;
    if (nearest_ident) nearest_ident[r] = h_ni[r];
    if (nearest_den) nearest_den[r] = h_nd[r];
  }
  if (want_red && n == 1) red[0] = 0;
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_alignment_weights(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use, double* weight) {
  if (!c || !weight || !cells_ok(n, len, cell, use)) return DAFS_HIP_EINVAL;
  if (n == 1) {  // no launch
    weight[0] = 1.0;
    return DAFS_HIP_OK;
  }
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  carve cv;
  const size_t o_cell = cv.take((size_t)n * len), o_cell_t = cv.take((size_t)n * len), o_use = cv.take(use ? len : 0);
  const size_t o_cnt = cv.take((size_t)5 * len * 4), o_inv = cv.take((size_t)5 * len * 8), o_u = cv.take((size_t)n * 8);
  int rc;
  if ((rc = c->work.reserve(cv.reserve_bytes()))) return rc;
  uint8_t* w = c->work.ptr;
  std::vector<double> u(n);
  call_frame f(c);
  hipStream_t st = f.st;
  if (f.up(w + o_cell, cell, (size_t)n * len) || f.up(w + o_use, use, use ? len : 0)) return DAFS_HIP_ELAUNCH;
  if ((rc = ali_transpose(w + o_cell, n, len, w + o_cell_t, st))) return rc;
  if ((rc = ali_columns(w + o_cell, n, len, (uint32_t*)(w + o_cnt), (double*)(w + o_inv), st))) return rc;
  if ((rc = ali_row_weights(w + o_cell_t, use ? w + o_use : nullptr, (const double*)(w + o_inv), n, len, (double*)(w + o_u), st))) return rc;
  if (f.down(u.data(), w + o_u, (size_t)n * 8)) return DAFS_HIP_ELAUNCH;
  if ((rc = f.finish())) return rc;
  double total = 0.0;
  for (uint32_t r = 0; r < n; ++r) total += u[r];
  for (uint32_t r = 0; r < n; ++r) weight[r] = (u[r] * (double)n) / total;
  return DAFS_HIP_OK;
}

extern "C" int dafs_host_nr_select(uint32_t n, const uint32_t* red, const uint32_t* rank, const uint8_t* forced, uint8_t* kept, uint32_t* by) {
  if (!n || !red || !rank || !kept || !by) {
    set_last_error("nr_select: no rows, or a missing array");
    return DAFS_HIP_EINVAL;
  }
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t k = 0; k < n; ++k) {
    if (rank[k] >= n || seen[rank[k]]) {
      set_last_error("nr_select: the visiting order is not a permutation of the rows");
      return DAFS_HIP_EINVAL;
    }
    seen[rank[k]] = 1;
  }
  const size_t redw = ((size_t)n + 31) / 32;
  std::vector<uint32_t> keepers;  // the kept rows in visiting order
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t r = rank[k];
    const uint32_t* row = red + (size_t)r * redw;
    uint32_t remover = DAFS_HIP_NONE;
    if (!forced || !forced[r])
      for (uint32_t q : keepers)
        if ((row[q / 32] >> (q % 32)) & 1u) { remover = q; break; }
    kept[r] = remover == DAFS_HIP_NONE ? 1 : 0;
    by[r] = remover;
    if (kept[r]) keepers.push_back(r);
  }
  return DAFS_HIP_OK;
}
