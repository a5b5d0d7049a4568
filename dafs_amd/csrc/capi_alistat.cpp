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
#include "ctx.h"
#include "hip_util.h"
#include "last_error.h"

using namespace dafs;

namespace {

struct dev_mem {  // the matrices of one call: not kept in the context
  void* p = nullptr;
  ~dev_mem() { if (p) (void)hipFree(p); }
};

// Every return waits for the stream: the queued copies read and write the caller's buffers and this call's vectors.
struct stream_drain {
  hipStream_t st;
  ~stream_drain() { (void)hipStreamSynchronize(st); }
};

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
  uint32_t chunk = std::min(words, kAliMaxChunk);
  if (const char* e = getenv("DAFS_ALI_CHUNK_WORDS")) {  // tests: a smaller LDS stage (the results do not depend on it)
    const long v = strtol(e, nullptr, 10);
    if (v >= 1 && v <= (long)kAliMaxChunk) chunk = std::min(words, (uint32_t)v);
  }

  uint32_t band_blocks = kAliBandBlocks;
  if (const char* e = getenv("DAFS_ALI_BAND_BLOCKS")) {  // tests: several launches per pass at small sizes
    const long v = strtol(e, nullptr, 10);
    if (v >= 1 && v <= (long)kAliBandBlocks) band_blocks = (uint32_t)v;
  }

  // device workspace, carved from c->work
  size_t used = 0;
  auto take = [&](size_t bytes) { const size_t at = used; used += (bytes + 255) & ~(size_t)255; return at; };
  const size_t o_cell = take((size_t)n * len), o_use = take(use ? len : 0), o_cand = take(cand ? n : 0);
  const size_t o_planes = take((size_t)words * 4 * n * 8), o_res = take((size_t)n * 4), o_base = take((size_t)n * 4);
  const size_t o_best = take((size_t)n * 8), o_ni = take((size_t)n * 4), o_nd = take((size_t)n * 4);
  int rc;
  if ((rc = c->work.reserve(used + 256))) return rc;
  uint8_t* w = c->work.ptr;
  dev_mem mi, ma, mr;
  if (n > 1) {
    if (ident && hip_check(hipMalloc(&mi.p, (size_t)n * n * 4))) return DAFS_HIP_ENOMEM;
    if (aligned && hip_check(hipMalloc(&ma.p, (size_t)n * n * 4))) return DAFS_HIP_ENOMEM;
    if (want_red && hip_check(hipMalloc(&mr.p, (size_t)n * redw * 4))) return DAFS_HIP_ENOMEM;
  }
  hipStream_t st = c->stream;
  std::vector<uint32_t> h_res(n), h_base(n), h_ni(n, 0), h_nd(n, 0);
  std::vector<unsigned long long> h_best(n, 0);
  stream_drain drain{st};  // declared after every host buffer the stream touches, so it waits before they go
  auto up = [&](size_t off, const void* src, size_t bytes) { return bytes && hip_check(hipMemcpyAsync(w + off, src, bytes, hipMemcpyHostToDevice, st)); };
  auto down = [&](void* dst, const void* src, size_t bytes) { return hip_check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st)); };

  ali_args a;
  memset(&a, 0, sizeof a);
  a.planes = (const uint64_t*)(w + o_planes);
  a.res = (const uint32_t*)(w + o_res);
  a.cand = cand ? w + o_cand : nullptr;
  a.ident = (uint32_t*)mi.p;
  a.aligned = (uint32_t*)ma.p;
  a.best = (unsigned long long*)(w + o_best);
  a.red = (uint32_t*)mr.p;
  a.threshold = nr_threshold;
  a.n = n; a.words = words; a.chunk = chunk; a.redw = redw; a.band_blocks = band_blocks;

  if (up(o_cell, cell, (size_t)n * len) || up(o_use, use, use ? len : 0) || up(o_cand, cand, cand ? n : 0)) return DAFS_HIP_ELAUNCH;
  if (hip_check(hipMemsetAsync(w + o_res, 0, (size_t)n * 4, st)) || hip_check(hipMemsetAsync(w + o_base, 0, (size_t)n * 4, st)) ||
      hip_check(hipMemsetAsync(w + o_best, 0, (size_t)n * 8, st)))
    return DAFS_HIP_ELAUNCH;
  if ((rc = ali_pack(w + o_cell, use ? w + o_use : nullptr, n, len, (uint64_t*)(w + o_planes), (uint32_t*)(w + o_res), (uint32_t*)(w + o_base), st)))
    return rc;
  if (n > 1) {
    if ((mi.p || ma.p) && (rc = ali_pairs(ALI_MATRIX, a, st))) return rc;
    if (want_near) {
      if ((rc = ali_pairs(ALI_NEAREST, a, st))) return rc;
      if ((rc = ali_nearest_counts(a, (uint32_t*)(w + o_ni), (uint32_t*)(w + o_nd), st))) return rc;
      if (down(h_best.data(), w + o_best, (size_t)n * 8) || down(h_ni.data(), w + o_ni, (size_t)n * 4) || down(h_nd.data(), w + o_nd, (size_t)n * 4))
        return DAFS_HIP_ELAUNCH;
    }
    if (want_red && (rc = ali_pairs(ALI_RED, a, st))) return rc;
  }
  if (down(h_res.data(), w + o_res, (size_t)n * 4) || down(h_base.data(), w + o_base, (size_t)n * 4)) return DAFS_HIP_ELAUNCH;
  // the large outputs go to the caller directly; their diagonal is written after the wait
  if (mi.p && down(ident, mi.p, (size_t)n * n * 4)) return DAFS_HIP_ELAUNCH;
  if (ma.p && down(aligned, ma.p, (size_t)n * n * 4)) return DAFS_HIP_ELAUNCH;
  if (mr.p && down(red, mr.p, (size_t)n * redw * 4)) return DAFS_HIP_ELAUNCH;
  if (hip_check(hipStreamSynchronize(st))) return DAFS_HIP_ELAUNCH;

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
  size_t used = 0;
  auto take = [&](size_t bytes) { const size_t at = used; used += (bytes + 255) & ~(size_t)255; return at; };
  const size_t o_cell = take((size_t)n * len), o_cell_t = take((size_t)n * len), o_use = take(use ? len : 0);
  const size_t o_cnt = take((size_t)5 * len * 4), o_inv = take((size_t)5 * len * 8), o_u = take((size_t)n * 8);
  int rc;
  if ((rc = c->work.reserve(used + 256))) return rc;
  uint8_t* w = c->work.ptr;
  hipStream_t st = c->stream;
  std::vector<double> u(n);
  stream_drain drain{st};
  if (hip_check(hipMemcpyAsync(w + o_cell, cell, (size_t)n * len, hipMemcpyHostToDevice, st))) return DAFS_HIP_ELAUNCH;
  if (use && hip_check(hipMemcpyAsync(w + o_use, use, len, hipMemcpyHostToDevice, st))) return DAFS_HIP_ELAUNCH;
  if ((rc = ali_transpose(w + o_cell, n, len, w + o_cell_t, st))) return rc;
  if ((rc = ali_columns(w + o_cell, n, len, (uint32_t*)(w + o_cnt), (double*)(w + o_inv), st))) return rc;
  if ((rc = ali_row_weights(w + o_cell_t, use ? w + o_use : nullptr, (const double*)(w + o_inv), n, len, (double*)(w + o_u), st))) return rc;
  if (hip_check(hipMemcpyAsync(u.data(), w + o_u, (size_t)n * 8, hipMemcpyDeviceToHost, st))) return DAFS_HIP_ELAUNCH;
  if (hip_check(hipStreamSynchronize(st))) return DAFS_HIP_ELAUNCH;
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
