// dafs_amd/csrc/capi_support.cpp -- dafs_hip_structure_support: per row of an alignment, how many pairs of a given structure
// it holds, how many of those its residues can form, and the base-pairing probability its own store gives them (support.hip).
// The reference has no counterpart.  Host work: the checks, all before the one launch, and the layout of the batch.
#include <hip/hip_runtime.h>
#include <string.h>
#include <vector>

#include "../../include/dafs_hip.h"
#include "call_frame.h"
#include "call_host.h"
#include "support.h"

using namespace dafs;

extern "C" int dafs_hip_structure_support(dafs_hip_ctx* c, uint32_t nalign, const uint32_t* n_rows, const uint32_t* len, const uint32_t* seq,
                                          const uint8_t* mask, const uint32_t* ss, uint32_t* both, uint32_t* canonical, uint32_t* half,
                                          double* expected) {
  if (!c) return DAFS_HIP_EINVAL;
  if (nalign == 0) return DAFS_HIP_OK;
  if (!n_rows || !len || !seq || !mask || !ss) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const bp_store& bps = c->bp[c->cur_bp];
  if (!bps.valid || c->fold_pending) return DAFS_HIP_EINVAL;
  const uint32_t N = (uint32_t)c->len.size();
  std::vector<sup_row> rows;
  uint64_t mask_at = 0, ss_at = 0;
  std::vector<uint8_t> used;
  for (uint32_t a = 0, r0 = 0; a < nalign; r0 += n_rows[a], ++a) {
    const uint32_t L = len[a];
    if (!n_rows[a] || !L) return DAFS_HIP_EINVAL;
    if (!structure_ok(ss + ss_at, L, used)) return DAFS_HIP_EINVAL;
    for (uint32_t r = 0; r < n_rows[a]; ++r) {
      const uint32_t x = seq[r0 + r];
      if (x >= N) return DAFS_HIP_EINVAL;
      uint32_t cnt = 0;
      for (uint32_t col = 0; col < L; ++col) cnt += mask[mask_at + col] ? 1 : 0;
      if (cnt != c->len[x]) return DAFS_HIP_EINVAL;
      sup_row row;
      row.mask_off = mask_at; row.pos_off = mask_at; row.ss_off = ss_at;
      row.len = L; row.seq = x; row.code_off = c->off[x]; row.pad = 0;
      rows.push_back(row);
      mask_at += L;
    }
    ss_at += L;
  }
  const size_t R = rows.size();
  if (R > 0x7fffffffull) return DAFS_HIP_EOVERFLOW;

  carve cv;  // device workspace, carved from c->work
  const size_t o_rows = cv.take(R * sizeof(sup_row)), o_ss = cv.take(ss_at * 4), o_mask = cv.take(mask_at), o_pos = cv.take(mask_at * 4);
  const size_t o_both = cv.take(R * 4), o_can = cv.take(R * 4), o_half = cv.take(R * 4), o_exp = cv.take(R * 8);
  int rc;
  if ((rc = c->work.reserve(cv.reserve_bytes()))) return rc;
  uint8_t* w = c->work.ptr;
  sup_args g;
  memset(&g, 0, sizeof g);
  g.bp = bps.view();
  g.rows = (const sup_row*)(w + o_rows);
  g.mask = w + o_mask;
  g.ss = (const uint32_t*)(w + o_ss);
  g.codes = c->codes.ptr;
  g.pos = (uint32_t*)(w + o_pos);
  g.both = (uint32_t*)(w + o_both);
  g.canonical = (uint32_t*)(w + o_can);
  g.half = (uint32_t*)(w + o_half);
  g.expected = (double*)(w + o_exp);
  g.nrows = (uint32_t)R;
  call_frame f(c);  // `rows` is in flight
  if (f.up(w + o_rows, rows.data(), R * sizeof(sup_row)) || f.up(w + o_ss, ss, ss_at * 4) || f.up(w + o_mask, mask, mask_at)) return DAFS_HIP_ELAUNCH;
  if ((rc = sup_launch(g, f.st))) return rc;
  // what the caller asked for goes into its memory directly
  if (f.down(both, g.both, R * 4) || f.down(canonical, g.canonical, R * 4) || f.down(half, g.half, R * 4) || f.down(expected, g.expected, R * 8))
    return DAFS_HIP_ELAUNCH;
  return f.finish();
}
