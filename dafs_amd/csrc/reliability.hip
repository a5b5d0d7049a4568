// dafs_amd/csrc/reliability.hip -- per-residue alignment reliability from the sparse stores a run already holds
// (dafs_hip_alignment_reliability, capi_reliability.cpp; definitions in DESIGN.md "Alignment reliability").
//
// rel(r, i) of residue i of row r (sequence x) at column c: over the other rows q (sequence y) in ascending row order, the
// term mp[x][y](i, j) when q has residue j at c, else max(0, 1 - sum of row i of mp[x][y]); their double sum / (n - 1).
// col(c) is the mean of rel over the residues of column c, the consensus-pair value the mean of bp[x](i, j) over the rows
// that hold both residues of a pair of ss.  Every sum runs in one thread in the stated order: no cross-lane reduction and
// no atomics, so the results do not depend on the launch geometry and repeat bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dafs_hip.h"
#include "hip_util.h"
#include "reliability.h"
#include "stage.h"

namespace dafs {

// One wavefront per row, 64 columns per step: pos[r * len + c] = residue index of row r at column c (DAFS_HIP_NONE for a
// gap) and col_of[res_off[r] + i] = column of residue i.  The mask has been checked to place exactly len[x] residues.
__global__ __launch_bounds__(64) void k_rel_pos(const uint8_t* __restrict__ mask, uint32_t len, const uint64_t* __restrict__ res_off,
                                                uint32_t* __restrict__ pos, uint32_t* __restrict__ col_of) {
  const uint32_t r = blockIdx.x, lane = threadIdx.x;
  const uint8_t* m = mask + (size_t)r * len;
  uint32_t* pr = pos + (size_t)r * len;
  uint32_t* co = col_of + res_off[r];
  uint32_t run = 0;
  for (uint32_t c0 = 0; c0 < len; c0 += 64) {
    const uint32_t c = c0 + lane;
    const bool res = c < len && m[c] != 0;
    const uint64_t b = __ballot(res);
    const uint32_t k = run + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    if (c < len) pr[c] = res ? k : DAFS_HIP_NONE;
    if (res) co[k] = c;
    run += (uint32_t)__popcll(b);
  }
}

// One wavefront per block of 64 consecutive residues of one row; lane t owns residue i0 + t and walks the other rows in
// order.  For each row q the lanes read adjacent row pointers of one matrix and then its adjacent rows (mp_row).
__global__ __launch_bounds__(256) void k_rel_residue(rel_args a) {
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= a.nblocks) return;
  const uint2 blk = a.blocks[w];
  const uint32_t r = blk.x, i = blk.y + (threadIdx.x & 63);
  const uint64_t r0 = a.res_off[r];
  if (i >= (uint32_t)(a.res_off[r + 1] - r0)) return;
  const uint32_t x = a.seq[r];
  const uint32_t c = a.col_of[r0 + i];
  double acc = 0.0;
  for (uint32_t q = 0; q < a.n; ++q) {
    if (q == r) continue;
    const uint32_t j = a.pos[(size_t)q * a.len + c];
    const row_ref rr = mp_row(a.mp, x, a.seq[q], i);
    double term;
    if (j != DAFS_HIP_NONE) {  // the stored probability of (i, j), 0 when the pair is not stored
      float v = 0.0f;
      for (uint32_t k = 0; k < rr.n; ++k)
        if (rr.col[k] == j) v = rr.val[k];
      term = (double)v;
    } else {  // a gap opposite i: correct with the probability that i matches nothing in y
      double mass = 0.0;
      for (uint32_t k = 0; k < rr.n; ++k) mass += (double)rr.val[k];
      const double t = 1.0 - mass;
      term = t > 0.0 ? t : 0.0;
    }
    acc += term;
  }
  a.res_rel[r0 + i] = a.n > 1 ? acc / (double)(a.n - 1) : 1.0;
}

// One thread per column: col(c) and, with a structure, the consensus-pair value at the pair's left column.
__global__ __launch_bounds__(256) void k_rel_column(rel_args a) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= a.len) return;
  double s = 0.0;
  uint32_t cnt = 0;
  for (uint32_t r = 0; r < a.n; ++r) {
    const uint32_t i = a.pos[(size_t)r * a.len + c];
    if (i != DAFS_HIP_NONE) { s += a.res_rel[a.res_off[r] + i]; ++cnt; }
  }
  a.col_rel[c] = cnt ? s / (double)cnt : 0.0;
  double ps = 0.0;
  uint32_t pc = 0;
  const uint32_t c2 = a.ss ? a.ss[c] : DAFS_HIP_NONE;
  if (c2 != DAFS_HIP_NONE) {
    for (uint32_t r = 0; r < a.n; ++r) {
      const uint32_t i = a.pos[(size_t)r * a.len + c], j = a.pos[(size_t)r * a.len + c2];
      if (i == DAFS_HIP_NONE || j == DAFS_HIP_NONE) continue;
      const row_ref br = bp_row(a.bp, a.seq[r], i);
      float v = 0.0f;
      for (uint32_t k = 0; k < br.n; ++k)
        if (br.col[k] == j) v = br.val[k];
      ps += (double)v;
      ++pc;
    }
  }
  a.pair_rel[c] = pc ? ps / (double)pc : 0.0;
  a.pair_rows[c] = pc;
}

int rel_launch(const rel_args& a, const uint8_t* mask, hipStream_t st) {
  if (!a.n || !a.len) return DAFS_HIP_EINVAL;
  STAGE_LAUNCH(ST_REL_POS, st) hipLaunchKernelGGL(k_rel_pos, dim3(a.n), dim3(64), 0, st, mask, a.len, a.res_off, a.pos, a.col_of);
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  if (a.nblocks) {
    STAGE_LAUNCH(ST_REL_RESIDUE, st) hipLaunchKernelGGL(k_rel_residue, dim3((a.nblocks + 3) / 4), dim3(256), 0, st, a);
    if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  }
  STAGE_LAUNCH(ST_REL_COLUMN, st) hipLaunchKernelGGL(k_rel_column, dim3((a.len + 255) / 256), dim3(256), 0, st, a);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

}  // namespace dafs
