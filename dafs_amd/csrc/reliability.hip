// dafs_amd/csrc/reliability.hip -- per-residue alignment reliability from the sparse stores a run already holds, for the
// many alignments of a chunk in three launches (dafs_hip_alignment_reliabilities, capi_reliability.cpp; definitions in
// DESIGN.md "Alignment reliability", the batch in section 17).
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

// One wavefront per row of the chunk, 64 columns per step: pos[cell] = residue index of the row at that column
// (DAFS_HIP_NONE for a gap) and col_of[res0 + i] = column of residue i.  The mask has been checked to place exactly len[x]
// residues.
__global__ __launch_bounds__(64) void k_rel_pos(rel_args a) {
  const uint32_t r = blockIdx.x, lane = threadIdx.x;
  const rel_row row = a.rows[r];
  const rel_aln al = a.alns[row.aln];
  const uint32_t len = al.len;
  const size_t cell = al.cell0 + (size_t)(r - al.row0) * len;
  const uint8_t* m = a.mask + cell;
  uint32_t* pr = a.pos + cell;
  uint32_t* co = a.col_of + row.res0;
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

// One wavefront per block of 64 consecutive residues of one wanted row; lane t owns residue i0 + t and walks the other rows
// of its alignment in order.  For each row q the lanes read adjacent row pointers of one matrix and then its adjacent rows
// (mp_row).
__global__ __launch_bounds__(256) void k_rel_residue(rel_args a) {
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= a.nblocks) return;
  const uint2 blk = a.blocks[w];
  const uint32_t r = blk.x, i = blk.y + (threadIdx.x & 63);
  const rel_row row = a.rows[r];
  const uint32_t x = row.seq;
  if (i >= row.nres) return;
  const rel_aln al = a.alns[row.aln];
  const uint32_t c = a.col_of[row.res0 + i];
  const uint32_t* pos = a.pos + al.cell0 + c;
  const uint32_t self = r - (uint32_t)al.row0;
  double acc = 0.0;
  for (uint32_t q = 0; q < al.n; ++q) {
    if (q == self) continue;
    const uint32_t j = pos[(size_t)q * al.len];
    const row_ref rr = mp_row(a.mp, x, a.rows[al.row0 + q].seq, i);
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
  a.res_rel[row.rel0 + i] = al.n > 1 ? acc / (double)(al.n - 1) : 1.0;
}

// One wavefront per block of 64 columns of one alignment, one thread per column: col(c) and, with a structure, the
// consensus-pair value at the pair's left column.  col(c) of an alignment with a row that is not wanted is NaN.
__global__ __launch_bounds__(256) void k_rel_column(rel_args a) {
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= a.ncol_blocks) return;
  const uint2 blk = a.col_blocks[w];
  const rel_aln al = a.alns[blk.x];
  const uint32_t c = blk.y + (threadIdx.x & 63);
  if (c >= al.len) return;
  const uint32_t* pos = a.pos + al.cell0;
  const rel_row* rows = a.rows + al.row0;
  if (al.all_wanted) {
    double s = 0.0;
    uint32_t cnt = 0;
    for (uint32_t r = 0; r < al.n; ++r) {
      const uint32_t i = pos[(size_t)r * al.len + c];
      if (i != DAFS_HIP_NONE) { s += a.res_rel[rows[r].rel0 + i]; ++cnt; }
    }
    a.col_rel[al.col0 + c] = cnt ? s / (double)cnt : 0.0;
  } else {
    a.col_rel[al.col0 + c] = __longlong_as_double(0x7ff8000000000000ll);
  }
  double ps = 0.0;
  uint32_t pc = 0;
  const uint32_t c2 = a.ss ? a.ss[al.col0 + c] : DAFS_HIP_NONE;
  if (c2 != DAFS_HIP_NONE) {
    for (uint32_t r = 0; r < al.n; ++r) {
      const uint32_t i = pos[(size_t)r * al.len + c], j = pos[(size_t)r * al.len + c2];
      if (i == DAFS_HIP_NONE || j == DAFS_HIP_NONE) continue;
      const row_ref br = bp_row(a.bp, rows[r].seq, i);
      float v = 0.0f;
      for (uint32_t k = 0; k < br.n; ++k)
        if (br.col[k] == j) v = br.val[k];
      ps += (double)v;
      ++pc;
    }
  }
  a.pair_rel[al.col0 + c] = pc ? ps / (double)pc : 0.0;
  a.pair_rows[al.col0 + c] = pc;
}

int rel_launch(const rel_args& a, hipStream_t st) {
  if (!a.nrows || !a.ncol_blocks) return DAFS_HIP_EINVAL;
  STAGE_LAUNCH(ST_REL_POS, st) hipLaunchKernelGGL(k_rel_pos, dim3(a.nrows), dim3(64), 0, st, a);
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  if (a.nblocks) {
    STAGE_LAUNCH(ST_REL_RESIDUE, st) hipLaunchKernelGGL(k_rel_residue, dim3((a.nblocks + 3) / 4), dim3(256), 0, st, a);
    if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  }
  STAGE_LAUNCH(ST_REL_COLUMN, st) hipLaunchKernelGGL(k_rel_column, dim3((a.ncol_blocks + 3) / 4), dim3(256), 0, st, a);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

}  // namespace dafs
