// dafs_amd/csrc/support.hip -- how far each row of an alignment keeps a given structure (dafs_hip_structure_support,
// capi_support.cpp; definitions in DESIGN.md section 16).
//
// Per row r (sequence x) and pair c1 -> c2 of the structure, with i, j the residues of r at the two columns: `both` counts the
// pairs whose two residues the row holds, `canonical` those of them CONTRAfold can pair, `half` the pairs with exactly one
// residue, and `expected` is the sum of bp[x](i, j) over the `both` pairs, each term widened to double and added in ascending
// c1.  The counts are popcounts of ballots; the sum is taken by one lane from the terms its wavefront has laid down in column
// order, so neither depends on the launch geometry: no cross-lane floating-point reduction and no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/dafs_hip.h"
#include "hip_util.h"
#include "stage.h"
#include "support.h"

namespace dafs {

// CONTRAfold's alphabet is "ACGU" (class codes 0..3; T, N and the rest are its symbol 4) and it pairs AU, GU, CG (cf_comp)
__device__ __forceinline__ bool sup_comp(uint32_t a, uint32_t b) {
  return (a == 0 && b == 3) || (a == 3 && b == 0) || (a == 2 && b == 3) || (a == 3 && b == 2) || (a == 1 && b == 2) || (a == 2 && b == 1);
}

// One wavefront per row, 64 columns per step.  First the column -> residue map by ballot and popcount (as k_rel_pos), then
// the pairs: lane t looks at column c0 + t as a left column.
__global__ __launch_bounds__(64) void k_ss_support(sup_args a) {
  __shared__ double terms[64];
  const uint32_t r = blockIdx.x, lane = threadIdx.x;
  const sup_row row = a.rows[r];
  const uint8_t* m = a.mask + row.mask_off;
  uint32_t* pos = a.pos + row.pos_off;
  const uint32_t* ss = a.ss + row.ss_off;
  const uint8_t* code = a.codes + row.code_off;
  uint32_t run = 0;
  for (uint32_t c0 = 0; c0 < row.len; c0 += 64) {
    const uint32_t c = c0 + lane;
    const bool res = c < row.len && m[c] != 0;
    const uint64_t b = __ballot(res);
    if (c < row.len) pos[c] = res ? run + (uint32_t)__popcll(b & ((1ull << lane) - 1ull)) : DAFS_HIP_NONE;
    run += (uint32_t)__popcll(b);
  }
  __syncthreads();  // one wavefront: the map is written before any lane reads a partner's entry
  uint32_t n_both = 0, n_can = 0, n_half = 0;
  double acc = 0.0;
  for (uint32_t c0 = 0; c0 < row.len; c0 += 64) {
    const uint32_t c = c0 + lane;
    const uint32_t c2 = c < row.len ? ss[c] : DAFS_HIP_NONE;
    bool both = false, half = false, can = false;
    double term = 0.0;
    if (c2 != DAFS_HIP_NONE) {
      const uint32_t i = pos[c], j = pos[c2];
      both = i != DAFS_HIP_NONE && j != DAFS_HIP_NONE;
      half = (i != DAFS_HIP_NONE) != (j != DAFS_HIP_NONE);
      if (both) {
        can = sup_comp(code[i], code[j]);
        const row_ref br = bp_row(a.bp, row.seq, i);
        float v = 0.0f;  // the stored probability of (i, j), 0 when the pair is not stored
        for (uint32_t k = 0; k < br.n; ++k)
          if (br.col[k] == j) v = br.val[k];
        term = (double)v;
      }
    }
    const uint64_t bb = __ballot(both);
    n_both += (uint32_t)__popcll(bb);
    n_can += (uint32_t)__popcll(__ballot(can));
    n_half += (uint32_t)__popcll(__ballot(half));
    terms[lane] = term;
    __syncthreads();
    if (lane == 0)
      for (uint64_t rest = bb; rest; rest &= rest - 1) acc += terms[__ffsll((unsigned long long)rest) - 1];
    __syncthreads();
  }
  if (lane == 0) {
    a.both[r] = n_both;
    a.canonical[r] = n_can;
    a.half[r] = n_half;
    a.expected[r] = acc;
  }
}

int sup_launch(const sup_args& a, hipStream_t st) {
  if (!a.nrows) return DAFS_HIP_EINVAL;
  STAGE_LAUNCH(ST_SS_SUPPORT, st) hipLaunchKernelGGL(k_ss_support, dim3(a.nrows), dim3(64), 0, st, a);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

}  // namespace dafs
