// dafs_amd/csrc/pairwise.hip -- the two-sequence families of an all-against-all pairwise run, built on the device from one
// N-sequence phase 1 (dafs_hip_pairs_from, include/dafs_hip.h).  The base-pairing rows of a sequence
// do not depend on its partner and the pair kernels' result for (x, y) does not depend on the batch, so the P families
// [x, y] need no recomputation: their stores are gathers by pair index out of the source's -- the gather of families.hip
// with the members x, y of family p at rows 2p and 2p + 1.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

#include "../../include/dafs_hip.h"
#include "ctx.h"
#include "families.h"
#include "hip_util.h"

using namespace dafs;

extern "C" int dafs_hip_pairs_from(dafs_hip_ctx* dst, const dafs_hip_ctx* src, uint32_t npairs, const uint32_t* pair_x, const uint32_t* pair_y) {
  if (!dst || !src || dst == src || npairs == 0 || !pair_x || !pair_y || dst->device != src->device) return DAFS_HIP_EINVAL;
  const uint32_t n = (uint32_t)src->len.size();
  const mp_store& smp = src->mp[0];
  const bp_store& sbp = src->bp[0];
  // one family of N >= 2 sequences with both raw stores complete: base-pairing rows of every sequence, matching rows and
  // scores of every pair (a shard of align_posteriors holds some pairs only)
  if (n < 2 || src->fam.nfam() != 1 || src->fold_pending || dst->fold_pending) return DAFS_HIP_EINVAL;
  if (!smp.valid || smp.n_tasks != src->fam.npairs() || src->sim.empty() || !sbp.valid) return DAFS_HIP_EINVAL;
  if (npairs > 0x7FFFFFFFu) return DAFS_HIP_EOVERFLOW;  // the 2P sequence indices are 32-bit
  for (uint32_t p = 0; p < npairs; ++p)
    if (pair_x[p] >= pair_y[p] || pair_y[p] >= n) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(dst->device))) return DAFS_HIP_ENODEV;
  std::vector<uint32_t> first((size_t)npairs + 1), member(2 * (size_t)npairs);
  for (uint32_t p = 0; p < npairs; ++p) {
    first[p] = 2 * p;
    member[2 * p] = pair_x[p]; member[2 * p + 1] = pair_y[p];
  }
  first[npairs] = 2 * npairs;
  return families_gather(dst, src, npairs, first.data(), member.data());
}
