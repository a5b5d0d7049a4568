// dafs_amd/csrc/families.hip -- families over arbitrary subsets of the sequences of one N-sequence phase 1, built on the
// device (dafs_hip_families_from, include/dafs_hip.h).  The base-pairing rows of a sequence do not depend
// on its family and the pair kernels' result for (x, y) does not depend on the batch, so a family whose members ascend needs
// no recomputation: a dst pair (a < b) is the src pair (x < y) in the same orientation, and its stores are gathers by pair
// index out of the source's.  Index work only, like store_dev.hip: no arithmetic on the probabilities, every copy device to
// device.  dafs_hip_pairs_from (pairwise.hip) is the case of two-member families and runs through the same gather.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "../../include/dafs_hip.h"
#include "ctx.h"
#include "families.h"
#include "hip_util.h"
#include "store_dev.h"

namespace dafs {

// thread k < np: dst pair k = (a, b), the source pair (member[a], member[b]) (row-major pair id x N - x (x + 1) / 2 + y - x - 1
// of the one-family source): its task, entry count and similarity score; thread k < m: dst sequence k, the source sequence
// member[k]: its base-pairing entry count
__global__ __launch_bounds__(256) void k_fam_index(const uint32_t* __restrict__ pair_a, const uint32_t* __restrict__ pair_b, uint32_t np,
                                                   const uint32_t* __restrict__ member, uint32_t m, uint32_t nsrc,
                                                   const uint32_t* __restrict__ src_task_of_pair, const uint32_t* __restrict__ src_pair_nnz,
                                                   const float* __restrict__ src_sim, const uint32_t* __restrict__ src_bp_nnz, uint32_t* __restrict__ task,
                                                   uint32_t* __restrict__ pair_nnz, float* __restrict__ sim, uint32_t* __restrict__ bp_nnz) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < np) {
    const uint32_t x = member[pair_a[k]], y = member[pair_b[k]];
    const uint64_t id = (uint64_t)x * nsrc - (uint64_t)x * (x + 1) / 2 + (y - x - 1);
    const uint32_t t = src_task_of_pair[id];
    task[k] = t;
    pair_nnz[k] = src_pair_nnz[t];
    sim[k] = src_sim[t];
  }
  if (k < m) bp_nnz[k] = src_bp_nnz[member[k]];
}

// block p: pair p's row pointers (len a + 1 of mp[a][b], then len b + 1 of mp[b][a]; relative to the pair, so they copy as
// they are) and its 2 * nnz entries, from the source task's place to the pair's
__global__ __launch_bounds__(256) void k_fam_mp_gather(const uint32_t* __restrict__ task, const uint32_t* __restrict__ pair_a, const uint32_t* __restrict__ pair_b,
                                                       const uint32_t* __restrict__ len, const uint64_t* __restrict__ src_rp_off,
                                                       const uint64_t* __restrict__ src_pair_off, const uint32_t* __restrict__ src_rowptr,
                                                       const uint32_t* __restrict__ src_col, const float* __restrict__ src_val,
                                                       const uint32_t* __restrict__ pair_nnz, const uint64_t* __restrict__ rp_off,
                                                       const uint64_t* __restrict__ pair_off, uint32_t* __restrict__ rowptr, uint32_t* __restrict__ col,
                                                       float* __restrict__ val) {
  const uint32_t p = blockIdx.x, t = task[p];
  const uint32_t nrp = len[pair_a[p]] + len[pair_b[p]] + 2;
  const uint32_t* rs = src_rowptr + src_rp_off[t];
  uint32_t* rd = rowptr + rp_off[p];
  for (uint32_t k = threadIdx.x; k < nrp; k += blockDim.x) rd[k] = rs[k];
  const uint64_t s = src_pair_off[t], d = pair_off[p], n2 = 2ull * pair_nnz[p];
  for (uint64_t e = threadIdx.x; e < n2; e += blockDim.x) { col[d + e] = src_col[s + e]; val[d + e] = src_val[s + e]; }
}

// block s: dst sequence s, source sequence x = member[s]: its len x + 1 row pointers (relative to its first entry) and its entries
__global__ __launch_bounds__(256) void k_fam_bp_gather(const uint32_t* __restrict__ member, const uint32_t* __restrict__ src_len,
                                                       const uint64_t* __restrict__ src_rp_off, const uint64_t* __restrict__ src_bp_off,
                                                       const uint32_t* __restrict__ src_rowptr, const uint32_t* __restrict__ src_col,
                                                       const float* __restrict__ src_val, const uint32_t* __restrict__ nnz, const uint64_t* __restrict__ rp_off,
                                                       const uint64_t* __restrict__ bp_off, uint32_t* __restrict__ rowptr, uint32_t* __restrict__ col,
                                                       float* __restrict__ val) {
  const uint32_t s = blockIdx.x, x = member[s];
  const uint32_t nrp = src_len[x] + 1;
  const uint32_t* rs = src_rowptr + src_rp_off[x];
  uint32_t* rd = rowptr + rp_off[s];
  for (uint32_t k = threadIdx.x; k < nrp; k += blockDim.x) rd[k] = rs[k];
  const uint64_t a = src_bp_off[x], b = bp_off[s], n = nnz[s];
  for (uint64_t e = threadIdx.x; e < n; e += blockDim.x) { col[b + e] = src_col[a + e]; val[b + e] = src_val[a + e]; }
}

int families_gather(dafs_hip_ctx* dst, const dafs_hip_ctx* src, uint32_t nfam, const uint32_t* first, const uint32_t* member) {
  const uint32_t n = (uint32_t)src->len.size();
  const uint32_t m = first[nfam];
  const mp_store& smp = src->mp[0];
  const bp_store& sbp = src->bp[0];
  int rc;
  {  // the m sequences and the nfam families (what dafs_hip_set_sequences + dafs_hip_set_families leave)
    std::vector<const char*> seqs(m);
    std::vector<uint32_t> lens(m);
    for (uint32_t s = 0; s < m; ++s) { seqs[s] = src->seq.data() + src->off[member[s]]; lens[s] = src->len[member[s]]; }
    if ((rc = dafs_hip_set_sequences(dst, m, seqs.data(), lens.data()))) return rc;
    if (nfam > 1 && (rc = dafs_hip_set_families(dst, nfam, first))) return rc;
  }
  const uint32_t np = (uint32_t)dst->fam.npairs();
  mp_store& mp = dst->mp[0];
  bp_store& bp = dst->bp[0];
  // host tables of the matching store: the pairs family by family, row-major inside (family_layout::pairs); pair p is task
  // p, its row pointers follow those of pair p - 1
  mp.pair_x.resize(np); mp.pair_y.resize(np); mp.task_of_pair.resize(np); mp.rp_by_pair.resize(np);
  dst->fam.pairs(0, np, mp.pair_x.data(), mp.pair_y.data());
  uint64_t rp_total = 0;
  for (uint32_t p = 0; p < np; ++p) {
    mp.task_of_pair[p] = p;
    mp.rp_by_pair[p] = rp_total;
    rp_total += (uint64_t)dst->len[mp.pair_x[p]] + 1 + dst->len[mp.pair_y[p]] + 1;
  }
  mp.n_tasks = np;
  mp.rp_total = rp_total;
  mp.listed = false;
  if ((rc = mp.rowptr_pool.reserve(rp_total))) return rc;
  if ((rc = mp.pair_nnz.reserve(np))) return rc;
  if ((rc = mp.pair_off.reserve((size_t)np + 1))) return rc;
  if ((rc = mp.rp_off.upload(mp.rp_by_pair.data(), np, dst->stream))) return rc;
  if ((rc = mp.d_task_of_pair.upload(mp.task_of_pair.data(), np, dst->stream))) return rc;
  if ((rc = dst->d_pair_x.upload(mp.pair_x.data(), np, dst->stream))) return rc;
  if ((rc = dst->d_pair_y.upload(mp.pair_y.data(), np, dst->stream))) return rc;
  if ((rc = dst->task_sim.reserve(np))) return rc;
  if ((rc = bp.rowptr.reserve(dst->seq_rp_off[m]))) return rc;
  if ((rc = bp.nnz.reserve(m))) return rc;
  if ((rc = bp.bp_off.reserve((size_t)m + 1))) return rc;
  if ((rc = bp.rp_off.upload(dst->seq_rp_off.data(), (size_t)m + 1, dst->stream))) return rc;
  // the member list and each pair's source task
  if ((rc = dst->work.reserve(((size_t)m + np) * 4 + 64))) return rc;
  uint32_t* d_member = (uint32_t*)dst->work.ptr;
  uint32_t* d_task = d_member + m;
  if (hip_check(hipMemcpyAsync(d_member, member, (size_t)m * 4, hipMemcpyHostToDevice, dst->stream))) return DAFS_HIP_ELAUNCH;
  hipLaunchKernelGGL(k_fam_index, dim3((std::max(np, m) + 255) / 256), dim3(256), 0, dst->stream, dst->d_pair_x.ptr, dst->d_pair_y.ptr, np, d_member, m, n,
                     smp.d_task_of_pair.ptr, smp.pair_nnz.ptr, src->task_sim.ptr, sbp.nnz.ptr, d_task, mp.pair_nnz.ptr, dst->task_sim.ptr, bp.nnz.ptr);
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  // first entries: one scan over the per-pair counts (2 nnz: both directions), one over the per-sequence counts
  if ((rc = scan_excl_launch(mp.pair_nnz.ptr, 2u, mp.pair_off.ptr, np, dst->stream))) return rc;
  if ((rc = scan_excl_launch(bp.nnz.ptr, 1u, bp.bp_off.ptr, m, dst->stream))) return rc;
  uint64_t mp_total = 0, bp_total = 0;
  if (hip_check(hipMemcpyAsync(&mp_total, mp.pair_off.ptr + np, sizeof mp_total, hipMemcpyDeviceToHost, dst->stream)) ||
      hip_check(hipMemcpyAsync(&bp_total, bp.bp_off.ptr + m, sizeof bp_total, hipMemcpyDeviceToHost, dst->stream)) ||
      hip_check(hipStreamSynchronize(dst->stream)))
    return DAFS_HIP_ELAUNCH;
  if ((rc = mp.col.reserve(mp_total + 1))) return rc;
  if ((rc = mp.val.reserve(mp_total + 1))) return rc;
  if ((rc = bp.col.reserve(bp_total + 1))) return rc;
  if ((rc = bp.val.reserve(bp_total + 1))) return rc;
  if (np) {  // families of one sequence have no pair
    hipLaunchKernelGGL(k_fam_mp_gather, dim3(np), dim3(256), 0, dst->stream, d_task, dst->d_pair_x.ptr, dst->d_pair_y.ptr, dst->d_len.ptr, smp.rp_off.ptr,
                       smp.pair_off.ptr, smp.rowptr_pool.ptr, smp.col.ptr, smp.val.ptr, mp.pair_nnz.ptr, mp.rp_off.ptr, mp.pair_off.ptr, mp.rowptr_pool.ptr,
                       mp.col.ptr, mp.val.ptr);
    if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  }
  hipLaunchKernelGGL(k_fam_bp_gather, dim3(m), dim3(256), 0, dst->stream, d_member, src->d_len.ptr, sbp.rp_off.ptr, sbp.bp_off.ptr, sbp.rowptr.ptr, sbp.col.ptr,
                     sbp.val.ptr, bp.nnz.ptr, bp.rp_off.ptr, bp.bp_off.ptr, bp.rowptr.ptr, bp.col.ptr, bp.val.ptr);
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  // the similarity blocks: unit diagonals, s_xy of the family's pairs
  const size_t nsim = (size_t)dst->fam.sim_floats();
  if ((rc = dst->d_sim.reserve(nsim))) return rc;
  if (hip_check(hipMemsetAsync(dst->d_sim.ptr, 0, nsim * sizeof(float), dst->stream))) return DAFS_HIP_ELAUNCH;
  if ((rc = sim_matrix_launch(dst->d_pair_x.ptr, dst->d_pair_y.ptr, dst->task_sim.ptr, np, dst->fam.d_seq.ptr, m, dst->d_sim.ptr, dst->stream))) return rc;
  dst->sim.assign(nsim, 0.0f);
  if (hip_check(hipMemcpyAsync(dst->sim.data(), dst->d_sim.ptr, nsim * sizeof(float), hipMemcpyDeviceToHost, dst->stream)) ||
      hip_check(hipStreamSynchronize(dst->stream)))
    return DAFS_HIP_ELAUNCH;
  mp.pool_used = mp_total;
  mp.pool_cap_hint = std::max<uint64_t>(mp.pool_cap_hint, mp_total);
  mp.valid = true;
  bp.total_nnz = bp_total;
  bp.valid = true;
  dst->cur_mp = dst->cur_bp = 0;
  return DAFS_HIP_OK;
}

}  // namespace dafs

using namespace dafs;

extern "C" int dafs_hip_families_from(dafs_hip_ctx* dst, const dafs_hip_ctx* src, uint32_t nfam, const uint32_t* first, const uint32_t* member) {
  if (!dst || !src || dst == src || nfam == 0 || !first || !member || dst->device != src->device) return DAFS_HIP_EINVAL;
  const uint32_t n = (uint32_t)src->len.size();
  const mp_store& smp = src->mp[0];
  // one family with its raw stores: base-pairing rows of every sequence, matching rows and scores of a prefix of the pairs
  if (n == 0 || src->fam.nfam() != 1 || src->fold_pending || dst->fold_pending) return DAFS_HIP_EINVAL;
  if (!smp.valid || !src->bp[0].valid) return DAFS_HIP_EINVAL;
  if (first[0] != 0) return DAFS_HIP_EINVAL;
  const bool from0 = smp.n_tasks > 0 && smp.pair_x[0] == 0 && smp.pair_y[0] == 1;  // the store's first pair is pair 0
  uint64_t npairs = 0;
  for (uint32_t f = 0; f < nfam; ++f) {
    if (first[f + 1] <= first[f]) return DAFS_HIP_EINVAL;
    const uint32_t* mb = member + first[f];
    const uint32_t k = first[f + 1] - first[f];
    for (uint32_t a = 0; a < k; ++a)
      if (mb[a] >= n || (a && mb[a] <= mb[a - 1])) return DAFS_HIP_EINVAL;
    if (k < 2) continue;
    // the pair ids ascend with (x, y), so the family's last pair has its largest id
    const uint64_t x = mb[k - 2], y = mb[k - 1];
    if (!from0 || x * n - x * (x + 1) / 2 + (y - x - 1) >= smp.n_tasks) return DAFS_HIP_EINVAL;
    npairs += (uint64_t)k * (k - 1) / 2;
  }
  if (first[nfam] > 0x7FFFFFFFu || npairs > 0x7FFFFFFFull) return DAFS_HIP_EOVERFLOW;  // sequence and pair indices are 32-bit
  if (hip_check(hipSetDevice(dst->device))) return DAFS_HIP_ENODEV;
  return families_gather(dst, src, nfam, first, member);
}
