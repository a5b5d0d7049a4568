// dafs_amd/csrc/pairwise.hip -- the two-sequence families of an all-against-all pairwise run, built on the device from one
// N-sequence phase 1 (dafs_hip_pairs_from, include/dafs_hip.h).  The base-pairing rows of a sequence
// do not depend on its partner and the pair kernels' result for (x, y) does not depend on the batch, so the P families
// [x, y] need no recomputation: their stores are gathers by pair index out of the source's.  Index work only, like
// store_dev.hip: no arithmetic on the probabilities, every copy device to device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "../../include/dafs_hip.h"
#include "ctx.h"
#include "hip_util.h"
#include "store_dev.h"

namespace dafs {

// pair p = (x, y): the source task of (x, y) (row-major pair id x N - x (x + 1) / 2 + y - x - 1 of the one-family
// source), its entry count and similarity score; dst sequences 2p (x) and 2p + 1 (y): their base-pairing entry counts
__global__ __launch_bounds__(256) void k_pairs_index(const uint32_t* __restrict__ px, const uint32_t* __restrict__ py, uint32_t np, uint32_t nsrc,
                                                     const uint32_t* __restrict__ src_task_of_pair, const uint32_t* __restrict__ src_pair_nnz,
                                                     const float* __restrict__ src_sim, const uint32_t* __restrict__ src_bp_nnz, uint32_t* __restrict__ task,
                                                     uint32_t* __restrict__ pair_nnz, float* __restrict__ sim, uint32_t* __restrict__ bp_nnz) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= np) return;
  const uint32_t x = px[p], y = py[p];
  const uint64_t id = (uint64_t)x * nsrc - (uint64_t)x * (x + 1) / 2 + (y - x - 1);
  const uint32_t t = src_task_of_pair[id];
  task[p] = t;
  pair_nnz[p] = src_pair_nnz[t];
  sim[p] = src_sim[t];
  bp_nnz[2 * p] = src_bp_nnz[x];
  bp_nnz[2 * p + 1] = src_bp_nnz[y];
}

// block p: pair p's row pointers (len x + 1 of mp[x][y], then len y + 1 of mp[y][x]; relative to the pair, so they copy as
// they are) and its 2 * nnz entries, from the source task's place to the pair's
__global__ __launch_bounds__(256) void k_pairs_mp_gather(const uint32_t* __restrict__ task, const uint32_t* __restrict__ len, const uint64_t* __restrict__ src_rp_off,
                                                         const uint64_t* __restrict__ src_pair_off, const uint32_t* __restrict__ src_rowptr,
                                                         const uint32_t* __restrict__ src_col, const float* __restrict__ src_val,
                                                         const uint32_t* __restrict__ pair_nnz, const uint64_t* __restrict__ rp_off,
                                                         const uint64_t* __restrict__ pair_off, uint32_t* __restrict__ rowptr, uint32_t* __restrict__ col,
                                                         float* __restrict__ val) {
  const uint32_t p = blockIdx.x, t = task[p];
  const uint32_t nrp = len[2 * p] + len[2 * p + 1] + 2;
  const uint32_t* rs = src_rowptr + src_rp_off[t];
  uint32_t* rd = rowptr + rp_off[p];
  for (uint32_t k = threadIdx.x; k < nrp; k += blockDim.x) rd[k] = rs[k];
  const uint64_t s = src_pair_off[t], d = pair_off[p], n2 = 2ull * pair_nnz[p];
  for (uint64_t e = threadIdx.x; e < n2; e += blockDim.x) { col[d + e] = src_col[s + e]; val[d + e] = src_val[s + e]; }
}

// block s: dst sequence s, source sequence x: its len x + 1 row pointers (relative to its first entry) and its entries
__global__ __launch_bounds__(256) void k_pairs_bp_gather(const uint32_t* __restrict__ px, const uint32_t* __restrict__ py, const uint32_t* __restrict__ src_len,
                                                         const uint64_t* __restrict__ src_rp_off, const uint64_t* __restrict__ src_bp_off,
                                                         const uint32_t* __restrict__ src_rowptr, const uint32_t* __restrict__ src_col,
                                                         const float* __restrict__ src_val, const uint32_t* __restrict__ nnz, const uint64_t* __restrict__ rp_off,
                                                         const uint64_t* __restrict__ bp_off, uint32_t* __restrict__ rowptr, uint32_t* __restrict__ col,
                                                         float* __restrict__ val) {
  const uint32_t s = blockIdx.x, x = (s & 1) ? py[s >> 1] : px[s >> 1];
  const uint32_t nrp = src_len[x] + 1;
  const uint32_t* rs = src_rowptr + src_rp_off[x];
  uint32_t* rd = rowptr + rp_off[s];
  for (uint32_t k = threadIdx.x; k < nrp; k += blockDim.x) rd[k] = rs[k];
  const uint64_t a = src_bp_off[x], b = bp_off[s], n = nnz[s];
  for (uint64_t e = threadIdx.x; e < n; e += blockDim.x) { col[b + e] = src_col[a + e]; val[b + e] = src_val[a + e]; }
}

}  // namespace dafs

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
  const uint32_t m = 2 * npairs;
  int rc;
  {  // the 2P sequences and the P families [2p, 2p + 1] (what dafs_hip_set_sequences + dafs_hip_set_families leave)
    std::vector<const char*> seqs(m);
    std::vector<uint32_t> lens(m), first(npairs + 1);
    for (uint32_t p = 0; p < npairs; ++p) {
      const uint32_t x = pair_x[p], y = pair_y[p];
      seqs[2 * p] = src->seq.data() + src->off[x]; lens[2 * p] = src->len[x];
      seqs[2 * p + 1] = src->seq.data() + src->off[y]; lens[2 * p + 1] = src->len[y];
      first[p] = 2 * p;
    }
    first[npairs] = m;
    if ((rc = dafs_hip_set_sequences(dst, m, seqs.data(), lens.data()))) return rc;
    if (npairs > 1 && (rc = dafs_hip_set_families(dst, npairs, first.data()))) return rc;
  }
  mp_store& mp = dst->mp[0];
  bp_store& bp = dst->bp[0];
  // host tables of the matching store: pair p is (2p, 2p + 1) and task p; its row pointers follow those of pair p - 1
  mp.pair_x.resize(npairs); mp.pair_y.resize(npairs); mp.task_of_pair.resize(npairs); mp.rp_by_pair.resize(npairs);
  uint64_t rp_total = 0;
  for (uint32_t p = 0; p < npairs; ++p) {
    mp.pair_x[p] = 2 * p; mp.pair_y[p] = 2 * p + 1; mp.task_of_pair[p] = p;
    mp.rp_by_pair[p] = rp_total;
    rp_total += (uint64_t)dst->len[2 * p] + 1 + dst->len[2 * p + 1] + 1;
  }
  mp.n_tasks = npairs;
  mp.rp_total = rp_total;
  if ((rc = mp.rowptr_pool.reserve(rp_total))) return rc;
  if ((rc = mp.pair_nnz.reserve(npairs))) return rc;
  if ((rc = mp.pair_off.reserve((size_t)npairs + 1))) return rc;
  if ((rc = mp.rp_off.upload(mp.rp_by_pair.data(), npairs, dst->stream))) return rc;
  if ((rc = mp.d_task_of_pair.upload(mp.task_of_pair.data(), npairs, dst->stream))) return rc;
  if ((rc = dst->d_pair_x.upload(mp.pair_x.data(), npairs, dst->stream))) return rc;
  if ((rc = dst->d_pair_y.upload(mp.pair_y.data(), npairs, dst->stream))) return rc;
  if ((rc = dst->task_sim.reserve(npairs))) return rc;
  if ((rc = bp.rowptr.reserve(dst->seq_rp_off[m]))) return rc;
  if ((rc = bp.nnz.reserve(m))) return rc;
  if ((rc = bp.bp_off.reserve((size_t)m + 1))) return rc;
  if ((rc = bp.rp_off.upload(dst->seq_rp_off.data(), (size_t)m + 1, dst->stream))) return rc;
  // the pair list and each pair's source task
  if ((rc = dst->work.reserve((size_t)npairs * 12 + 64))) return rc;
  uint32_t* d_px = (uint32_t*)dst->work.ptr;
  uint32_t* d_py = d_px + npairs;
  uint32_t* d_task = d_py + npairs;
  if (hip_check(hipMemcpyAsync(d_px, pair_x, (size_t)npairs * 4, hipMemcpyHostToDevice, dst->stream)) ||
      hip_check(hipMemcpyAsync(d_py, pair_y, (size_t)npairs * 4, hipMemcpyHostToDevice, dst->stream)))
    return DAFS_HIP_ELAUNCH;
  hipLaunchKernelGGL(k_pairs_index, dim3((npairs + 255) / 256), dim3(256), 0, dst->stream, d_px, d_py, npairs, n, smp.d_task_of_pair.ptr, smp.pair_nnz.ptr,
                     src->task_sim.ptr, sbp.nnz.ptr, d_task, mp.pair_nnz.ptr, dst->task_sim.ptr, bp.nnz.ptr);
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  // first entries: one scan over the per-pair counts (2 nnz: both directions), one over the per-sequence counts
  if ((rc = scan_excl_launch(mp.pair_nnz.ptr, 2u, mp.pair_off.ptr, npairs, dst->stream))) return rc;
  if ((rc = scan_excl_launch(bp.nnz.ptr, 1u, bp.bp_off.ptr, m, dst->stream))) return rc;
  uint64_t mp_total = 0, bp_total = 0;
  if (hip_check(hipMemcpyAsync(&mp_total, mp.pair_off.ptr + npairs, sizeof mp_total, hipMemcpyDeviceToHost, dst->stream)) ||
      hip_check(hipMemcpyAsync(&bp_total, bp.bp_off.ptr + m, sizeof bp_total, hipMemcpyDeviceToHost, dst->stream)) ||
      hip_check(hipStreamSynchronize(dst->stream)))
    return DAFS_HIP_ELAUNCH;
  if ((rc = mp.col.reserve(mp_total + 1))) return rc;
  if ((rc = mp.val.reserve(mp_total + 1))) return rc;
  if ((rc = bp.col.reserve(bp_total + 1))) return rc;
  if ((rc = bp.val.reserve(bp_total + 1))) return rc;
  hipLaunchKernelGGL(k_pairs_mp_gather, dim3(npairs), dim3(256), 0, dst->stream, d_task, dst->d_len.ptr, smp.rp_off.ptr, smp.pair_off.ptr, smp.rowptr_pool.ptr,
                     smp.col.ptr, smp.val.ptr, mp.pair_nnz.ptr, mp.rp_off.ptr, mp.pair_off.ptr, mp.rowptr_pool.ptr, mp.col.ptr, mp.val.ptr);
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  hipLaunchKernelGGL(k_pairs_bp_gather, dim3(m), dim3(256), 0, dst->stream, d_px, d_py, src->d_len.ptr, sbp.rp_off.ptr, sbp.bp_off.ptr, sbp.rowptr.ptr,
                     sbp.col.ptr, sbp.val.ptr, bp.nnz.ptr, bp.rp_off.ptr, bp.bp_off.ptr, bp.rowptr.ptr, bp.col.ptr, bp.val.ptr);
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  // the similarity blocks [[1, s_xy], [s_xy, 1]]
  const size_t nsim = (size_t)dst->fam.sim_floats();
  if ((rc = dst->d_sim.reserve(nsim))) return rc;
  if (hip_check(hipMemsetAsync(dst->d_sim.ptr, 0, nsim * sizeof(float), dst->stream))) return DAFS_HIP_ELAUNCH;
  if ((rc = sim_matrix_launch(dst->d_pair_x.ptr, dst->d_pair_y.ptr, dst->task_sim.ptr, npairs, dst->fam.d_seq.ptr, m, dst->d_sim.ptr, dst->stream))) return rc;
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
