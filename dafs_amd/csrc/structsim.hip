// dafs_amd/csrc/structsim.hip -- the structural score of a pair of sequences (the reference has no
// counterpart for the score, tests/structure_sim_ref.py is the plain restatement).  It is the quantity
// relax_basepairing_probability sums (reference src/dafs.cpp:349-361), reduced to one scalar per pair and taken on integers.
//
// k_struct_sim  one wavefront per task of the resident un-relaxed matching store.  The base-pair entries (i, j, p) of x are
//               dealt over the 64 lanes; a lane walks the entries (k, a) of row i and (l, b) of row j of mp[x][y] and looks l up
//               in row k of bp[y] with a binary search.  The rows of bp[y] and of mp[x][y] are copied into the wavefront's LDS
//               region first, as far as they fit: the walk gathers from them lane by lane.  Every term is a uint64, so neither
//               the dealing nor the order of the sums can change a bit: per-lane accumulators, one cross-lane integer sum, one
//               16-byte store per task.
// k_struct_w    one wavefront per sequence: W[x], the same quantisation summed over the sequence's base-pair entries.
//
// Nothing here trusts a hand-made store (dafs_hip_set_bp checks no column): an index that would leave its row pointers or
// its pool ends the term, it is never dereferenced.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dafs_hip.h"
#include "hip_util.h"
#include "stage.h"
#include "structsim.h"

namespace dafs {

namespace {

// c(v) of the contract: the stored float as a double in [0, 1]; NaN fails the first comparison and becomes 0
__device__ __forceinline__ double unit(float v) { return v > 0.0f ? (v < 1.0f ? (double)v : 1.0) : 0.0; }

// floor(d * 2^40) of a double in [0, 1]
__device__ __forceinline__ unsigned long long quant(double d) { return (unsigned long long)(d * 1099511627776.0); }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// Copies n words into the wavefront's LDS region when they still fit and returns the copy, else the source: the walk below reads
// through generic pointers and does not know which it got.
template <class T>
__device__ __forceinline__ const T* stage(const T* src, uint32_t n, uint32_t* region, uint32_t& used, uint32_t budget, uint32_t lane) {
  if (n > budget - used) return src;  // used <= budget
  T* dst = (T*)(region + used);
  for (uint32_t e = lane; e < n; e += 64) dst[e] = src[e];
  used += n;
  return dst;
}

__global__ __launch_bounds__(kStructThreads) void k_struct_sim(mp_store_dev mp, bp_store_dev bp, const uint2* __restrict__ task_xy,
                                                               uint32_t ntasks, uint32_t lds_words, ulonglong2* __restrict__ out) {
  __shared__ uint32_t lds[kStructThreads / 64][kStructLdsWords];
  const uint32_t lane = threadIdx.x & 63;
  // a spare wavefront of the last workgroup walks the last task again, for the barrier below, and stores nothing
  const uint32_t wave = blockIdx.x * (kStructThreads / 64) + (threadIdx.x >> 6);
  const uint32_t t = min(wave, ntasks - 1);
  const uint2 xy = task_xy[t];
  const uint32_t lx = mp.len[xy.x], ly = mp.len[xy.y];
  // the rows of mp[x][y]: the first len[x] + 1 row pointers of the task and its first nnz entries
  const uint32_t* rp = mp.rowptr_pool + mp.rp_off[t];
  const uint32_t* mc = mp.col + mp.pair_off[t];
  const float* mv = mp.val + mp.pair_off[t];
  const uint32_t m_nnz = mp.pair_nnz[t];
  const uint32_t* __restrict__ rpx = bp.rowptr + bp.rp_off[xy.x];
  const uint32_t* __restrict__ bcx = bp.col + bp.bp_off[xy.x];
  const float* __restrict__ bvx = bp.val + bp.bp_off[xy.x];
  const uint32_t* rpy = bp.rowptr + bp.rp_off[xy.y];
  const uint32_t* bcy = bp.col + bp.bp_off[xy.y];
  const float* bvy = bp.val + bp.bp_off[xy.y];
  const uint32_t nbx = rpx[lx], nby = rpy[ly];
  // What the inner walk gathers, lane by lane at unrelated addresses, goes into the wavefront's own LDS region first, array by
  // array while it fits (the rows of bp[y], then those of mp[x][y]); what does not fit is read where it lies.
  {
    uint32_t* region = lds[threadIdx.x >> 6];
    uint32_t used = 0;
    rpy = stage(rpy, ly + 1, region, used, lds_words, lane);
    bcy = stage(bcy, nby, region, used, lds_words, lane);
    bvy = stage(bvy, nby, region, used, lds_words, lane);
    rp = stage(rp, lx + 1, region, used, lds_words, lane);
    mc = stage(mc, m_nnz, region, used, lds_words, lane);
    mv = stage(mv, m_nnz, region, used, lds_words, lane);
  }
  __syncthreads();

  unsigned long long T = 0, terms = 0;
  for (uint32_t g = lane; g < nbx; g += 64) {
    // the row of entry g: rpx[i] <= g < rpx[i + 1] (rpx[0] = 0 <= g < nbx = rpx[lx]; empty rows are stepped over)
    uint32_t i = 0, hi = lx;
    while (hi - i > 1) {
      const uint32_t mid = (i + hi) >> 1;
      if (rpx[mid] <= g) i = mid; else hi = mid;
    }
    const uint32_t j = bcx[g];
    if (j >= lx) continue;
    const double cp = unit(bvx[g]);
    const uint32_t a0 = rp[i], a1 = min(rp[i + 1], m_nnz), b0 = rp[j], b1 = min(rp[j + 1], m_nnz);
    for (uint32_t ea = a0; ea < a1; ++ea) {
      const uint32_t k = mc[ea];
      if (k >= ly) continue;
      const uint32_t y0 = rpy[k], y1 = min(rpy[k + 1], nby);
      if (y0 >= y1) continue;
      const double ca = unit(mv[ea]);
      for (uint32_t eb = b0; eb < b1; ++eb) {
        const uint32_t l = mc[eb];
        if (l <= k) continue;  // bp[y] holds l > k only: k = l and k > l contribute nothing
        uint32_t lo = y0, up = y1;  // the first entry of row k of bp[y] whose column is >= l
        while (lo < up) {
          const uint32_t mid = (lo + up) >> 1;
          if (bcy[mid] < l) lo = mid + 1; else up = mid;
        }
        if (lo < y1 && bcy[lo] == l) {
          // two exact inner products, one rounding in the outer one, an exact scaling
          T += quant((cp * unit(bvy[lo])) * (ca * unit(mv[eb])));
          ++terms;
        }
      }
    }
  }
  T = wave_sum(T);
  terms = wave_sum(terms);
  if (lane == 0 && wave < ntasks) out[t] = make_ulonglong2(T, terms);
}

__global__ __launch_bounds__(kStructThreads) void k_struct_w(bp_store_dev bp, const uint32_t* __restrict__ len, uint32_t nseq,
                                                             unsigned long long* __restrict__ W) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t x = blockIdx.x * (kStructThreads / 64) + (threadIdx.x >> 6);
  if (x >= nseq) return;
  const uint32_t n = (bp.rowptr + bp.rp_off[x])[len[x]];
  const float* __restrict__ v = bp.val + bp.bp_off[x];
  unsigned long long w = 0;
  for (uint32_t g = lane; g < n; g += 64) w += quant(unit(v[g]));
  w = wave_sum(w);
  if (lane == 0) W[x] = w;
}

}  // namespace

int struct_sim_launch(const mp_store_dev& mp, const bp_store_dev& bp, const uint2* task_xy, uint32_t ntasks, uint32_t lds_words, ulonglong2* out,
                      hipStream_t st) {
  if (!task_xy || !out || lds_words > kStructLdsWords) return DAFS_HIP_EINVAL;
  if (ntasks == 0) return DAFS_HIP_OK;
  const uint32_t per_block = kStructThreads / 64;
  STAGE_LAUNCH(ST_STRUCT_SIM, st)
  hipLaunchKernelGGL(k_struct_sim, dim3((ntasks + per_block - 1) / per_block), dim3(kStructThreads), 0, st, mp, bp, task_xy, ntasks, lds_words, out);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

int struct_w_launch(const bp_store_dev& bp, const uint32_t* len, uint32_t nseq, unsigned long long* W, hipStream_t st) {
  if (!len || !W || nseq == 0) return DAFS_HIP_EINVAL;
  const uint32_t per_block = kStructThreads / 64;
  STAGE_LAUNCH(ST_STRUCT_W, st)
  hipLaunchKernelGGL(k_struct_w, dim3((nseq + per_block - 1) / per_block), dim3(kStructThreads), 0, st, bp, len, nseq, W);
  return hip_check(hipGetLastError()) ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;
}

}  // namespace dafs
