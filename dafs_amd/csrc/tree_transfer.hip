// dafs_amd/csrc/tree_transfer.hip -- the transfer bootstrap of the neighbour-joining tree on the device (DESIGN.md section 28;
// the reference has no counterpart, tests/transfer_ref.py is the plain restatement).  Integers only: no floating point, no
// polling, no workgroup that knows of another; every wait is a __syncthreads().
//
// The host gives every leaf a position in the walk of the main tree, rotated so that leaf 0 stands at position 0
// (tree_support.h): a non-trivial side of the main tree is then a run [lo, lo + len) of positions that never holds position 0.
//
// k_transfer_sides  ONE workgroup per replicate tree.  Per node u below the root the set of the leaves below u as bits over
//                   positions, word-major (set[word][node]), so that lanes that own consecutive nodes read consecutive
//                   addresses.  The leaves first (all threads, coalesced), then the joins in ascending order: a thread owns
//                   a word and ORs that word of the two children, which are earlier nodes, so it reads only what the leaf
//                   pass (behind a barrier) or it itself has written, and the n - 2 dependent joins need no barrier between
//                   them.  Then, threads across nodes, per word the count of set bits in the words before it (16 bits);
//                   the row behind the last word is the size of the set.  A tree that would lead an index astray (a child
//                   that is not an earlier node, a position that is not below n) is refused in the head before anything is
//                   written.
// k_transfer        a wavefront per split of the main tree, lanes stride over the nodes u of one replicate, a grid
//                   dimension over the replicates as k_boot_dist has.  |side(v) & S(u)| = rank(u, hi) - rank(u, lo) with
//                   rank(u, x) = rank[x >> 6][u] + popcount(set[x >> 6][u] & ((1 << (x & 63)) - 1)); H = len + |S(u)| - 2 *
//                   that; min(H, n - H) makes it the same for S(u) and the rest of the leaves, so nobody asks where leaf 0
//                   is.  x & 63 = 0 masks the whole word away, and its index (one past the last word when x = n) is not
//                   used.  One butterfly leaves the wavefront's minimum; a wavefront sees all nodes, so the minimum needs no
//                   atomic, and the sum over the replicates is one 64-bit integer atomicAdd per (split, replicate).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dafs_hip.h"
#include "hip_util.h"
#include "stage.h"
#include "tree_transfer.h"

namespace dafs {

namespace {

__global__ __launch_bounds__(kTransferSidesThreads) void k_transfer_sides(uint32_t n, const uint32_t* __restrict__ pos, const int32_t* __restrict__ left,
                                                                          const int32_t* __restrict__ right, transfer_head* heads, uint8_t* sets,
                                                                          size_t per_tree, size_t set_bytes) {
  __shared__ uint32_t bad_any;
  const uint32_t tid = threadIdx.x, T = 2 * n - 1, nodes = T - 1, words = (n + 63) / 64;
  left += (size_t)blockIdx.x * T;
  right += (size_t)blockIdx.x * T;
  unsigned long long* set = (unsigned long long*)(sets + (size_t)blockIdx.x * per_tree);
  uint16_t* rank = (uint16_t*)(sets + (size_t)blockIdx.x * per_tree + set_bytes);

  if (tid == 0) bad_any = 0;
  __syncthreads();
  uint32_t bad = 0;
  for (uint32_t v = tid; v < T; v += kTransferSidesThreads) {
    const int32_t l = left[v], r = right[v];
    if (v < n) bad |= (l != -1 || r != -1 || pos[v] >= n) ? 1u : 0u;
    else bad |= (l < 0 || r < 0 || (uint32_t)l >= v || (uint32_t)r >= v || l == r) ? 1u : 0u;
  }
  if (bad) atomicOr(&bad_any, 1u);
  __syncthreads();
  if (bad_any) {  // refused: nothing is written (the whole workgroup leaves)
    if (tid == 0) heads[blockIdx.x].bad_tree = 1;
    return;
  }

  // the leaves: one bit each
  for (size_t at = tid; at < (size_t)words * n; at += kTransferSidesThreads) {
    const uint32_t w = (uint32_t)(at / n), leaf = (uint32_t)(at % n), p = pos[leaf];
    set[(size_t)w * nodes + leaf] = (p >> 6) == w ? 1ull << (p & 63) : 0ull;
  }
  __syncthreads();
  // the joins below the root, ascending: this thread's words only
  for (uint32_t w = tid; w < words; w += kTransferSidesThreads) {
    unsigned long long* row = set + (size_t)w * nodes;
    for (uint32_t v = n; v < nodes; ++v) row[v] = row[(uint32_t)left[v]] | row[(uint32_t)right[v]];
  }
  __syncthreads();
  // per node the bits before each word, and the size
  for (uint32_t u = tid; u < nodes; u += kTransferSidesThreads) {
    uint32_t run = 0;
    for (uint32_t w = 0; w < words; ++w) {
      rank[(size_t)w * nodes + u] = (uint16_t)run;
      run += (uint32_t)__popcll(set[(size_t)w * nodes + u]);
    }
    rank[(size_t)words * nodes + u] = (uint16_t)run;
  }
}

__global__ __launch_bounds__(kTransferThreads) void k_transfer(uint32_t n, uint32_t splits, const transfer_split* __restrict__ split,
                                                               transfer_head* heads, const uint8_t* __restrict__ sets, size_t per_tree, size_t set_bytes,
                                                               unsigned long long* sum, int32_t* each, uint32_t kk0) {
  const uint32_t lane = threadIdx.x & 63, s = blockIdx.x * (kTransferThreads / 64) + (threadIdx.x >> 6), kk = kk0 + blockIdx.z;
  if (s >= splits || heads[kk].bad_tree) return;  // the whole wavefront leaves
  const uint32_t nodes = 2 * n - 2, words = (n + 63) / 64;
  const uint32_t lo = split[s].lo, len = split[s].len;
  if (lo < 1 || len < 2 || len > n || lo > n - len) {
    if (lane == 0) atomicOr(&heads[kk].bad_split, 1u);
    return;
  }
  const uint32_t hi = lo + len;  // <= n
  const unsigned long long* set = (const unsigned long long*)(sets + (size_t)kk * per_tree);
  const uint16_t* rank = (const uint16_t*)(sets + (size_t)kk * per_tree + set_bytes);
  // a bit offset of 0 masks its word away: the word's row is then never the one past the last (hi = n, n a multiple of 64)
  const unsigned long long mask_lo = (1ull << (lo & 63)) - 1, mask_hi = (1ull << (hi & 63)) - 1;
  const unsigned long long* set_lo = set + (size_t)(mask_lo ? lo >> 6 : 0) * nodes;
  const unsigned long long* set_hi = set + (size_t)(mask_hi ? hi >> 6 : 0) * nodes;
  const uint16_t* rank_lo = rank + (size_t)(lo >> 6) * nodes;
  const uint16_t* rank_hi = rank + (size_t)(hi >> 6) * nodes;  // hi >> 6 <= words: the rows of rank are words + 1
  const uint16_t* size = rank + (size_t)words * nodes;
  uint32_t best = n;
  for (uint32_t u = lane; u < nodes; u += 64) {
    const uint32_t below_hi = rank_hi[u] + (uint32_t)__popcll(set_hi[u] & mask_hi);
    const uint32_t below_lo = rank_lo[u] + (uint32_t)__popcll(set_lo[u] & mask_lo);
    const uint32_t h = len + size[u] - 2 * (below_hi - below_lo);  // |side(v) xor S(u)|, 0 .. n
    const uint32_t m = h < n - h ? h : n - h;
    best = m < best ? m : best;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)best, d, 64);
    best = o < best ? o : best;
  }
  if (lane == 0) {
    if (each) each[(size_t)kk * splits + s] = (int32_t)best;
    atomicAdd(&sum[s], (unsigned long long)best);
  }
}

}  // namespace

int transfer_launch(uint32_t n, uint32_t count, uint32_t splits, const uint32_t* pos, const transfer_split* split, const int32_t* left,
                    const int32_t* right, void* workspace, unsigned long long* sum, int32_t* each, hipStream_t st) {
  if (n < 4 || n > kNjMaxN || !count || count > 65535 || !splits || splits > 2 * n - 2) return DAFS_HIP_EINVAL;
  if (!pos || !split || !left || !right || !workspace || !sum) return DAFS_HIP_EINVAL;
  transfer_head* heads = (transfer_head*)workspace;
  uint8_t* sets = (uint8_t*)workspace + transfer_heads_bytes(count);
  const size_t per_tree = transfer_per_tree_bytes(n), set_bytes = transfer_set_bytes(n);
  if (hip_check(hipMemsetAsync(heads, 0, (size_t)count * sizeof(transfer_head), st))) return DAFS_HIP_ELAUNCH;
  STAGE_LAUNCH(ST_TRANSFER_SIDES, st)
  hipLaunchKernelGGL(k_transfer_sides, dim3(count), dim3(kTransferSidesThreads), 0, st, n, pos, left, right, heads, sets, per_tree, set_bytes);
  if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  // so many replicates per launch that it stays under 2^32 work-items
  const uint32_t blocks = (splits + kTransferThreads / 64 - 1) / (kTransferThreads / 64);
  const uint32_t per = ((1u << 24) - 1) / blocks ? ((1u << 24) - 1) / blocks : 1;
  for (uint32_t kk = 0; kk < count; kk += per) {
    const uint32_t z = count - kk < per ? count - kk : per;
    STAGE_LAUNCH(ST_TRANSFER, st)
    hipLaunchKernelGGL(k_transfer, dim3(blocks, 1, z), dim3(kTransferThreads), 0, st, n, splits, split, heads, sets, per_tree, set_bytes, sum, each, kk);
    if (hip_check(hipGetLastError())) return DAFS_HIP_ELAUNCH;
  }
  return DAFS_HIP_OK;
}

}  // namespace dafs
