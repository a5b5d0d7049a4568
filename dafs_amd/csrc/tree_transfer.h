// dafs_amd/csrc/tree_transfer.h -- launch interface of the transfer-bootstrap kernels (tree_transfer.hip; dafs_hip_tree_transfer,
// dafs_hipk_tree_transfer and dafs_hip_alignment_bootstrap_transfer in capi_nj_boot.cpp; the contract, to the bit, in DESIGN.md
// section 28).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nj.h"

namespace dafs {

// A non-trivial side of the main tree as a run of positions [lo, lo + len): lo >= 1, len >= 2, lo + len <= n (tree_support.h).
// The depth of the split, min(len, n - len), stays on the host: the kernels do not need it.
struct transfer_split { uint32_t lo, len; };

// What the kernels refuse, per replicate tree.  Non-zero: nothing of that replicate is added to the sums.
struct transfer_head {
  uint32_t bad_tree;   // a leaf with a child, a child that is not an earlier node, or a position that is not below n
  uint32_t bad_split;  // a run that does not lie in 1 .. n
};

constexpr uint32_t kTransferSidesThreads = 256;
constexpr uint32_t kTransferThreads = 256;  // four wavefronts, a split each

// Per replicate: the sets of the 2n - 2 nodes below the root, word-major (set[word][node], ceil(n / 64) words of 64
// positions), and per word the count of set positions in the words before it (rank[word][node], 16 bits; one row more than
// the sets: rank[words][node] is the size of the set).
inline uint32_t transfer_words(uint32_t n) { return (n + 63) / 64; }
inline size_t transfer_set_bytes(uint32_t n) { return nj_round((size_t)transfer_words(n) * (2 * (size_t)n - 2) * 8); }
inline size_t transfer_rank_bytes(uint32_t n) { return nj_round(((size_t)transfer_words(n) + 1) * (2 * (size_t)n - 2) * 2); }
inline size_t transfer_heads_bytes(uint32_t count) { return nj_round((size_t)count * sizeof(transfer_head)); }
inline size_t transfer_per_tree_bytes(uint32_t n) { return transfer_set_bytes(n) + transfer_rank_bytes(n); }
// the workspace of `count` replicate trees: the heads, then sets and ranks of each
inline size_t transfer_workspace_bytes(uint32_t n, uint32_t count) {
  return transfer_heads_bytes(count) + (size_t)count * transfer_per_tree_bytes(n);
}

// `count` replicate trees of n >= 4 leaves on st: left / right [count][2n-1] device arrays, pos[n] the leaves' positions,
// split[splits] the runs of the main tree.  sum[splits] (64-bit, zeroed by the caller before the first chunk) gains the
// transfer index of every replicate; each (or null) [count][splits] receives them one by one.  The heads are zeroed here.
int transfer_launch(uint32_t n, uint32_t count, uint32_t splits, const uint32_t* pos, const transfer_split* split, const int32_t* left,
                    const int32_t* right, void* workspace, unsigned long long* sum, int32_t* each, hipStream_t st);

}  // namespace dafs
