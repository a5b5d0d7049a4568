// dafs_amd/csrc/tree_support.h -- how many replicate trees hold each split of a main tree, host code
// without HIP: dafs_host_tree_support (host_text.cpp) takes all replicates at once, dafs_hip_alignment_bootstrap
// (capi_nj_boot.cpp) adds them chunk by chunk.
//
// Exact and without bit sets (Day's comparison of trees).  The leaves get positions in the order a walk of the main tree
// meets them, rotated so that leaf 0 stands at position 0.  The leaves below a main node are then a circular run of
// positions, and the side of the node (the leaves below it if leaf 0 is not among them, otherwise the rest) is a plain run
// [lo, hi] with lo >= 1.  A set of leaves is that run if and only if its smallest position is lo, its largest hi and its size
// hi - lo + 1.  So a replicate node needs three numbers: an ascending pass (children precede their join) forms them for the
// leaves below every node, and one walk from the root down to leaf 0 forms them for the rest of the leaves of the nodes
// above leaf 0.  No recursion anywhere: a chain of any depth uses none of the call stack.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace dafs {

// the checks of dafs_host_cluster_cut; nullptr for a well-formed tree, otherwise what is wrong with it
inline const char* tree_malformed(uint32_t n, const int32_t* left, const int32_t* right) {
  if (!n || n > 0x7FFFFFFFu / 2) return "too many leaves";
  const uint32_t T = 2 * n - 1;
  std::vector<uint8_t> is_child(T, 0);
  for (uint32_t i = 0; i < T; ++i) {
    if (i < n) {
      if (left[i] != -1 || right[i] != -1) return "malformed tree (a leaf with a child)";
      continue;
    }
    const int64_t ch[2] = {left[i], right[i]};
    if (ch[0] == ch[1]) return "malformed tree (a join of a node with itself)";
    for (int64_t c : ch) {
      if (c < 0 || c >= (int64_t)i) return "malformed tree (a child that is not an earlier node)";
      if (is_child[c]) return "malformed tree (a node that is a child twice)";
      is_child[c] = 1;
    }
  }
  return nullptr;
}

class support_counter {
 public:
  // a well-formed main tree (tree_malformed)
  support_counter(uint32_t n, const int32_t* left, const int32_t* right) : n_(n), T_(2 * n - 1), pos_(n, 0), split_of_(2 * n - 1, -1) {
    if (n_ < 4) return;  // no split with two leaves on either side
    std::vector<uint32_t> order;  // the leaves as a walk meets them, the left child first
    order.reserve(n_);
    std::vector<uint32_t> stack(1, T_ - 1);
    while (!stack.empty()) {
      const uint32_t v = stack.back();
      stack.pop_back();
      if (v < n_) { order.push_back(v); continue; }
      stack.push_back((uint32_t)right[v]);
      stack.push_back((uint32_t)left[v]);
    }
    uint32_t at0 = 0;
    for (uint32_t p = 0; p < n_; ++p)
      if (order[p] == 0) at0 = p;
    for (uint32_t p = 0; p < n_; ++p) pos_[order[p]] = (p + n_ - at0) % n_;
    std::vector<run> side;
    sides(left, right, side);
    // one entry per different split: the two children of the root carry the same one
    std::vector<std::pair<uint64_t, uint32_t> > keyed;
    for (uint32_t v = 0; v + 1 < T_; ++v)
      if (side[v].count >= 2 && n_ - side[v].count >= 2) keyed.push_back(std::make_pair(key(side[v]), v));
    std::sort(keyed.begin(), keyed.end());
    for (size_t k = 0; k < keyed.size(); ++k) {
      if (k == 0 || keyed[k].first != keyed[k - 1].first) keys_.push_back(keyed[k].first);
      split_of_[keyed[k].second] = (int32_t)(keys_.size() - 1);
    }
    hits_.assign(keys_.size(), 0);
    seen_.assign(keys_.size(), 0);
  }

  // a well-formed replicate tree over the same leaves: every split of the main tree that it holds counts once
  void add(const int32_t* left, const int32_t* right) {
    if (keys_.empty()) return;
    ++stamp_;
    std::vector<run> side;
    sides(left, right, side);
    for (uint32_t v = 0; v + 1 < T_; ++v) {
      const run& s = side[v];
      if (s.count < 2 || n_ - s.count < 2 || s.hi - s.lo + 1 != s.count) continue;
      const std::vector<uint64_t>::const_iterator it = std::lower_bound(keys_.begin(), keys_.end(), key(s));
      if (it == keys_.end() || *it != key(s)) continue;
      const size_t id = (size_t)(it - keys_.begin());
      if (seen_[id] == stamp_) continue;
      seen_[id] = stamp_;
      ++hits_[id];
    }
  }

  // per node of the main tree the count, -1 for the root and for trivial splits
  void result(int32_t* support) const {
    for (uint32_t v = 0; v < T_; ++v) support[v] = split_of_[v] < 0 ? -1 : (int32_t)hits_[split_of_[v]];
  }

  // The transfer bootstrap compares sets of positions on the device: the position of every leaf, and
  // per node of the tree given (the main tree) the run [lo, lo + len) of its side; len = 0 for the root and trivial splits.
  const std::vector<uint32_t>& positions() const { return pos_; }
  void runs(const int32_t* left, const int32_t* right, std::vector<uint32_t>& lo, std::vector<uint32_t>& len) const {
    lo.assign(T_, 0);
    len.assign(T_, 0);
    if (n_ < 4) return;
    std::vector<run> side;
    sides(left, right, side);
    for (uint32_t v = 0; v + 1 < T_; ++v)
      if (side[v].count >= 2 && n_ - side[v].count >= 2) { lo[v] = side[v].lo; len[v] = side[v].count; }
  }

 private:
  struct run { uint32_t lo, hi, count; };
  static uint64_t key(const run& s) { return ((uint64_t)s.lo << 32) | s.hi; }
  static run merged(const run& a, const run& b) {
    if (!a.count) return b;
    if (!b.count) return a;
    return run{std::min(a.lo, b.lo), std::max(a.hi, b.hi), a.count + b.count};
  }
  // per node below the root the smallest and largest position and the size of its side
  void sides(const int32_t* left, const int32_t* right, std::vector<run>& side) const {
    side.assign(T_, run{0, 0, 0});
    std::vector<uint32_t> parent(T_, UINT32_MAX);
    for (uint32_t v = 0; v < n_; ++v) side[v] = run{pos_[v], pos_[v], 1};
    for (uint32_t v = n_; v < T_; ++v) {
      side[v] = merged(side[(uint32_t)left[v]], side[(uint32_t)right[v]]);
      parent[(uint32_t)left[v]] = parent[(uint32_t)right[v]] = v;
    }
    // the nodes above leaf 0 hold it: their side is the rest of the leaves, gathered from the root down
    std::vector<uint32_t> path;
    for (uint32_t v = 0; v != UINT32_MAX; v = parent[v]) path.push_back(v);
    run rest{0, 0, 0};  // the leaves that are not below path[k]
    for (size_t k = path.size() - 1; k-- > 0;) {
      const uint32_t up = path[k + 1], v = path[k];
      const uint32_t sibling = (uint32_t)left[up] == v ? (uint32_t)right[up] : (uint32_t)left[up];
      rest = merged(rest, side[sibling]);  // side[sibling] is still the sibling's own leaves: it is not on the path
      side[v] = rest;
    }
  }

  uint32_t n_, T_;
  std::vector<uint32_t> pos_;
  std::vector<int32_t> split_of_;
  std::vector<uint64_t> keys_;
  std::vector<uint32_t> hits_, seen_;
  uint32_t stamp_ = 0;
};

}  // namespace dafs
