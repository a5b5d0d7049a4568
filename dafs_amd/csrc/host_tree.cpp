// dafs_amd/csrc/host_tree.cpp -- DAFS::build_tree (reference src/dafs.cpp:446-492) as a C entry point, so that
// every host (the C++ command line, the Python driver of tests and bench.py) builds the guide tree with the same
// code: greedy joins taken from a max-heap of (similarity, (i, j)), merged distance (d[ii][l] + d[ii][r]) * s / 2.
// Also the merge of new sequences into a fixed seed alignment (dafs_host_merge_added) and the cut of a guide tree into
// clusters (dafs_host_cluster_cut), shared the same way, and the distances of an alignment's rows from the integer matrices of
// dafs_hip_alignment_identity (dafs_host_nj_distances).
// Host logic only; nothing here touches the device.
#include <cmath>
#include <cstdint>
#include <queue>
#include <utility>
#include <vector>

#include "../../include/dafs_hip.h"
#include "call_host.h"

using dafs::refuse;

extern "C" int dafs_host_build_tree(uint32_t n0, const float* sim, float* score, int32_t* left, int32_t* right) {
  if (!n0 || !sim || !score || !left || !right) return DAFS_HIP_EINVAL;
  typedef std::pair<float, std::pair<uint32_t, uint32_t> > node_t;
  uint32_t n = n0;
  const uint32_t T = 2 * n0 - 1;
  for (uint32_t i = 0; i < T; ++i) { score[i] = 0.0f; left[i] = -1; right[i] = -1; }
  std::vector<std::vector<float> > d(n, std::vector<float>(n, 0.0f));
  std::vector<uint32_t> idx(T, UINT32_MAX);
  for (uint32_t i = 0; i != n; ++i) idx[i] = i;
  std::priority_queue<node_t> pq;
  for (uint32_t i = 0; i + 1 < n; ++i)
    for (uint32_t j = i + 1; j != n; ++j) {
      d[i][j] = d[j][i] = sim[(size_t)i * n0 + j];
      pq.push(std::make_pair(sim[(size_t)i * n0 + j], std::make_pair(i, j)));
    }
  while (!pq.empty()) {
    const node_t t = pq.top();
    pq.pop();
    const uint32_t a = t.second.first, b = t.second.second;
    if (idx[a] == UINT32_MAX || idx[b] == UINT32_MAX) continue;
    const uint32_t l = idx[a], r = idx[b];
    idx[a] = idx[b] = UINT32_MAX;
    for (uint32_t i = 0; i != n; ++i)
      if (idx[i] != UINT32_MAX) {
        const uint32_t ii = idx[i];
        d[ii][l] = d[l][ii] = (d[ii][l] + d[ii][r]) * t.first / 2;
        pq.push(std::make_pair(d[ii][l], std::make_pair(i, n)));
      }
    score[n] = t.first;
    left[n] = (int32_t)a;
    right[n] = (int32_t)b;
    idx[n++] = l;
  }
  return DAFS_HIP_OK;
}

// The cut of `dafs --cluster`.  A join's children always have lower node indices than the join, so one
// ascending pass decides every join after the joins below it.
extern "C" int dafs_host_cluster_cut(uint32_t n, const float* score, const int32_t* left, const int32_t* right, int mode, float threshold,
                                     uint32_t count, uint32_t* labels, uint32_t* n_clusters) {
  if (!n || !score || !left || !right || !labels || !n_clusters) return refuse("cluster cut: invalid argument");
  if (mode != DAFS_CLUSTER_THRESHOLD && mode != DAFS_CLUSTER_COUNT) return refuse("cluster cut: unknown mode");
  if (mode == DAFS_CLUSTER_THRESHOLD && std::isnan(threshold)) return refuse("cluster cut: the threshold is not a number");
  if (mode == DAFS_CLUSTER_COUNT && (count < 1 || count > n)) return refuse("cluster cut: the number of clusters must be 1 .. the number of sequences");
  if (n > 0x7FFFFFFFu / 2) return refuse("cluster cut: too many sequences");
  const uint32_t T = 2 * n - 1;
  std::vector<uint32_t> parent(T, UINT32_MAX);
  for (uint32_t i = 0; i < T; ++i) {
    if (i < n) {
      if (left[i] != -1 || right[i] != -1) return refuse("cluster cut: malformed tree (a leaf with a child)");
      continue;
    }
    const int64_t ch[2] = {left[i], right[i]};
    if (ch[0] == ch[1]) return refuse("cluster cut: malformed tree (a join of a node with itself)");
    for (int64_t c : ch) {
      if (c < 0 || c >= (int64_t)i) return refuse("cluster cut: malformed tree (a child that is not an earlier node)");
      if (parent[c] != UINT32_MAX) return refuse("cluster cut: malformed tree (a node that is a child twice)");
      parent[c] = i;
    }
  }
  // 2n - 2 child slots were filled with distinct nodes below the root: every node but the root has its parent
  std::vector<uint8_t> kept(T, 1);  // leaves count as kept
  const uint32_t undone_from = mode == DAFS_CLUSTER_COUNT ? T - (count - 1) : T;
  for (uint32_t i = n; i < T; ++i) {
    const bool own = mode == DAFS_CLUSTER_COUNT ? i < undone_from : score[i] >= threshold;
    kept[i] = own && kept[left[i]] && kept[right[i]];
  }
  std::vector<uint32_t> label_of(T, UINT32_MAX);
  uint32_t next = 0;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t top = i;
    while (parent[top] != UINT32_MAX && kept[parent[top]]) top = parent[top];
    if (label_of[top] == UINT32_MAX) label_of[top] = next++;
    labels[i] = label_of[top];
  }
  *n_clusters = next;
  return DAFS_HIP_OK;
}

// DESIGN.md section 22, "Distances from an alignment": nj_pair_distance of every pair of rows, 0 on the diagonal.
extern "C" int dafs_host_nj_distances(uint32_t n, const uint32_t* ident, const uint32_t* aligned, int model, double* dist) {
  if (!n || !ident || !aligned || !dist) return refuse("nj_distances: a missing argument");
  if (model != DAFS_NJ_P && model != DAFS_NJ_JC) return refuse("nj_distances: unknown model");
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t s = 0; s < n; ++s) {
      const size_t at = (size_t)r * n + s;
      if (r == s) { dist[at] = 0.0; continue; }
      if (ident[at] > aligned[at]) return refuse("nj_distances: more identical columns than aligned ones");
      dist[at] = dafs::nj_pair_distance(model, aligned[at] - ident[at], aligned[at]);
    }
  return DAFS_HIP_OK;
}

// The merge of `dafs --seed`: k new sequences placed into a fixed seed of C columns from their
// column maps z.  Anchors are shifted by one below (slot 0 is anchor -1, slot c + 1 is seed column c).
extern "C" int dafs_host_merge_added(uint32_t C, uint32_t k, const uint32_t* lens, const uint32_t* z, uint32_t* seed_col,
                                     uint32_t* res_col, uint32_t* width) {
  if (!width || (C && !seed_col) || (k && !lens)) return DAFS_HIP_EINVAL;
  uint64_t total = 0;
  for (uint32_t j = 0; j != k; ++j) total += lens[j];
  if (total && (!z || !res_col)) return DAFS_HIP_EINVAL;
  // per anchor slot the widest insert block any sequence needs; matched columns must rise strictly within a sequence
  std::vector<uint32_t> W((size_t)C + 1, 0);
  const uint32_t* zj = z;
  for (uint32_t j = 0; j != k; zj += lens[j], ++j) {
    uint32_t a = 0, cnt = 0;
    for (uint32_t i = 0; i != lens[j]; ++i) {
      if (zj[i] == DAFS_HIP_NONE) { ++cnt; continue; }
      if (zj[i] >= C || zj[i] + 1 <= a) return DAFS_HIP_EINVAL;
      if (cnt > W[a]) W[a] = cnt;
      a = zj[i] + 1;
      cnt = 0;
    }
    if (cnt > W[a]) W[a] = cnt;
  }
  // layout: the anchor -1 block, then per seed column the column and its block
  std::vector<uint32_t> start((size_t)C + 1);
  uint64_t pos = W[0];
  start[0] = 0;
  for (uint32_t c = 0; c != C; ++c) {
    seed_col[c] = (uint32_t)pos;
    start[c + 1] = (uint32_t)++pos;
    pos += W[c + 1];
    if (pos >= DAFS_HIP_NONE) return DAFS_HIP_EINVAL;
  }
  // every residue: its seed column, or the next free place of its block (left-justified)
  zj = z;
  uint32_t* rj = res_col;
  for (uint32_t j = 0; j != k; zj += lens[j], rj += lens[j], ++j) {
    uint32_t a = 0, t = 0;
    for (uint32_t i = 0; i != lens[j]; ++i) {
      if (zj[i] == DAFS_HIP_NONE) {
        rj[i] = start[a] + t++;
      } else {
        rj[i] = seed_col[zj[i]];
        a = zj[i] + 1;
        t = 0;
      }
    }
  }
  *width = (uint32_t)pos;
  return DAFS_HIP_OK;
}
