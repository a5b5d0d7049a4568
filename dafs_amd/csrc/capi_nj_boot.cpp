// dafs_amd/csrc/capi_nj_boot.cpp -- dafs_hip_nj_trees (L1), dafs_hipk_nj_batch (L0), dafs_hip_alignment_bootstrap and
// dafs_hip_bootstrap_alignment: many neighbour-joining trees in one call, and the bootstrap support of a tree from replicate
// alignments drawn, measured and joined on the device (nj_boot.hip; the contract in DESIGN.md section 23); dafs_hip_tree_transfer
// (L1), dafs_hipk_tree_transfer (L0) and dafs_hip_alignment_bootstrap_transfer: the transfer index of every split of the main
// tree against the replicate trees (tree_transfer.hip; section 28).  The reference has no counterpart.
//
// Host work: the checks (everything is refused before the first launch), the used columns transposed for the device, the
// chunks of replicates under a byte budget, the entries of the fix-up list recomputed with the host's log(), the refusals a
// launch reports in its heads, and the count of the splits (tree_support.h).  Device memory belongs to one call.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <new>
#include <vector>

#include "../../include/dafs_hip.h"
#include "alistat.h"
#include "call_frame.h"
#include "call_host.h"
#include "nj_boot.h"
#include "tree_support.h"
#include "tree_transfer.h"

using namespace dafs;

namespace {

thread_local uint64_t g_fixups = 0;

// what the heads of the joined matrices k0, k0 + 1, ... say: the first one that has something to say
int heads_verdict(const char* who, const char* what, uint32_t n, uint32_t k0, const std::vector<nj_head>& heads) {
  for (size_t k = 0; k < heads.size(); ++k)
    if (int rc = nj_head_verdict(who, what, k0 + (uint32_t)k, n, heads[k])) return rc;
  return DAFS_HIP_OK;
}

// The matrix of replicate k on the host, from the transposed used columns: the overflow path of the fix-up list.
void host_replicate_distances(uint32_t n, uint32_t U, const uint8_t* cells, uint64_t seed, uint32_t k, int model, double* dist) {
  const uint64_t base = mix64(seed + kMixGolden * (uint64_t)(k + 1));
  std::vector<uint32_t> draw(U);
  for (uint32_t i = 0; i < U; ++i) draw[i] = (uint32_t)(((mix64(base + i) >> 32) * (uint64_t)U) >> 32);
  std::vector<uint8_t> rep((size_t)n * U);  // row-major
  for (uint32_t i = 0; i < U; ++i)
    for (uint32_t r = 0; r < n; ++r) rep[(size_t)r * U + i] = cells[(size_t)draw[i] * n + r];
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t s = r + 1; s < n; ++s) {
      const uint8_t* x = &rep[(size_t)r * U];
      const uint8_t* y = &rep[(size_t)s * U];
      uint32_t comp = 0, ident = 0;
      for (uint32_t i = 0; i < U; ++i) {
        comp += x[i] <= 4 && y[i] <= 4 ? 1u : 0u;
        ident += x[i] <= 3 && x[i] == y[i] ? 1u : 0u;
      }
      dist[(size_t)r * n + s] = nj_pair_distance(model, comp - ident, comp);
    }
}

// the checks the two alignment calls share; the used columns in ascending order into cols
int columns_of(const char* who, uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use, std::vector<uint32_t>& cols) {
  char msg[160];
  if (n == 0 || n > kNjMaxN) { snprintf(msg, sizeof msg, "%s: it takes 1 to 16384 rows", who); return refuse(msg); }
  if (len == 0 || len > kAliMaxLen) { snprintf(msg, sizeof msg, "%s: it takes 1 to 1048576 columns", who); return refuse(msg); }
  for (size_t at = 0; at < (size_t)n * len; ++at)
    if (cell[at] > 5) { snprintf(msg, sizeof msg, "%s: a cell code above 5", who); return refuse(msg); }
  for (uint32_t c = 0; c < len; ++c)
    if (!use || use[c]) cols.push_back(c);
  if (cols.empty()) return refuse(dafs_host_bootstrap_refusal(DAFS_BOOTSTRAP_NO_COLUMN));
  return DAFS_HIP_OK;
}

// cells[u * n + r] = cell[r][cols[u]]
std::vector<uint8_t> transposed(uint32_t n, uint32_t len, const uint8_t* cell, const std::vector<uint32_t>& cols) {
  std::vector<uint8_t> out(cols.size() * (size_t)n);
  for (size_t u = 0; u < cols.size(); ++u)
    for (uint32_t r = 0; r < n; ++r) out[u * n + r] = cell[(size_t)r * len + cols[u]];
  return out;
}

// What the transfer kernels take from the main tree: the leaves' positions and, per node with a
// non-trivial split, the run of its side.  Both children of the root are listed: they carry the same run and get the same sum.
struct transfer_plan {
  std::vector<uint32_t> pos, node;  // node[s]: the main node of run s
  std::vector<transfer_split> split;
  transfer_plan(uint32_t n, const support_counter& counter, const int32_t* left, const int32_t* right) : pos(counter.positions()) {
    std::vector<uint32_t> lo, len;
    counter.runs(left, right, lo, len);
    for (uint32_t v = 0; v + 1 < 2 * n - 1; ++v)
      if (len[v]) { node.push_back(v); split.push_back(transfer_split{lo[v], len[v]}); }
  }
  uint32_t splits() const { return (uint32_t)split.size(); }
  // transfer[2n-1] from the sums of the runs; -1 for the root and trivial splits
  void result(uint32_t n, const std::vector<unsigned long long>& sum, int64_t* transfer) const {
    for (size_t v = 0; v < 2 * (size_t)n - 1; ++v) transfer[v] = -1;
    for (size_t s = 0; s < node.size(); ++s) transfer[node[s]] = (int64_t)sum[s];
  }
};

// the first replicate of the chunk that the transfer kernels refused
int transfer_verdict(const char* who, uint32_t k0, const std::vector<transfer_head>& heads) {
  for (size_t k = 0; k < heads.size(); ++k)
    if (heads[k].bad_tree || heads[k].bad_split) {
      char msg[160];
      snprintf(msg, sizeof msg, "%s: replicate %u: %s", who, k0 + (uint32_t)k,
               heads[k].bad_tree ? "malformed tree (the transfer kernels refused it)" : "a run of the main tree outside the positions");
      return refuse(msg);
    }
  return DAFS_HIP_OK;
}

size_t boot_byte_budget() {
  // 8 GiB, or half of what the device has free: at 2 048 rows a replicate takes 67 MB, and a chunk should hold a workgroup
  // for every compute unit where the replicates allow it
  size_t budget = (size_t)8 << 30, free_bytes = 0, total_bytes = 0;
  if (!hip_check(hipMemGetInfo(&free_bytes, &total_bytes)) && free_bytes / 2 < budget) budget = free_bytes / 2;
  return (size_t)env_uint("DAFS_NJ_BOOT_BYTES", 1, SIZE_MAX, budget);  // tests: small chunks (the results do not depend on them)
}

}  // namespace

extern "C" uint64_t dafs_hip_bootstrap_fixups(void) { return g_fixups; }

extern "C" size_t dafs_hipk_nj_batch_workspace(uint32_t n, uint32_t count) {
  return n >= 2 && n <= kNjMaxN && count ? nj_batch_workspace_bytes(n, count) : 0;
}

extern "C" int dafs_hipk_nj_batch(uint32_t n, uint32_t count, const double* d_dist, void* d_workspace, int32_t* d_left, int32_t* d_right,
                                  double* d_length, void* hip_stream) {
  if (n < 2 || n > kNjMaxN) return refuse("nj_batch: the launch takes 2 to 16384 rows");
  if (!count) return refuse("nj_batch: no matrix");
  if (!d_dist || !d_workspace || !d_left || !d_right || !d_length) return refuse("nj_batch: a missing argument");
  if ((uintptr_t)d_workspace & 255) return refuse("nj_batch: the workspace must be 256-byte aligned");
  return nj_batch_launch(n, count, d_dist, d_workspace, d_left, d_right, d_length, n <= nj_batch_max_n(), (hipStream_t)hip_stream);
}

extern "C" int dafs_hip_nj_trees(dafs_hip_ctx* c, uint32_t n, uint32_t count, const double* dist, int32_t* left, int32_t* right,
                                 double* length) {
  if (!c || !dist || !left || !right || !length) return refuse("nj_trees: a missing argument");
  if (n == 0 || n > kNjMaxN) return refuse("nj_trees: it takes 1 to 16384 rows");
  if (!count) return refuse("nj_trees: no matrix");
  for (uint32_t k = 0; k < count; ++k) {
    const double* d = dist + (size_t)k * n * n;
    for (uint32_t x = 0; x + 1 < n; ++x)
      for (uint32_t y = x + 1; y < n; ++y)
        if (!isfinite(d[(size_t)x * n + y])) {
          char msg[160];
          snprintf(msg, sizeof msg, "nj_trees: matrix %u: the entry (%u, %u) above the diagonal is not finite", k, x, y);
          return refuse(msg);
        }
  }
  if (n == 1) {  // one-leaf trees: no launch
    for (uint32_t k = 0; k < count; ++k) {
      left[k] = right[k] = -1;
      length[k] = 0.0;
    }
    return DAFS_HIP_OK;
  }
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const size_t T = 2 * (size_t)n - 1, all = (size_t)count * T;
  carve cv;  // the three output arrays of one allocation
  const size_t o_length = cv.take(all * 8), o_left = cv.take(all * 4), o_right = cv.take(all * 4);
  std::vector<nj_head> heads(count);
  call_frame f(c);
  void *in, *ws, *out;
  if (!(in = f.alloc((size_t)count * n * n * 8)) || !(ws = f.alloc(nj_batch_workspace_bytes(n, count))) || !(out = f.alloc(cv.bytes())))
    return DAFS_HIP_ENOMEM;
  double* d_length = (double*)((uint8_t*)out + o_length);
  int32_t* d_left = (int32_t*)((uint8_t*)out + o_left);
  int32_t* d_right = (int32_t*)((uint8_t*)out + o_right);
  int rc;
  if (f.up(in, dist, (size_t)count * n * n * 8)) return DAFS_HIP_ELAUNCH;
  if ((rc = nj_batch_launch(n, count, (const double*)in, ws, d_left, d_right, d_length, n <= nj_batch_max_n(), f.st))) return rc;
  if (f.down(heads.data(), ws, (size_t)count * sizeof(nj_head))) return DAFS_HIP_ELAUNCH;
  if ((rc = f.finish())) return rc;
  if ((rc = heads_verdict("nj_trees", "matrix", n, 0, heads))) return rc;
  if (hip_check(hipMemcpy(length, d_length, all * 8, hipMemcpyDeviceToHost)) || hip_check(hipMemcpy(left, d_left, all * 4, hipMemcpyDeviceToHost)) ||
      hip_check(hipMemcpy(right, d_right, all * 4, hipMemcpyDeviceToHost)))
    return DAFS_HIP_ELAUNCH;
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_bootstrap_alignment(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use, uint64_t seed,
                                            uint32_t k, uint8_t* out_cell) {
  if (!c || !cell || !out_cell) return refuse("bootstrap_alignment: a missing argument");
  if (k >= kBootMaxReplicates) return refuse("bootstrap_alignment: the replicates are numbered 0 to 65535");
  std::vector<uint32_t> cols;
  if (int rc = columns_of("bootstrap_alignment", n, len, cell, use, cols)) return rc;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const uint32_t U = (uint32_t)cols.size(), words = (U + 63) / 64;
  const std::vector<uint8_t> cells = transposed(n, len, cell, cols);
  std::vector<uint64_t> planes((size_t)words * 4 * n);
  call_frame f(c);
  void *d_cells, *d_planes;
  if (!(d_cells = f.alloc(cells.size())) || !(d_planes = f.alloc(planes.size() * 8))) return DAFS_HIP_ENOMEM;
  boot_args a;
  memset(&a, 0, sizeof a);
  a.cells = (const uint8_t*)d_cells;
  a.planes = (uint64_t*)d_planes;
  a.seed = seed;
  a.n = n; a.U = U; a.words = words; a.k0 = k; a.count = 1;
  int rc;
  if (f.up(d_cells, cells.data(), cells.size())) return DAFS_HIP_ELAUNCH;
  if ((rc = boot_pack(a, f.st))) return rc;
  if (f.down(planes.data(), d_planes, planes.size() * 8)) return DAFS_HIP_ELAUNCH;
  if ((rc = f.finish())) return rc;
  for (uint32_t r = 0; r < n; ++r)
    for (uint32_t i = 0; i < U; ++i) {
      const uint64_t* w = &planes[(size_t)(i / 64) * 4 * n];
      const uint32_t b = i % 64;
      const uint32_t lo = (uint32_t)(w[(size_t)ALI_LO * n + r] >> b) & 1, hi = (uint32_t)(w[(size_t)ALI_HI * n + r] >> b) & 1;
      const bool base = (w[(size_t)ALI_BASE * n + r] >> b) & 1, res = (w[(size_t)ALI_RES * n + r] >> b) & 1;
      out_cell[(size_t)r * U + i] = (uint8_t)(base ? (lo | (hi << 1)) : res ? 4 : 5);
    }
  return DAFS_HIP_OK;
}

// the body of dafs_hip_alignment_bootstrap and dafs_hip_alignment_bootstrap_transfer; transfer: null for the first
static int alignment_bootstrap(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use, int model, uint32_t B, uint64_t seed,
                               const int32_t* main_left, const int32_t* main_right, int32_t* support, int32_t* rep_left, int32_t* rep_right,
                               int64_t* transfer) {
  if (model != DAFS_NJ_P && model != DAFS_NJ_JC) return refuse(dafs_host_phylogeny_refusal(DAFS_PHYLOGENY_UNKNOWN_MODEL));
  if (B == 0 || B > kBootMaxReplicates) return refuse(dafs_host_bootstrap_refusal(DAFS_BOOTSTRAP_COUNT));
  std::vector<uint32_t> cols;
  if (int rc = columns_of("alignment_bootstrap", n, len, cell, use, cols)) return rc;
  if (const char* bad = tree_malformed(n, main_left, main_right)) {
    char msg[160];
    snprintf(msg, sizeof msg, "alignment_bootstrap: the main tree: %s", bad);
    return refuse(msg);
  }
  const size_t T = 2 * (size_t)n - 1;
  if (n <= 3) {  // no split with two leaves on either side: nothing is drawn or launched
    for (size_t v = 0; v < T; ++v) support[v] = -1;
    if (transfer)
      for (size_t v = 0; v < T; ++v) transfer[v] = -1;
    if (rep_left)
      for (size_t v = 0; v < (size_t)B * T; ++v) rep_left[v] = rep_right[v] = -1;
    return DAFS_HIP_OK;
  }
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const uint32_t U = (uint32_t)cols.size(), words = (U + 63) / 64;
  const bool batched = n <= nj_batch_max_n();
  const double guard = env_double("DAFS_NJ_BOOT_GUARD", 1.0 / 1048576.0);
  const uint32_t fix_cap = (uint32_t)env_uint("DAFS_NJ_BOOT_FIXUPS", 1, 65536, 65536);  // tests: a list that overflows
  // replicates per chunk under the byte budget: the planes, the matrix, the working copy and the outputs of each
  const size_t plane_bytes = (size_t)words * 4 * n * 8, dist_bytes = (size_t)n * n * 8;
  const size_t per = plane_bytes + dist_bytes + (batched ? nj_batch_copy_bytes(n) : 0) + T * 16 + sizeof(nj_head) +
                     (transfer ? transfer_per_tree_bytes(n) + sizeof(transfer_head) : 0);  // the sets and ranks of the transfer kernels
  const size_t budget = boot_byte_budget();
  const uint32_t chunk_reps = (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(B, kBootChunkReplicates), budget / per));
  const size_t all = (size_t)chunk_reps * T;
  carve cv;  // the three output arrays of one allocation
  const size_t o_length = cv.take(all * 8), o_left = cv.take(all * 4), o_right = cv.take(all * 4);

  std::vector<uint8_t> cells;
  std::vector<int32_t> h_left, h_right, all_left, all_right;
  std::vector<nj_head> heads;
  std::vector<transfer_head> t_heads;
  std::vector<unsigned long long> t_sum;
  std::vector<uint32_t> t_pos;
  std::vector<transfer_split> t_split;
  std::vector<boot_fix> fix;
  std::vector<double> patch, whole;
  try {
    cells = transposed(n, len, cell, cols);
    h_left.resize(all);
    h_right.resize(all);
    if (rep_left) { all_left.resize((size_t)B * T); all_right.resize((size_t)B * T); }  // the caller's stay untouched by a refusal
  } catch (const std::bad_alloc&) {
    return DAFS_HIP_ENOMEM;
  }
  call_frame f(c);  // queued copies use this call's vectors
  hipStream_t st = f.st;
  void *d_cells, *d_planes, *d_dist, *d_ws, *d_out, *d_fix;
  if (!(d_cells = f.alloc(cells.size())) || !(d_planes = f.alloc(chunk_reps * plane_bytes)) || !(d_dist = f.alloc(chunk_reps * dist_bytes)) ||
      !(d_ws = f.alloc(batched ? nj_batch_workspace_bytes(n, chunk_reps) : nj_batch_heads_bytes(chunk_reps) + nj_workspace_bytes(n))) ||
      !(d_out = f.alloc(cv.bytes())) || !(d_fix = f.alloc(256 + (size_t)fix_cap * sizeof(boot_fix))))
    return DAFS_HIP_ENOMEM;
  double* d_length = (double*)((uint8_t*)d_out + o_length);
  int32_t* d_left = (int32_t*)((uint8_t*)d_out + o_left);
  int32_t* d_right = (int32_t*)((uint8_t*)d_out + o_right);
  if (f.up(d_cells, cells.data(), cells.size())) return DAFS_HIP_ELAUNCH;

  try {
  support_counter counter(n, main_left, main_right);
  const transfer_plan plan(n, counter, main_left, main_right);
  const uint32_t S = plan.splits();  // n >= 4: at least one
  void *d_pos = nullptr, *d_split = nullptr, *d_sum = nullptr, *d_tws = nullptr;
  if (transfer) {
    t_sum.resize(S);
    t_pos = plan.pos;  // queued copies read them: they outlive the frame
    t_split = plan.split;
    if (!(d_pos = f.alloc((size_t)n * 4)) || !(d_split = f.alloc((size_t)S * sizeof(transfer_split))) || !(d_sum = f.alloc((size_t)S * 8)) ||
        !(d_tws = f.alloc(transfer_workspace_bytes(n, chunk_reps))))
      return DAFS_HIP_ENOMEM;
    if (f.up(d_pos, t_pos.data(), (size_t)n * 4) || f.up(d_split, t_split.data(), (size_t)S * sizeof(transfer_split)) ||
        f.fill(d_sum, 0, (size_t)S * 8))
      return DAFS_HIP_ELAUNCH;
  }
  boot_args a;
  memset(&a, 0, sizeof a);
  a.cells = (const uint8_t*)d_cells;
  a.planes = (uint64_t*)d_planes;
  a.dist = (double*)d_dist;
  a.fix_count = (uint32_t*)d_fix;
  a.fix = (boot_fix*)((uint8_t*)d_fix + 256);
  a.seed = seed;
  a.guard = guard;
  a.n = n; a.U = U; a.words = words; a.chunk = std::min(words, kAliMaxChunk);
  a.fix_cap = fix_cap;
  a.model = model;
  int rc;
  for (uint32_t k0 = 0; k0 < B; k0 += chunk_reps) {
    const uint32_t count = std::min(chunk_reps, B - k0);
    a.k0 = k0;
    a.count = count;
    if (f.fill(a.fix_count, 0, 4)) return DAFS_HIP_ELAUNCH;
    if ((rc = boot_pack(a, st)) || (rc = boot_dist(a, st))) return rc;
    // the one wait of a chunk: the length of the fix-up list
    uint32_t fixes = 0;
    if (f.down(&fixes, a.fix_count, 4) || f.finish()) return DAFS_HIP_ELAUNCH;
    g_fixups += fixes;
    if (fixes > fix_cap) {  // the list overflowed: this chunk's matrices whole, on the host
      whole.assign((size_t)count * n * n, 0.0);
      for (uint32_t kk = 0; kk < count; ++kk) host_replicate_distances(n, U, cells.data(), seed, k0 + kk, model, &whole[(size_t)kk * n * n]);
      if (f.up(d_dist, whole.data(), whole.size() * 8)) return DAFS_HIP_ELAUNCH;
    } else if (fixes) {
      fix.resize(fixes);
      if (hip_check(hipMemcpy(fix.data(), a.fix, (size_t)fixes * sizeof(boot_fix), hipMemcpyDeviceToHost))) return DAFS_HIP_ELAUNCH;
      if (fixes <= 64) {  // the usual few: one word each
        patch.resize(fixes);
        for (uint32_t i = 0; i < fixes; ++i) {
          patch[i] = nj_pair_distance(model, fix[i].mism, fix[i].comp);
          if (f.up(a.dist + ((size_t)fix[i].k * n + fix[i].r) * n + fix[i].s, &patch[i], 8)) return DAFS_HIP_ELAUNCH;
        }
      } else {  // many: the matrices make the round trip once
        whole.resize((size_t)count * n * n);
        if (hip_check(hipMemcpy(whole.data(), d_dist, whole.size() * 8, hipMemcpyDeviceToHost))) return DAFS_HIP_ELAUNCH;
        for (const boot_fix& x : fix) whole[((size_t)x.k * n + x.r) * n + x.s] = nj_pair_distance(model, x.mism, x.comp);
        if (f.up(d_dist, whole.data(), whole.size() * 8)) return DAFS_HIP_ELAUNCH;
      }
    }
    if ((rc = nj_batch_launch(n, count, a.dist, d_ws, d_left, d_right, d_length, batched, st))) return rc;
    // the transfer kernels read the trees where the joins left them; a tree that a refused replicate left unfinished is
    // refused by them too, and the verdict on the joins comes first
    if (transfer && (rc = transfer_launch(n, count, S, (const uint32_t*)d_pos, (const transfer_split*)d_split, d_left, d_right, d_tws,
                                          (unsigned long long*)d_sum, nullptr, st)))
      return rc;
    heads.resize(count);
    t_heads.resize(transfer ? count : 0);
    if (f.down(heads.data(), d_ws, (size_t)count * sizeof(nj_head)) || f.down(h_left.data(), d_left, (size_t)count * T * 4) ||
        f.down(h_right.data(), d_right, (size_t)count * T * 4) ||
        (transfer && f.down(t_heads.data(), d_tws, (size_t)count * sizeof(transfer_head))) || f.finish())
      return DAFS_HIP_ELAUNCH;
    if ((rc = heads_verdict("alignment_bootstrap", "replicate", n, k0, heads))) return rc;
    if ((rc = transfer_verdict("alignment_bootstrap", k0, t_heads))) return rc;
    for (uint32_t kk = 0; kk < count; ++kk) counter.add(&h_left[kk * T], &h_right[kk * T]);
    if (rep_left) {
      memcpy(&all_left[(size_t)k0 * T], h_left.data(), (size_t)count * T * 4);
      memcpy(&all_right[(size_t)k0 * T], h_right.data(), (size_t)count * T * 4);
    }
  }
  if (transfer) {  // only the sums come back, at the end
    if (f.down(t_sum.data(), d_sum, (size_t)S * 8) || f.finish()) return DAFS_HIP_ELAUNCH;
    plan.result(n, t_sum, transfer);
  }
  counter.result(support);
  if (rep_left) {
    memcpy(rep_left, all_left.data(), all_left.size() * 4);
    memcpy(rep_right, all_right.data(), all_right.size() * 4);
  }
  } catch (const std::bad_alloc&) {
    return DAFS_HIP_ENOMEM;
  }
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_alignment_bootstrap(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use, int model, uint32_t B,
                                            uint64_t seed, const int32_t* main_left, const int32_t* main_right, int32_t* support, int32_t* rep_left,
                                            int32_t* rep_right) {
  g_fixups = 0;
  if (!c || !cell || !main_left || !main_right || !support || (rep_left == nullptr) != (rep_right == nullptr))
    return refuse("alignment_bootstrap: a missing argument");
  return alignment_bootstrap(c, n, len, cell, use, model, B, seed, main_left, main_right, support, rep_left, rep_right, nullptr);
}

extern "C" int dafs_hip_alignment_bootstrap_transfer(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use, int model,
                                                     uint32_t B, uint64_t seed, const int32_t* main_left, const int32_t* main_right, int32_t* support,
                                                     int32_t* rep_left, int32_t* rep_right, int64_t* transfer) {
  g_fixups = 0;
  if (!c || !cell || !main_left || !main_right || !support || !transfer || (rep_left == nullptr) != (rep_right == nullptr))
    return refuse("alignment_bootstrap_transfer: a missing argument");
  return alignment_bootstrap(c, n, len, cell, use, model, B, seed, main_left, main_right, support, rep_left, rep_right, transfer);
}

extern "C" size_t dafs_hipk_tree_transfer_workspace(uint32_t n, uint32_t count) {
  return n >= 4 && n <= kNjMaxN && count && count <= kBootChunkReplicates ? transfer_workspace_bytes(n, count) : 0;
}

extern "C" int dafs_hipk_tree_transfer(uint32_t n, uint32_t count, uint32_t splits, const uint32_t* d_pos, const uint32_t* d_split,
                                       const int32_t* d_left, const int32_t* d_right, void* d_workspace, uint64_t* d_transfer, int32_t* d_each,
                                       void* hip_stream) {
  if (n < 4 || n > kNjMaxN) return refuse("tree_transfer: the launch takes 4 to 16384 leaves");
  if (!count || count > kBootChunkReplicates) return refuse("tree_transfer: the launch takes 1 to 32768 replicate trees");
  if (!splits || splits > 2 * n - 2) return refuse("tree_transfer: the launch takes 1 to 2n - 2 runs");
  if (!d_pos || !d_split || !d_left || !d_right || !d_workspace || !d_transfer) return refuse("tree_transfer: a missing argument");
  if ((uintptr_t)d_workspace & 255) return refuse("tree_transfer: the workspace must be 256-byte aligned");
  static_assert(sizeof(transfer_split) == 8 && sizeof(unsigned long long) == 8, "the runs are pairs of uint32, the sums 64 bits");
  return transfer_launch(n, count, splits, d_pos, (const transfer_split*)d_split, d_left, d_right, d_workspace, (unsigned long long*)d_transfer, d_each,
                         (hipStream_t)hip_stream);
}

extern "C" int dafs_host_transfer_runs(uint32_t n, const int32_t* left, const int32_t* right, uint32_t* pos, uint32_t* lo, uint32_t* len) {
  if (!n || !left || !right || !pos || !lo || !len) return refuse("transfer_runs: a missing argument");
  if (const char* bad = tree_malformed(n, left, right)) {
    char msg[160];
    snprintf(msg, sizeof msg, "transfer_runs: %s", bad);
    return refuse(msg);
  }
  try {
    const support_counter counter(n, left, right);
    std::vector<uint32_t> vlo, vlen;
    counter.runs(left, right, vlo, vlen);
    memcpy(pos, counter.positions().data(), (size_t)n * 4);
    memcpy(lo, vlo.data(), vlo.size() * 4);
    memcpy(len, vlen.data(), vlen.size() * 4);
  } catch (const std::bad_alloc&) {
    return DAFS_HIP_ENOMEM;
  }
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_tree_transfer(dafs_hip_ctx* c, uint32_t n, const int32_t* main_left, const int32_t* main_right, uint32_t B,
                                      const int32_t* rep_left, const int32_t* rep_right, int64_t* transfer, int32_t* transfer_each) {
  if (!c || !main_left || !main_right || !rep_left || !rep_right || !transfer) return refuse("tree_transfer: a missing argument");
  if (n == 0 || n > kNjMaxN) return refuse("tree_transfer: it takes 1 to 16384 leaves");
  if (B == 0 || B > kBootMaxReplicates) return refuse("tree_transfer: it takes 1 to 65536 replicate trees");
  char msg[200];
  if (const char* bad = tree_malformed(n, main_left, main_right)) {
    snprintf(msg, sizeof msg, "tree_transfer: the main tree: %s", bad);
    return refuse(msg);
  }
  const size_t T = 2 * (size_t)n - 1;
  for (uint32_t k = 0; k < B; ++k)
    if (const char* bad = tree_malformed(n, rep_left + k * T, rep_right + k * T)) {
      snprintf(msg, sizeof msg, "tree_transfer: replicate %u: %s", k, bad);
      return refuse(msg);
    }
  if (n <= 3) {  // no split with two leaves on either side: nothing is launched
    for (size_t v = 0; v < T; ++v) transfer[v] = -1;
    if (transfer_each)
      for (size_t v = 0; v < (size_t)B * T; ++v) transfer_each[v] = -1;
    return DAFS_HIP_OK;
  }
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  try {
    const support_counter counter(n, main_left, main_right);
    const transfer_plan plan(n, counter, main_left, main_right);
    const uint32_t S = plan.splits();
    // trees per chunk under the byte budget of dafs_hip_alignment_bootstrap: the two arrays, the sets and ranks, the indices
    const size_t per = T * 8 + transfer_per_tree_bytes(n) + sizeof(transfer_head) + (transfer_each ? (size_t)S * 4 : 0);
    const uint32_t chunk = (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(B, kBootChunkReplicates), boot_byte_budget() / per));
    std::vector<unsigned long long> sum(S);
    std::vector<transfer_head> heads;
    std::vector<int32_t> each(transfer_each ? (size_t)B * S : 0);  // the caller's stay untouched by a refusal
    call_frame f(c);
    void *d_pos, *d_split, *d_sum, *d_tws, *d_left, *d_right, *d_each = nullptr;
    if (!(d_pos = f.alloc((size_t)n * 4)) || !(d_split = f.alloc((size_t)S * sizeof(transfer_split))) || !(d_sum = f.alloc((size_t)S * 8)) ||
        !(d_tws = f.alloc(transfer_workspace_bytes(n, chunk))) || !(d_left = f.alloc(chunk * T * 4)) || !(d_right = f.alloc(chunk * T * 4)) ||
        (transfer_each && !(d_each = f.alloc((size_t)chunk * S * 4))))
      return DAFS_HIP_ENOMEM;
    if (f.up(d_pos, plan.pos.data(), (size_t)n * 4) || f.up(d_split, plan.split.data(), (size_t)S * sizeof(transfer_split)) ||
        f.fill(d_sum, 0, (size_t)S * 8))
      return DAFS_HIP_ELAUNCH;
    for (uint32_t k0 = 0; k0 < B; k0 += chunk) {
      const uint32_t count = std::min(chunk, B - k0);
      if (f.up(d_left, rep_left + k0 * T, count * T * 4) || f.up(d_right, rep_right + k0 * T, count * T * 4)) return DAFS_HIP_ELAUNCH;
      if (int rc = transfer_launch(n, count, S, (const uint32_t*)d_pos, (const transfer_split*)d_split, (const int32_t*)d_left,
                                   (const int32_t*)d_right, d_tws, (unsigned long long*)d_sum, (int32_t*)d_each, f.st))
        return rc;
      heads.resize(count);
      if (f.down(heads.data(), d_tws, (size_t)count * sizeof(transfer_head)) ||
          (transfer_each && f.down(&each[(size_t)k0 * S], d_each, (size_t)count * S * 4)) || f.finish())
        return DAFS_HIP_ELAUNCH;
      if (int rc = transfer_verdict("tree_transfer", k0, heads)) return rc;
    }
    if (f.down(sum.data(), d_sum, (size_t)S * 8) || f.finish()) return DAFS_HIP_ELAUNCH;
    plan.result(n, sum, transfer);
    if (transfer_each) {
      for (size_t v = 0; v < (size_t)B * T; ++v) transfer_each[v] = -1;
      for (uint32_t k = 0; k < B; ++k)
        for (uint32_t s = 0; s < S; ++s) transfer_each[k * T + plan.node[s]] = each[(size_t)k * S + s];
    }
  } catch (const std::bad_alloc&) {
    return DAFS_HIP_ENOMEM;
  }
  return DAFS_HIP_OK;
}
