// dafs_amd/csrc/capi_reliability.cpp -- dafs_hip_alignment_reliability: per-residue, per-column and per-consensus-pair
// reliability of an alignment from the context's matching and base-pairing stores (reliability.hip).  The reference has no
// counterpart: DAFS prints an alignment and a structure and no sign of which parts of them to trust.
//
// Host work: the checks, the rows put into ascending sequence order (the order every sum is stated in, so the order the
// caller gives the rows in changes no bit), the blocks of 64 residues, and the expected accuracy, which folds the residue
// values one by one in that order.
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>

#include "../../include/dafs_hip.h"
#include "ctx.h"
#include "hip_util.h"
#include "reliability.h"

using namespace dafs;

extern "C" int dafs_hip_alignment_reliability(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint32_t* seq, const uint8_t* mask,
                                              const uint32_t* ss, int mp_relaxed, int bp_relaxed, double* res_rel, double* col_rel,
                                              double* pair_rel, uint32_t* pair_rows, double* expected_accuracy) {
  if (!c || !n || !len || !seq || !mask) return DAFS_HIP_EINVAL;
  if (mp_relaxed > 1 || bp_relaxed > 1) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const uint32_t N = (uint32_t)c->len.size();
  // rows: known sequences, each once, one family, and a mask that places every residue of its sequence
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  for (uint32_t r = 0; r < n; ++r)
    if (seq[r] >= N) return DAFS_HIP_EINVAL;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return seq[a] < seq[b]; });
  for (uint32_t k = 1; k < n; ++k)
    if (seq[order[k]] == seq[order[k - 1]] || !c->fam.same_family(seq[order[0]], seq[order[k]])) return DAFS_HIP_EINVAL;
  std::vector<uint32_t> sseq(n);
  std::vector<uint64_t> res_off(n + 1, 0);
  std::vector<uint8_t> smask((size_t)n * len);
  std::vector<uint2> blocks;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t r = order[k];
    const uint8_t* m = mask + (size_t)r * len;
    uint32_t cnt = 0;
    for (uint32_t col = 0; col < len; ++col) cnt += m[col] ? 1 : 0;
    if (cnt != c->len[seq[r]]) return DAFS_HIP_EINVAL;
    sseq[k] = seq[r];
    res_off[k + 1] = res_off[k] + cnt;
    memcpy(smask.data() + (size_t)k * len, m, len);
    for (uint32_t i0 = 0; i0 < cnt; i0 += 64) blocks.push_back(make_uint2(k, i0));
  }
  const uint64_t total = res_off[n];
  // ss: left column -> right column, each column in at most one pair
  if (ss) {
    std::vector<uint8_t> used(len, 0);
    for (uint32_t col = 0; col < len; ++col) {
      const uint32_t p = ss[col];
      if (p == DAFS_HIP_NONE) continue;
      if (p <= col || p >= len || used[col] || used[p]) return DAFS_HIP_EINVAL;
      used[col] = used[p] = 1;
    }
  }
  // the stores: negative = the one the progressive phase reads now; a matching store must hold every pair of the context
  const int m = mp_relaxed < 0 ? c->cur_mp : mp_relaxed;
  const int b = bp_relaxed < 0 ? c->cur_bp : bp_relaxed;
  if (n > 1 && (!c->mp[m].valid || c->mp[m].n_tasks != c->fam.npairs())) return DAFS_HIP_EINVAL;
  if (n > 1 && c->mp[m].listed) return DAFS_HIP_EINVAL;  // dafs_hip_consistency_match_pairs: the unlisted pairs are empty, not zero
  if (ss && !c->bp[b].valid) return DAFS_HIP_EINVAL;

  // device workspace, carved from c->work
  size_t used = 0;
  auto take = [&](size_t bytes) { const size_t at = used; used += (bytes + 255) & ~(size_t)255; return at; };
  const size_t o_seq = take((size_t)n * 4), o_off = take((size_t)(n + 1) * 8), o_blk = take(blocks.size() * 8 + 8);
  const size_t o_ss = take((size_t)len * 4), o_mask = take((size_t)n * len), o_pos = take((size_t)n * len * 4);
  const size_t o_col = take(total * 4), o_res = take(total * 8), o_crel = take((size_t)len * 8), o_prel = take((size_t)len * 8);
  const size_t o_prows = take((size_t)len * 4);
  int rc;
  if ((rc = c->work.reserve(used + 256))) return rc;
  uint8_t* w = c->work.ptr;
  rel_args a;
  memset(&a, 0, sizeof a);
  if (n > 1) a.mp = c->mp_view(c->mp[m]);
  if (ss) a.bp = c->bp[b].view();
  a.seq = (const uint32_t*)(w + o_seq);
  a.res_off = (const uint64_t*)(w + o_off);
  a.blocks = (const uint2*)(w + o_blk);
  a.ss = ss ? (const uint32_t*)(w + o_ss) : nullptr;
  a.pos = (uint32_t*)(w + o_pos);
  a.col_of = (uint32_t*)(w + o_col);
  a.res_rel = (double*)(w + o_res);
  a.col_rel = (double*)(w + o_crel);
  a.pair_rel = (double*)(w + o_prel);
  a.pair_rows = (uint32_t*)(w + o_prows);
  a.n = n; a.len = len; a.nblocks = (uint32_t)blocks.size();
  hipStream_t st = c->stream;
  auto up = [&](size_t off, const void* src, size_t bytes) { return bytes && hip_check(hipMemcpyAsync(w + off, src, bytes, hipMemcpyHostToDevice, st)); };
  if (up(o_seq, sseq.data(), (size_t)n * 4) || up(o_off, res_off.data(), (size_t)(n + 1) * 8) || up(o_blk, blocks.data(), blocks.size() * 8) ||
      (ss && up(o_ss, ss, (size_t)len * 4)) || up(o_mask, smask.data(), smask.size()))
    return DAFS_HIP_ELAUNCH;
  if ((rc = rel_launch(a, w + o_mask, st))) return rc;
  std::vector<double> rel(total);
  if (hip_check(hipMemcpyAsync(rel.data(), a.res_rel, total * 8, hipMemcpyDeviceToHost, st))) return DAFS_HIP_ELAUNCH;
  if (col_rel && hip_check(hipMemcpyAsync(col_rel, a.col_rel, (size_t)len * 8, hipMemcpyDeviceToHost, st))) return DAFS_HIP_ELAUNCH;
  if (pair_rel && hip_check(hipMemcpyAsync(pair_rel, a.pair_rel, (size_t)len * 8, hipMemcpyDeviceToHost, st))) return DAFS_HIP_ELAUNCH;
  if (pair_rows && hip_check(hipMemcpyAsync(pair_rows, a.pair_rows, (size_t)len * 4, hipMemcpyDeviceToHost, st))) return DAFS_HIP_ELAUNCH;
  if (hip_check(hipStreamSynchronize(st))) return DAFS_HIP_ELAUNCH;  // the host vectors above stay alive until here
  if (res_rel) {  // back into the caller's row order
    std::vector<uint64_t> given_off(n + 1, 0);
    for (uint32_t r = 0; r < n; ++r) given_off[r + 1] = given_off[r] + c->len[seq[r]];
    for (uint32_t k = 0; k < n; ++k)
      memcpy(res_rel + given_off[order[k]], rel.data() + res_off[k], (res_off[k + 1] - res_off[k]) * 8);
  }
  if (expected_accuracy) {
    double s = 0.0;
    for (uint64_t k = 0; k < total; ++k) s += rel[k];
    *expected_accuracy = s / (double)total;
  }
  return DAFS_HIP_OK;
}
