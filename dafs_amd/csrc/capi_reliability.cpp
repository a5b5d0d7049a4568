// dafs_amd/csrc/capi_reliability.cpp -- dafs_hip_alignment_reliabilities: per-residue, per-column and per-consensus-pair
// reliability of many alignments from the context's matching and base-pairing stores (reliability.hip), in chunks under a
// budget of device memory, three launches and one copy each way per chunk; dafs_hip_alignment_reliability is the batch of
// one.  The reference has no counterpart: DAFS prints an alignment and a structure and no sign of which parts of them to
// trust.
//
// Host work: the checks, the rows put into ascending sequence order (the order every sum is stated in, so the order the
// caller gives the rows in changes no bit), the blocks of 64 residues of the wanted rows, and the expected accuracy, which
// folds the residue values one by one in that order.  Everything is checked before the first launch.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <limits>
#include <numeric>
#include <vector>

#include "../../include/dafs_hip.h"
#include "call_frame.h"
#include "call_host.h"
#include "reliability.h"

using namespace dafs;

namespace {

// The device workspace of one chunk, carved from c->work: what is uploaded, what comes back, then the maps.
struct rel_carve : carve {
  size_t o_alns, o_rows, o_blk, o_cblk, o_ss, o_mask, head_bytes, o_res, o_crel, o_prel, o_prows, out_bytes, o_pos, o_col;
  rel_carve(size_t alns, size_t rows, size_t blocks, size_t col_blocks, size_t cols, size_t cells, size_t wanted, size_t residues, bool ss) {
    o_alns = take(alns * sizeof(rel_aln)); o_rows = take(rows * sizeof(rel_row)); o_blk = take(blocks * 8); o_cblk = take(col_blocks * 8);
    o_ss = take(ss ? cols * 4 : 0); o_mask = take(cells);
    head_bytes = top;
    o_res = take(wanted * 8); o_crel = take(cols * 8); o_prel = take(cols * 8); o_prows = take(cols * 4);
    out_bytes = top - o_res;
    o_pos = take(cells * 4); o_col = take(residues * 4);
  }
};

}  // namespace

extern "C" int dafs_hip_alignment_reliabilities(dafs_hip_ctx* c, uint32_t nalign, const uint32_t* n_rows, const uint32_t* len, const uint32_t* seq,
                                                const uint8_t* mask, const uint32_t* ss, const uint8_t* want, int mp_relaxed, int bp_relaxed,
                                                double* res_rel, double* col_rel, double* pair_rel, uint32_t* pair_rows,
                                                double* expected_accuracy) {
  if (!c) return DAFS_HIP_EINVAL;
  if (nalign == 0) return DAFS_HIP_OK;
  if (!n_rows || !len || !seq || !mask) return DAFS_HIP_EINVAL;
  if (mp_relaxed > 1 || bp_relaxed > 1 || c->fold_pending) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const uint32_t N = (uint32_t)c->len.size();
  // ---- everything the launches will read, checked on the host first ----
  // the stores: negative = the one the progressive phase reads now
  const mp_store& mps = c->mp[mp_relaxed < 0 ? c->cur_mp : mp_relaxed];
  const bp_store& bps = c->bp[bp_relaxed < 0 ? c->cur_bp : bp_relaxed];
  if (ss && !bps.valid) return DAFS_HIP_EINVAL;
  std::vector<size_t> row0(nalign + 1, 0), mask0(nalign + 1, 0), col0(nalign + 1, 0);
  std::vector<uint64_t> bytes(nalign);
  for (uint32_t a = 0; a < nalign; ++a) {
    if (!n_rows[a] || !len[a]) return DAFS_HIP_EINVAL;
    row0[a + 1] = row0[a] + n_rows[a];
    mask0[a + 1] = mask0[a] + (size_t)n_rows[a] * len[a];
    col0[a + 1] = col0[a] + len[a];
    bytes[a] = dafs_host_reliability_bytes(n_rows[a], len[a]);
  }
  const size_t R = row0[nalign];
  if (R > 0x7fffffffull) return DAFS_HIP_EOVERFLOW;
  // rows: known sequences, each once in its alignment, one family, and a mask that places every residue of its sequence;
  // order[]: per alignment its rows (indices into the caller's) in ascending sequence order, the order every sum is stated in
  std::vector<uint64_t> given_res0(R + 1, 0);  // the caller's res_rel: first residue of each row
  for (size_t r = 0; r < R; ++r) {
    if (seq[r] >= N) return DAFS_HIP_EINVAL;
    given_res0[r + 1] = given_res0[r] + c->len[seq[r]];
  }
  std::vector<uint32_t> order(R);
  std::iota(order.begin(), order.end(), 0u);
  std::vector<uint8_t> all_wanted(nalign, 1), used;
  for (uint32_t a = 0; a < nalign; ++a) {
    const uint32_t n = n_rows[a], L = len[a];
    uint32_t* o = order.data() + row0[a];
    std::sort(o, o + n, [&](uint32_t p, uint32_t q) { return seq[p] < seq[q]; });
    for (uint32_t k = 1; k < n; ++k)
      if (seq[o[k]] == seq[o[k - 1]] || !c->fam.same_family(seq[o[0]], seq[o[k]])) return DAFS_HIP_EINVAL;
    for (uint32_t r = 0; r < n; ++r) {
      const uint8_t* m = mask + mask0[a] + (size_t)r * L;
      uint32_t cnt = 0;
      for (uint32_t col = 0; col < L; ++col) cnt += m[col] ? 1 : 0;
      if (cnt != c->len[seq[row0[a] + r]]) return DAFS_HIP_EINVAL;
      if (want && !want[row0[a] + r]) all_wanted[a] = 0;
    }
    if (ss && !structure_ok(ss + col0[a], L, used)) return DAFS_HIP_EINVAL;
    if (n > 1) {  // the matching store: whole, and holding every pair of a wanted row with another row of the alignment
      if (!mps.valid || mps.n_tasks != c->fam.npairs()) return DAFS_HIP_EINVAL;
      if (mps.listed)
        for (uint32_t k = 0; k < n; ++k) {
          if (want && !want[o[k]]) continue;
          for (uint32_t q = 0; q < n; ++q) {
            if (q == k) continue;
            const uint32_t lo = seq[o[std::min(k, q)]], hi = seq[o[std::max(k, q)]];
            if (!mps.holds(c->fam.seq[lo].row_base + (hi - lo - 1))) return DAFS_HIP_EINVAL;
          }
        }
    }
  }
  // tests: budgets that put every alignment in a chunk of its own
  const uint64_t budget = env_uint("DAFS_HIP_REL_BATCH_BYTES", 0, UINT64_MAX, dafs_host_reliability_batch_bytes());
  std::vector<uint32_t> chunk_of(nalign);
  int rc;
  if ((rc = dafs_host_pack_greedy(nalign, bytes.data(), budget, chunk_of.data()))) return rc;

  // every chunk's carving against its estimate, and the workspace of the largest, before the first launch
  size_t work_bytes = 0;
  for (uint32_t a0 = 0; a0 < nalign;) {
    uint32_t a1 = a0;
    uint64_t estimate = 0, residues = 0, wanted = 0;
    size_t nblocks = 0, ncol_blocks = 0;
    for (; a1 < nalign && chunk_of[a1] == chunk_of[a0]; ++a1) {
      estimate += bytes[a1];
      ncol_blocks += (len[a1] + 63) / 64;
      for (size_t r = row0[a1]; r < row0[a1 + 1]; ++r) {
        const uint32_t nres = c->len[seq[r]];
        residues += nres;
        if (want && !want[r]) continue;
        wanted += nres;
        nblocks += (nres + 63) / 64;
      }
    }
    const rel_carve cv(a1 - a0, row0[a1] - row0[a0], nblocks, ncol_blocks, col0[a1] - col0[a0], mask0[a1] - mask0[a0], wanted, residues,
                       ss != nullptr);
    if (cv.reserve_bytes() > estimate) {  // dafs_host_reliability_bytes is the bound of this carving
      fprintf(stderr, "dafs_hip: a chunk of %u alignments takes %zu bytes, over its estimate of %llu\n", a1 - a0, cv.reserve_bytes(),
              (unsigned long long)estimate);
      return DAFS_HIP_ELAUNCH;
    }
    work_bytes = std::max(work_bytes, cv.reserve_bytes());
    a0 = a1;
  }
  if ((rc = c->work.reserve(work_bytes))) return rc;

  std::vector<rel_aln> alns;
  std::vector<rel_row> rows;
  std::vector<uint2> blocks, col_blocks;
  std::vector<uint8_t> head, out;
  call_frame f(c);  // `head` and `out` are in flight when an error ends a chunk early
  for (uint32_t a0 = 0; a0 < nalign;) {
    uint32_t a1 = a0;
    while (a1 < nalign && chunk_of[a1] == chunk_of[a0]) ++a1;
    const uint32_t m = a1 - a0;
    const size_t nrow = row0[a1] - row0[a0], cells = mask0[a1] - mask0[a0], cols = col0[a1] - col0[a0];
    // the chunk's descriptors and work lists
    alns.assign(m, rel_aln());
    rows.assign(nrow, rel_row());
    blocks.clear();
    col_blocks.clear();
    uint64_t residues = 0, wanted = 0;
    bool pairs = false;
    for (uint32_t a = a0; a < a1; ++a) {
      rel_aln& al = alns[a - a0];
      al.row0 = row0[a] - row0[a0]; al.cell0 = mask0[a] - mask0[a0]; al.col0 = col0[a] - col0[a0];
      al.n = n_rows[a]; al.len = len[a]; al.all_wanted = all_wanted[a]; al.pad = 0;
      pairs |= al.n > 1;
      for (uint32_t k = 0; k < al.n; ++k) {
        const uint32_t g = order[row0[a] + k];  // the caller's row
        rel_row& row = rows[al.row0 + k];
        row.aln = a - a0; row.seq = seq[g]; row.nres = c->len[seq[g]]; row.pad = 0;
        row.res0 = residues; row.rel0 = wanted;
        residues += row.nres;
        if (want && !want[g]) continue;
        wanted += row.nres;
        for (uint32_t i0 = 0; i0 < row.nres; i0 += 64) blocks.push_back(make_uint2((uint32_t)(al.row0 + k), i0));
      }
      for (uint32_t c0 = 0; c0 < al.len; c0 += 64) col_blocks.push_back(make_uint2(a - a0, c0));
    }
    const rel_carve cv(m, nrow, blocks.size(), col_blocks.size(), cols, cells, wanted, residues, ss != nullptr);
    const size_t o_alns = cv.o_alns, o_rows = cv.o_rows, o_blk = cv.o_blk, o_cblk = cv.o_cblk, o_ss = cv.o_ss, o_mask = cv.o_mask;
    const size_t o_res = cv.o_res, o_crel = cv.o_crel, o_prel = cv.o_prel, o_prows = cv.o_prows, o_pos = cv.o_pos, o_col = cv.o_col;
    const size_t head_bytes = cv.head_bytes, out_bytes = cv.out_bytes;
    uint8_t* w = c->work.ptr;
    head.assign(head_bytes, 0);
    memcpy(head.data() + o_alns, alns.data(), (size_t)m * sizeof(rel_aln));
    memcpy(head.data() + o_rows, rows.data(), nrow * sizeof(rel_row));
    if (!blocks.empty()) memcpy(head.data() + o_blk, blocks.data(), blocks.size() * 8);
    memcpy(head.data() + o_cblk, col_blocks.data(), col_blocks.size() * 8);
    if (ss) memcpy(head.data() + o_ss, ss + col0[a0], cols * 4);
    for (uint32_t a = a0; a < a1; ++a)  // the rows' masks in the sorted order
      for (uint32_t k = 0; k < n_rows[a]; ++k)
        memcpy(head.data() + o_mask + alns[a - a0].cell0 + (size_t)k * len[a], mask + mask0[a] + (size_t)(order[row0[a] + k] - row0[a]) * len[a], len[a]);
    rel_args g;
    memset(&g, 0, sizeof g);
    if (pairs) g.mp = c->mp_view(mps);
    if (ss) g.bp = bps.view();
    g.alns = (const rel_aln*)(w + o_alns);
    g.rows = (const rel_row*)(w + o_rows);
    g.mask = w + o_mask;
    g.blocks = (const uint2*)(w + o_blk);
    g.col_blocks = (const uint2*)(w + o_cblk);
    g.ss = ss ? (const uint32_t*)(w + o_ss) : nullptr;
    g.pos = (uint32_t*)(w + o_pos);
    g.col_of = (uint32_t*)(w + o_col);
    g.res_rel = (double*)(w + o_res);
    g.col_rel = (double*)(w + o_crel);
    g.pair_rel = (double*)(w + o_prel);
    g.pair_rows = (uint32_t*)(w + o_prows);
    g.nrows = (uint32_t)nrow; g.nblocks = (uint32_t)blocks.size(); g.ncol_blocks = (uint32_t)col_blocks.size();
    if (f.up(w, head.data(), head_bytes)) return DAFS_HIP_ELAUNCH;
    if ((rc = rel_launch(g, f.st))) return rc;
    out.resize(out_bytes);
    if (f.down(out.data(), w + o_res, out_bytes)) return DAFS_HIP_ELAUNCH;
    if ((rc = f.finish())) return rc;  // per chunk: the next one rewrites `head`
    const double* rel = (const double*)out.data();
    if (col_rel) memcpy(col_rel + col0[a0], out.data() + (o_crel - o_res), cols * 8);
    if (pair_rel) memcpy(pair_rel + col0[a0], out.data() + (o_prel - o_res), cols * 8);
    if (pair_rows) memcpy(pair_rows + col0[a0], out.data() + (o_prows - o_res), cols * 4);
    for (uint32_t a = a0; a < a1; ++a) {
      const rel_aln& al = alns[a - a0];
      if (res_rel)  // back into the caller's row order
        for (uint32_t k = 0; k < al.n; ++k) {
          const uint32_t gr = order[row0[a] + k];
          if (want && !want[gr]) continue;
          const rel_row& row = rows[al.row0 + k];
          memcpy(res_rel + given_res0[gr], rel + row.rel0, (size_t)row.nres * 8);
        }
      if (expected_accuracy) {  // the residue values folded one by one in the sorted order
        if (al.all_wanted) {
          const rel_row &first = rows[al.row0], &last = rows[al.row0 + al.n - 1];
          const uint64_t total = last.rel0 + last.nres - first.rel0;
          double s = 0.0;
          for (uint64_t k = 0; k < total; ++k) s += rel[first.rel0 + k];
          expected_accuracy[a] = s / (double)total;
        } else {
          expected_accuracy[a] = std::numeric_limits<double>::quiet_NaN();
        }
      }
    }
    a0 = a1;
  }
  return DAFS_HIP_OK;
}

// one alignment: the batch of one
extern "C" int dafs_hip_alignment_reliability(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint32_t* seq, const uint8_t* mask,
                                              const uint32_t* ss, int mp_relaxed, int bp_relaxed, double* res_rel, double* col_rel,
                                              double* pair_rel, uint32_t* pair_rows, double* expected_accuracy) {
  if (!c || !n || !len || !seq || !mask) return DAFS_HIP_EINVAL;
  return dafs_hip_alignment_reliabilities(c, 1, &n, &len, seq, mask, ss, nullptr, mp_relaxed, bp_relaxed, res_rel, col_rel, pair_rel, pair_rows,
                                          expected_accuracy);
}
