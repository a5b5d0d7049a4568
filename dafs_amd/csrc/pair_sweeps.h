// dafs_amd/csrc/pair_sweeps.h -- the model-independent parts of the pair-posterior kernels.
//
// Both alignment models (ProbCons pairhmm3.hip, CONTRAlign pairhmm5.hip) leave one float per DP
// cell in plane 0 of the wave's slab, indexed [(step*W + c)*64 + lane] in the skewed layout
// described in pairhmm3.hip.  pair_finish turns that plane into the sparse outputs:
//   sweep 3: p = post(slab value); threshold (wrapper >= th, adapter > th: reference
//            src/align.cpp:69-78); similarity-score DP (src/dafs.cpp:713-764); entry counts per
//            row (carried lane to lane with the row) and per column (registers)
//   sweep 4: the CSR of mp[x][y] and of mp[y][x] (src/dafs.cpp:155-167), staged in LDS a window of positions at a
//            time and copied out coalesced (k_pairhmm3), or scattered entry by entry (k_pairhmm5, and the
//            plane-and-rescan fallback of both)
//
// Column ownership.  A kernel instance is compiled for W columns per lane, but a wavefront whose
// pairs are short enough runs the W-1 instantiation of every sweep (lane t owns columns
// t*WR .. t*WR+WR-1, WR = W or W-1; the slab keeps stride W).  Lengths inside one batch differ by a few
// per cent (the benchmark sets: +-7 %), and with 5 instead of 6 columns that is 17 % of the cells.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "../../include/dafs_hip.h"
#include "hip_util.h"

namespace dafs {

// Neighbour exchange inside a group of G lanes: value of lane t-1 (shift_up1) or t+1 (shift_down1),
// `fill` at the group boundary.  One DPP move on the vector pipe, no LDS round trip: a group of 16 is
// one DPP row (row_shr:1 / row_shl:1, the boundary keeps `fill`); wider groups use the whole-wave
// shift of gfx9 (wave_shr:1 / wave_shl:1) and, for G = 32, one select for the lane at the seam.
__device__ __forceinline__ int dpp_row_shr1(int fill, int v) { return __builtin_amdgcn_update_dpp(fill, v, 0x111, 0xF, 0xF, false); }
__device__ __forceinline__ int dpp_row_shl1(int fill, int v) { return __builtin_amdgcn_update_dpp(fill, v, 0x101, 0xF, 0xF, false); }
__device__ __forceinline__ int dpp_wave_shr1(int fill, int v) { return __builtin_amdgcn_update_dpp(fill, v, 0x138, 0xF, 0xF, false); }
__device__ __forceinline__ int dpp_wave_shl1(int fill, int v) { return __builtin_amdgcn_update_dpp(fill, v, 0x130, 0xF, 0xF, false); }

template <int G>
__device__ __forceinline__ int shift_up1(int v, int fill, int t) {
  if constexpr (G == 16) return dpp_row_shr1(fill, v);
  const int r = dpp_wave_shr1(fill, v);
  if constexpr (G == 64) return r;
  return t == 0 ? fill : r;
}
template <int G>
__device__ __forceinline__ float shift_up1(float v, float fill, int t) {
  return __int_as_float(shift_up1<G>(__float_as_int(v), __float_as_int(fill), t));
}
template <int G>
__device__ __forceinline__ int shift_down1(int v, int fill, int t) {
  if constexpr (G == 16) return dpp_row_shl1(fill, v);
  const int r = dpp_wave_shl1(fill, v);
  if constexpr (G == 64) return r;
  return t == G - 1 ? fill : r;
}
template <int G>
__device__ __forceinline__ float shift_down1(float v, float fill, int t) {
  return __int_as_float(shift_down1<G>(__float_as_int(v), __float_as_int(fill), t));
}

// Columns per lane for this wavefront: W, or W-1 when every pair of the wave fits (wave-uniform, in an SGPR).
template <int G, int W>
__device__ __forceinline__ int pair_width(int L2) {
  if constexpr (W == 1) return 1;
  int m = L2;
#pragma unroll
  for (int o = G; o < 64; o <<= 1) m = max(m, __shfl_xor(m, o));
  m = __builtin_amdgcn_readfirstlane(m);
  return (m + 1 <= G * (W - 1)) ? W - 1 : W;
}

// WR = columns this wave's lanes own (W or W-1, compile time here: the kernels branch once per pair on pair_width and
// instantiate every sweep for both), W = slab stride.  post(sv, p) turns the WR slab values of a step into posteriors.
//
// Entries are rare (a few per row), so sweep 3 does not write the thresholded plane back for a fourth sweep over every
// cell to re-read: a lane with at least one entry in a step appends ONE record for that step to a private list (`list`: a
// second plane of the wave's scratch), {entry mask of its WR cells, row-1 | entries of the row left of its columns << 16,
// the WR posteriors}, padded to whole 16-byte words (WR <= 6: 32 bytes, two 16-byte buffer stores that every lane
// issues in every step and the range check drops for the lanes without a record: no branch), and sweep 4 walks the
// lists four records at a time, rebuilding an entry's position in its row from the carried count plus the mask's lower
// bits and its position in its column from a running position per column -- a third less HBM traffic for the whole
// kernel, and one list step per lane-step with entries instead of ~190 grid steps.  The positions index a window of
// the pair's pool region staged in LDS (`stage`, E positions; the launch derives E: pair_emit_window below).  A lane
// whose list is full (entries in most of its steps: th near 0) makes the call return false with nothing emitted and
// the slab untouched; the caller then runs the dense = true instantiation, which is the plane-and-rescan form.
template <int WR>
struct pair_rec {
  static constexpr int Q = (2 + WR + 3) / 4;  // 16-byte words per record
  static constexpr int D = 4 * Q;             // dwords per record (a lane's list holds list_cap / D records)
};
// staged: sweep 4 of the sparse form goes through windows staged in LDS (`stage`, E positions; k_pairhmm3) or scatters
// every entry from its lane (k_pairhmm5, which passes no stage).
//
// picked = true (k_pairhmm3, pairhmm3.hip "sweep 2p"): the backward sweep has stored no plane.  `slab` is then the plane
// of the lanes' CANDIDATE lists ({candidate mask, row, the WR sums F + B}, ncand records in descending row order, only
// the lane-steps with a cell that can reach th) and `list` the plane the final records go to; sweep 3 becomes
//   3b: every lane walks its own candidate list, two records per turn: p = post(sums), exact entry mask
//       = candidate && p >= th && p > th, the record goes back in place as {entry mask, row, p}
//   3c: the step of sweep 3 without slab loads and without post: a lane takes the entry mask and the posteriors of row
//       i from the record of that row (consumed from its last record downwards, i.e. rows ascending) and an empty
//       mask otherwise; similarity DP, counts, row pointers and the final records are those of sweep 3.
// The final records are a subset of the candidate records, so a list that held the candidates holds them too.
template <int G, int W, int WR, bool dense, bool staged, bool picked = false, class Args, class Post>
__device__ __forceinline__ bool pair_finish(const Args& a, float* __restrict__ slab, float* __restrict__ list, int list_cap, uint32_t* __restrict__ s_rowptr,
                                            uint2* __restrict__ stage, int E, int lane, int t, int g, int L1, int L2, int nsteps, bool act, uint32_t task,
                                            float th, Post post, int ncand = 0) {
  static_assert(!(picked && dense), "the candidate form is a sparse form");
  const int tlast = (L2 >= 0 ? L2 : 0) / WR;  // lane (within the group) that owns column L2
  const int j0 = t * WR;
  // The wave's list plane as a buffer.  Sweep 3: the record stores of a step are issued by every lane, and a lane without
  // a record gives an offset outside the buffer, which the range check drops without traffic.  Unconditional vector
  // stores keep the step free of branches around memory operations, so every wait of the loop can be counted (loads
  // and stores share one in-order counter; behind a branch the compiler has to wait for everything).  Sweep 4: a lane
  // that has run out of records reads outside the buffer and gets zeros, an empty entry mask.
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const __amdgpu_buffer_rsrc_t list_rs = __builtin_amdgcn_make_buffer_rsrc((void*)list, 0, list_cap * 256, 0x00020000);
  constexpr uint32_t NO_RECORD = 0x80000000u;  // beyond any list plane, and no wrap with the accesses' immediates
  // ------------------------------------------------------------------ sweep 3: posterior + sim + counts
  int colcnt[WR];
  float simv = 0.0f;
  uint32_t nnz = 0;
  int slab_nrec = 0;
  if constexpr (picked) {
    constexpr int Q = pair_rec<WR>::Q;
    const __amdgpu_buffer_rsrc_t cand_rs = __builtin_amdgcn_make_buffer_rsrc((void*)slab, 0, list_cap * 256, 0x00020000);
    auto rec_off = [lane](const int k, const bool have) { return have ? (uint32_t)(((uint32_t)k * Q * 64 + lane) * 16) : NO_RECORD; };
    // ---------------------------------------------------------------- sweep 3b: posteriors of the candidate records
    {
      int maxc = ncand;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) maxc = max(maxc, __shfl_xor(maxc, o));
      maxc = __builtin_amdgcn_readfirstlane(maxc);
      constexpr int K = 2;  // records per turn, their loads issued together
      for (int k0 = 0; k0 < maxc; k0 += K) {
        u32x4 r[K][Q];
#pragma unroll
        for (int kk = 0; kk < K; ++kk)
#pragma unroll
          for (int q = 0; q < Q; ++q) r[kk][q] = __builtin_amdgcn_raw_buffer_load_b128(cand_rs, (int)(rec_off(k0 + kk, k0 + kk < ncand) + q * 1024), 0, 0);
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
          uint32_t w[4 * Q];
#pragma unroll
          for (int q = 0; q < Q; ++q) { w[4 * q] = r[kk][q].x; w[4 * q + 1] = r[kk][q].y; w[4 * q + 2] = r[kk][q].z; w[4 * q + 3] = r[kk][q].w; }
          float sv[WR], pp[WR];
#pragma unroll
          for (int c = 0; c < WR; ++c) sv[c] = __uint_as_float(w[2 + c]);
          post(sv, pp);
          uint32_t exact = 0;  // wrapper (>= th keeps) then adapter (> th keeps), as in sweep 3
#pragma unroll
          for (int c = 0; c < WR; ++c) exact |= (uint32_t)((pp[c] >= th) && (pp[c] > th) ? 1 : 0) << c;
          w[0] &= exact;
#pragma unroll
          for (int c = 0; c < WR; ++c) w[2 + c] = __float_as_uint(pp[c]);
#pragma unroll
          for (int q = 0; q < Q; ++q) {  // a lane beyond its last record stores outside the buffer: dropped
            const u32x4 d = {w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
            __builtin_amdgcn_raw_buffer_store_b128(d, cand_rs, (int)(rec_off(k0 + kk, k0 + kk < ncand) + q * 1024), 0, 0);
          }
        }
      }
    }
#if defined(PAIR_EXP_STOP) && PAIR_EXP_STOP == 4  // tuning experiment: everything up to sweep 3b
    if (ncand != 12345) return true;
#endif
    // ---------------------------------------------------------------- sweep 3c: sim + counts from the records
    float pdp[WR];
    int ptr[WR];
#pragma unroll
    for (int c = 0; c < WR; ++c) { pdp[c] = 0.0f; ptr[c] = 0; colcnt[c] = 0; }
    float lastdp = 0.0f, dgdp = 0.0f;
    int lasttr = 0, dgtr = 0, lastcnt = 0;
    uint32_t rowacc = 0;
    if (t == G - 1) s_rowptr[0] = 0;
    int nrec = 0;  // final records of this lane
    // The lane's next record (the one with the lowest row not yet passed) waits in `cur`.  A step that consumes it
    // requests the one before it at once, into `pend`, which replaces `cur` at the top of the next step: a lane
    // consumes at most one record per step, and every lane issues the load in every step (outside the buffer where it
    // has consumed nothing), so the step has no branch around a memory operation and its waits are counted ones.
    int left = ncand;
    u32x4 cur[Q], pend[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) cur[q] = __builtin_amdgcn_raw_buffer_load_b128(cand_rs, (int)(rec_off(left - 1, left > 0) + q * 1024), 0, 0);
#pragma unroll
    for (int q = 0; q < Q; ++q) { asm volatile("" : "+v"(cur[q])); pend[q] = cur[q]; }
    bool took = false;
    for (int s = 0; s < nsteps; ++s) {
      const int i = s - t;
      const bool rowv = (i >= 0) && (i <= L1);
      if (took) {
#pragma unroll
        for (int q = 0; q < Q; ++q) cur[q] = pend[q];
      }
      const bool hit = left > 0 && (int)cur[0].y == i;
      left -= hit ? 1 : 0;
#pragma unroll
      for (int q = 0; q < Q; ++q) pend[q] = __builtin_amdgcn_raw_buffer_load_b128(cand_rs, (int)(rec_off(left - 1, hit && left > 0) + q * 1024), 0, 0);
      took = hit;
      uint32_t w[4 * Q];
#pragma unroll
      for (int q = 0; q < Q; ++q) { w[4 * q] = cur[q].x; w[4 * q + 1] = cur[q].y; w[4 * q + 2] = cur[q].z; w[4 * q + 3] = cur[q].w; }
      const uint32_t emask = hit ? w[0] : 0u;  // entries among the WR cells, bit c = cell c
      const float rdp = shift_up1<G>(lastdp, 0.0f, t);
      const int rtr = shift_up1<G>(lasttr, 0, t), rcnt = shift_up1<G>(lastcnt, 0, t);
      float ddp = dgdp, ldp = rdp;
      int dtr = dgtr, ltr = rtr, run = rcnt;
#pragma unroll
      for (int c = 0; c < WR; ++c) {  // the cell of sweep 3, with the entry bit and the posterior from the record
        const int j = j0 + c;
        const bool inner = rowv && (j <= L2) && i >= 1 && j >= 1;
        const bool entry = ((emask >> c) & 1u) != 0;
        const float p = __uint_as_float(w[2 + c]);
        const float udp = pdp[c];
        const int utr = ptr[c];
        const float dpe = entry ? ddp + p : -1.0f;
        const bool fl = dpe < ldp;
        float dp = fl ? ldp : dpe;
        int tr = fl ? ltr : dtr;
        const bool fu = dp < udp;
        dp = fu ? udp : dp;
        tr = (fu ? utr : tr) + 1;
        if (!inner) { dp = 0.0f; tr = 0; }
        ddp = udp; dtr = utr;
        pdp[c] = dp; ptr[c] = tr;
        ldp = dp; ltr = tr;
        const int e = entry ? 1 : 0;
        run += e;
        colcnt[c] += e;
      }
      {  // the step's final record (pair_rec): never more of them than candidate records, so it always fits
        w[0] = emask;
        w[1] = (uint32_t)((i - 1) | (rcnt << 16));
        const uint32_t ro = emask != 0 ? (uint32_t)(((uint32_t)nrec * Q * 64 + lane) * 16) : NO_RECORD;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          const u32x4 d = {w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]};
          __builtin_amdgcn_raw_buffer_store_b128(d, list_rs, (int)(ro + q * 1024), 0, 0);
        }
        nrec += emask != 0 ? 1 : 0;
      }
      dgdp = rdp; dgtr = rtr;
      lastdp = ldp; lasttr = ltr; lastcnt = run;
      if (i == L1 && t == tlast) {  // dafs.cpp:763; one lane of the group, once
        const int cl = L2 - j0;
        float sdp = 0.0f;
        int str = 1;
#pragma unroll
        for (int c = 0; c < WR; ++c)
          if (c == cl) { sdp = pdp[c]; str = ptr[c]; }
        simv = sdp / (float)str;
      }
      if (t == G - 1 && rowv && i >= 1) {  // row i is complete: its count has crossed the group
        rowacc += (uint32_t)run;
        s_rowptr[i] = rowacc;
      }
    }
    nnz = rowacc;
    slab_nrec = nrec;
  } else {
    float pdp[WR];
    int ptr[WR];
#pragma unroll
    for (int c = 0; c < WR; ++c) { pdp[c] = 0.0f; ptr[c] = 0; colcnt[c] = 0; }
    float lastdp = 0.0f, dgdp = 0.0f;
    int lasttr = 0, dgtr = 0, lastcnt = 0;
    uint32_t rowacc = 0;
    if (t == G - 1) s_rowptr[0] = 0;
    int nrec = 0;       // records in this lane's list
    bool ovf = false;
    // Slab values are fetched TWO steps ahead, into two register sets that take turns: the values a step starts with
    // were requested before the record stores of the step before, so waiting for them does not wait for those stores.
    // The last two steps refetch the last step's slots.
    float sva[WR], svb[WR];
#pragma unroll
    for (int c = 0; c < WR; ++c) sva[c] = slab[c * 64 + lane];
#pragma unroll
    for (int c = 0; c < WR; ++c) svb[c] = slab[(W + c) * 64 + lane];  // nsteps >= G >= 16: step 1 exists
    // both sets have arrived before the loop starts (the empty asm uses them), so the waits inside the loop count
    // what the loop itself has issued and not the order of these first requests
#pragma unroll
    for (int c = 0; c < WR; ++c) asm volatile("" : "+v"(sva[c]), "+v"(svb[c]));
    auto step = [&](const int s, float (&sv)[WR]) __attribute__((always_inline)) {
      const int i = s - t;
      const bool rowv = (i >= 0) && (i <= L1);
      float* __restrict__ slab_s = slab + (size_t)s * (W * 64);
      const float rdp = shift_up1<G>(lastdp, 0.0f, t);
      const int rtr = shift_up1<G>(lasttr, 0, t), rcnt = shift_up1<G>(lastcnt, 0, t);
      float ddp = dgdp, ldp = rdp;
      int dtr = dgtr, ltr = rtr, run = rcnt;
      float pp[WR];
      post(sv, pp);  // the model's posteriors of the WR cells, table reads batched
      {  // private slots: unguarded (cells outside the grid are ignored below)
        const float* __restrict__ slab_n = slab + (size_t)min(s + 2, nsteps - 1) * (W * 64);
#pragma unroll
        for (int c = 0; c < WR; ++c) sv[c] = slab_n[c * 64 + lane];
      }
      // One straight-line block for the WR cells (the posteriors' polynomials, the similarity DP and the counts as
      // selects: five independent chains the scheduler can interleave), then the step's record.  Written as per-cell
      // if / else, every cell becomes a handful of basic blocks and its polynomial waits for the cell before it.
      uint32_t emask = 0;  // entries among the WR cells, bit c = cell c
#pragma unroll
      for (int c = 0; c < WR; ++c) {
        const int j = j0 + c;
        const bool v = rowv && (j <= L2);
        const bool inner = v && i >= 1 && j >= 1;
        // wrapper (>= th keeps) then adapter (> th keeps): align.cpp:69-78
        const float p = pp[c];
        const bool entry = inner && (p >= th) && (p > th);
        if (dense) slab_s[c * 64 + lane] = entry ? p : 0.0f;
        // calculate_similarity_score, dafs.cpp:720-760: an entry starts from the diagonal (dp = ddp + p) and is replaced
        // by the left, then the upper neighbour where that is strictly larger; a non-entry starts from the left one.
        // Every dp is >= 0, so a start of -1 for a non-entry always takes the left neighbour.
        const float udp = pdp[c];
        const int utr = ptr[c];
        const float dpe = entry ? ddp + p : -1.0f;
        const bool fl = dpe < ldp;
        float dp = fl ? ldp : dpe;
        int tr = fl ? ltr : dtr;
        const bool fu = dp < udp;
        dp = fu ? udp : dp;
        tr = (fu ? utr : tr) + 1;
        if (!inner) { dp = 0.0f; tr = 0; }
        ddp = udp; dtr = utr;
        pdp[c] = dp; ptr[c] = tr;
        ldp = dp; ltr = tr;
        const int e = entry ? 1 : 0;
        run += e;
        colcnt[c] += e;
        emask |= (uint32_t)e << c;
      }
      if (!dense) {  // one record for the step (pair_rec), stored by the lanes that have entries and room for it
        const bool fits = (nrec + 1) * pair_rec<WR>::D <= list_cap;
        const bool app = emask != 0 && fits;
        ovf = ovf || (emask != 0 && !fits);
        float w[pair_rec<WR>::D];
        w[0] = __uint_as_float(emask);
        w[1] = __int_as_float((i - 1) | (rcnt << 16));
#pragma unroll
        for (int c = 0; c < WR; ++c) w[2 + c] = pp[c];
#pragma unroll
        for (int c = 2 + WR; c < pair_rec<WR>::D; ++c) w[c] = 0.0f;
        // 32-bit byte offset into the wave's list plane
        const uint32_t ro = app ? (uint32_t)(((uint32_t)nrec * pair_rec<WR>::Q * 64 + lane) * 16) : NO_RECORD;
#if !defined(PAIR_EXP_NORECSTORE)  // tuning experiment: what the record stores cost sweep 3
#pragma unroll
        for (int q = 0; q < pair_rec<WR>::Q; ++q) {
          const u32x4 d = {__float_as_uint(w[4 * q]), __float_as_uint(w[4 * q + 1]), __float_as_uint(w[4 * q + 2]), __float_as_uint(w[4 * q + 3])};
          __builtin_amdgcn_raw_buffer_store_b128(d, list_rs, (int)(ro + q * 1024), 0, 0);
        }
#else
        (void)ro; (void)list_rs;
#endif
        nrec += app ? 1 : 0;
      }
      dgdp = rdp; dgtr = rtr;
      lastdp = ldp; lasttr = ltr; lastcnt = run;
      if (i == L1 && t == tlast) {  // dafs.cpp:763; one lane of the group, once
        const int cl = L2 - j0;
        float sdp = 0.0f;
        int str = 1;
#pragma unroll
        for (int c = 0; c < WR; ++c)
          if (c == cl) { sdp = pdp[c]; str = ptr[c]; }
        simv = sdp / (float)str;
      }
      if (t == G - 1 && rowv && i >= 1) {  // row i is complete: its count has crossed the group
        rowacc += (uint32_t)run;
        s_rowptr[i] = rowacc;
      }
    };
    // Two steps per turn: each register set is refilled by the step that used it.  The sparse form rounds an odd step
    // count up instead of leaving the loop half way (one straight-line body, whose waits the compiler can count): in
    // step nsteps every lane's row lies beyond L1, so it finds no entry, appends nothing and writes no row pointer.
    // The dense form stores into the slab and must not run a step the slab does not have.
    const int nrun = dense ? nsteps : (nsteps + 1) & ~1;
    for (int s = 0; s < nrun; s += 2) {
      step(s, sva);
      if (dense && s + 1 >= nsteps) break;
      step(s + 1, svb);
    }
    nnz = rowacc;
    if (!dense && __any(ovf)) return false;  // wave-uniform: every pair of the wave takes the dense form
    slab_nrec = nrec;
  }
  nnz = __shfl(nnz, g * G + (G - 1));
  simv = __shfl(simv, g * G + tlast);

  // column prefix sums (row pointers of the transposed matrix)
  int colbase[WR];
  {
    int mine = 0;
#pragma unroll
    for (int c = 0; c < WR; ++c) mine += colcnt[c];
    int incl = mine;
#pragma unroll
    for (int o = 1; o < G; o <<= 1) {
      const int up = __shfl_up(incl, o, G);
      if (t >= o) incl += up;
    }
    int run = incl - mine;
#pragma unroll
    for (int c = 0; c < WR; ++c) { colbase[c] = run; run += colcnt[c]; }
  }

#if defined(PAIR_EXP_STOP) && PAIR_EXP_STOP == 3  // tuning experiment: everything up to sweep 3 (splits sweeps 3 and 4)
  if (simv != 12345.0f || nnz != 12345u || colbase[WR - 1] != 12345) return true;
#endif
  // reserve 2*nnz entries in the pool
  unsigned long long off = 0;
  if (t == 0 && act) off = atomicAdd(a.pool_top, 2ull * nnz);
  off = __shfl(off, g * G);
  const bool ok = act && (off + 2ull * nnz <= a.pool_cap);
  if (act && !ok && t == 0) atomicExch(a.status, DAFS_HIP_EOVERFLOW);
  const uint64_t rp = act ? a.rp_off[task] : 0;
  if (act && t == 0) {
    a.pair_off[task] = off;
    a.pair_nnz[task] = nnz;
    a.sim[task] = simv;
  }
  wave_lds_fence();
  // row pointers out (coalesced copy from LDS), transposed row pointers from registers
  if (act) {
    for (int r = t; r <= L1; r += G) a.rowptr_pool[rp + r] = s_rowptr[r];
    if (t == 0) a.rowptr_pool[rp + L1 + 1] = 0;
#pragma unroll
    for (int c = 0; c < WR; ++c) {
      const int j = j0 + c;
      if (j >= 1 && j <= L2) a.rowptr_pool[rp + L1 + 1 + j] = (uint32_t)(colbase[c] + colcnt[c]);
    }
  }

  // ------------------------------------------------------------------ sweep 4: emit CSR + transposed CSR
  if (!dense) {
    if (__any(ok)) {
      // A pair's pool region is one position space of 2 nnz slots, the row-CSR entries at [0, nnz) and the transposed
      // ones at [nnz, 2 nnz), the same position in ent_col and ent_val.  Both forms walk the lanes' lists K records at a
      // time (fetch: a lane beyond its n records reads outside the buffer).
      constexpr int Q = pair_rec<WR>::Q;
      constexpr int K = 4;  // records per turn, all arrived before the turn's first use (one wait per K records)
      int jm1 = j0 - 1;  // column numbers from one register: WR constants of the lane would be kept (spilled) kernel-wide
      asm volatile("" : "+v"(jm1));
      u32x4 cur[K][Q];
      auto fetch = [&](u32x4 (&r)[K][Q], const int k0, const int n) __attribute__((always_inline)) {
#pragma unroll
        for (int kk = 0; kk < K; ++kk) {
          const uint32_t ro = (k0 + kk < n) ? (uint32_t)(((uint32_t)(k0 + kk) * Q * 64 + lane) * 16) : NO_RECORD;
#pragma unroll
          for (int q = 0; q < Q; ++q) r[kk][q] = __builtin_amdgcn_raw_buffer_load_b128(list_rs, (int)(ro + q * 1024), 0, 0);
        }
#pragma unroll
        for (int kk = 0; kk < K; ++kk)
#pragma unroll
          for (int q = 0; q < Q; ++q) asm volatile("" : "+v"(r[kk][q]));
      };
      if constexpr (!staged) {
        // Scattered form: every entry is four 4-byte stores from its lane, behind a per-entry branch (the pool is
        // addressed with 64 bits).  The compiler cannot count stores behind branches, so all K records of a turn have
        // arrived before the turn's first store: one wait per K records.
        int maxrec = slab_nrec;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) maxrec = max(maxrec, __shfl_xor(maxrec, o));
        maxrec = __builtin_amdgcn_readfirstlane(maxrec);
        uint32_t colpos[WR];  // where the next entry of this lane's column c goes in the pair's transposed half
#pragma unroll
        for (int c = 0; c < WR; ++c) colpos[c] = nnz + (uint32_t)colbase[c];
        for (int k0 = 0; k0 < maxrec; k0 += K) {
          fetch(cur, k0, slab_nrec);
#pragma unroll
          for (int kk = 0; kk < K; ++kk) {
            uint32_t w[4 * Q];
#pragma unroll
            for (int q = 0; q < Q; ++q) { w[4 * q] = cur[kk][q].x; w[4 * q + 1] = cur[kk][q].y; w[4 * q + 2] = cur[kk][q].z; w[4 * q + 3] = cur[kk][q].w; }
            const uint32_t m = w[0];  // 0 beyond the lane's last record
            const int im1 = (int)w[1] & 0xFFFF;
            const uint32_t rowpos = s_rowptr[im1] + (uint32_t)((int)w[1] >> 16);  // the row's first entry of this lane
            int before = 0;  // entries of the record left of cell c
#pragma unroll
            for (int c = 0; c < WR; ++c) {
              const int e = (int)((m >> c) & 1u);
              if (e && ok) {
                const float p = __uint_as_float(w[2 + c]);
                const unsigned long long pos = off + rowpos + (uint32_t)before;
                a.ent_col[pos] = (uint32_t)(jm1 + c);
                a.ent_val[pos] = p;
                const unsigned long long tpos = off + colpos[c];
                a.ent_col[tpos] = (uint32_t)im1;
                a.ent_val[tpos] = p;
              }
              before += e;
              colpos[c] += (uint32_t)e;
            }
          }
        }
      } else {
        // Staged form: the region is produced window by window.  E consecutive positions are staged as {col, val} in the
        // group's own piece of LDS (`stage`) and then copied out with lane t writing positions t, t + G, ..., so that a
        // store instruction covers 4 G contiguous bytes per group instead of one scattered 4-byte request per lane.  The
        // window start w0 is the same for every group of the wave (each group counts in its own pair's positions); a
        // group whose pair has ended takes no part.  Every cell of a fetched record writes one slot, without a branch:
        // its position where it is an entry inside the window, and the lane's spare slot behind the window
        // (stage[E + t]) otherwise.  No workgroup barrier (the wavefronts of a workgroup take different numbers of
        // pairs): the stage is private to the wavefront, and DS operations of a wave execute in order.
        const uint32_t uE = (uint32_t)E;
        const uint32_t spare = uE + (uint32_t)t;
        const int nrec = ok ? slab_nrec : 0;
        const uint32_t npos = ok ? 2u * nnz : 0u;
        uint32_t maxpos = npos;
#pragma unroll
        for (int o = G; o < 64; o <<= 1) maxpos = max(maxpos, (uint32_t)__shfl_xor((int)maxpos, o));
        maxpos = __builtin_amdgcn_readfirstlane(maxpos);
        // this lane's columns occupy [tlo, thi) of the transposed half: lanes own ascending column ranges
        const uint32_t tlo = nnz + (uint32_t)colbase[0], thi = nnz + (uint32_t)(colbase[WR - 1] + colcnt[WR - 1]);
        int cursor = 0;  // row half: this lane's first record with an entry at or behind the window start
        for (uint32_t w0 = 0; w0 < maxpos; w0 += uE) {
          const uint32_t wend = w0 + uE;
          // Row half.  A lane's records are in row order, so their positions ascend: the lane resumes at its cursor and
          // stops at the first record that reaches beyond the window.  That record stays under the cursor (its entries
          // in front of the next window fall outside it then); the records wholly inside are passed.
          bool going = cursor < nrec;
          while (__any(going)) {
            fetch(cur, cursor, going ? nrec : 0);
            int adv = 0;
            bool stop = false;
#pragma unroll
            for (int kk = 0; kk < K; ++kk) {
              uint32_t w[4 * Q];
#pragma unroll
              for (int q = 0; q < Q; ++q) { w[4 * q] = cur[kk][q].x; w[4 * q + 1] = cur[kk][q].y; w[4 * q + 2] = cur[kk][q].z; w[4 * q + 3] = cur[kk][q].w; }
              const uint32_t m = w[0];  // 0 beyond the lane's last record
              const int im1 = (int)w[1] & 0xFFFF;
              const uint32_t rowpos = s_rowptr[im1] + (uint32_t)((int)w[1] >> 16);  // the row's first entry of this lane
              uint32_t before = 0;  // entries of the record left of cell c
#pragma unroll
              for (int c = 0; c < WR; ++c) {
                const uint32_t e = (m >> c) & 1u;
                const uint32_t rel = rowpos + before - w0;  // in front of the window: wraps to a large number
                stage[(e != 0 && rel < uE) ? rel : spare] = make_uint2((uint32_t)(jm1 + c), w[2 + c]);
                before += e;
              }
              const bool have = going && cursor + kk < nrec;  // by the index, so that every turn passes a record or stops
              const bool whole = have && rowpos + before <= wend;
              adv += whole ? 1 : 0;
              stop = stop || (have && !whole);
            }
            cursor += adv;
            going = going && !stop && cursor < nrec;
          }
          // Transposed half.  The window covers a contiguous range of columns, so only the lanes whose [tlo, thi) meets it
          // walk their lists; the others give the offset outside the buffer and cause no traffic.  A lane that takes
          // part walks its WHOLE list, so its running column positions start from the column bases in every window
          // it takes part in and have advanced past every earlier row when an entry of the window comes up.
          const bool part = nrec > 0 && wend > nnz && tlo < wend && thi > w0;
          int kmax = part ? nrec : 0;
#pragma unroll
          for (int o = 1; o < 64; o <<= 1) kmax = max(kmax, __shfl_xor(kmax, o));
          kmax = __builtin_amdgcn_readfirstlane(kmax);
          if (kmax > 0) {
            uint32_t colpos[WR];  // where the next entry of this lane's column c goes
#pragma unroll
            for (int c = 0; c < WR; ++c) colpos[c] = nnz + (uint32_t)colbase[c];
            for (int k0 = 0; k0 < kmax; k0 += K) {
              fetch(cur, k0, part ? nrec : 0);
#pragma unroll
              for (int kk = 0; kk < K; ++kk) {
                uint32_t w[4 * Q];
#pragma unroll
                for (int q = 0; q < Q; ++q) { w[4 * q] = cur[kk][q].x; w[4 * q + 1] = cur[kk][q].y; w[4 * q + 2] = cur[kk][q].z; w[4 * q + 3] = cur[kk][q].w; }
                const uint32_t m = w[0];
                const uint32_t im1 = w[1] & 0xFFFFu;
#pragma unroll
                for (int c = 0; c < WR; ++c) {
                  const uint32_t e = (m >> c) & 1u;
                  const uint32_t rel = colpos[c] - w0;
                  stage[(e != 0 && rel < uE) ? rel : spare] = make_uint2(im1, w[2 + c]);
                  colpos[c] += e;
                }
              }
            }
          }
          wave_lds_fence();
          // Copy out [w0, min(w0 + E, 2 nnz)): every position of that range has been written exactly once.
          const uint32_t n = min(uE, npos - min(npos, w0));  // 0 for a group whose pair has ended
          const uint32_t nmax = min(uE, maxpos - w0);
          uint32_t* __restrict__ out_col = a.ent_col + off + w0;
          float* __restrict__ out_val = a.ent_val + off + w0;
          // four runs per turn, their LDS reads together in front of the stores (a slot behind the window's end is read
          // from the first spare slot and not stored).  The lane number is taken afresh from one register here: hoisted
          // out of the loop over pairs, the lane's copy-out addresses would be kept, spilled, for the whole kernel.
          uint32_t tt = (uint32_t)t;
          asm volatile("" : "+v"(tt));
          for (uint32_t p0 = 0; p0 < nmax; p0 += 4 * G) {
            uint2 cv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) cv[u] = stage[min(p0 + (uint32_t)(u * G) + tt, uE)];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const uint32_t p = p0 + (uint32_t)(u * G) + tt;
              if (p < n) {
                out_col[p] = cv[u].x;
                out_val[p] = __uint_as_float(cv[u].y);
              }
            }
          }
          wave_lds_fence();  // the next window overwrites the stage
        }
      }
    }
  } else if (__any(ok)) {
    int colrun[WR];
#pragma unroll
    for (int c = 0; c < WR; ++c) colrun[c] = 0;
    int lastcnt = 0;
    int jm1 = j0 - 1;  // as in the sparse form
    asm volatile("" : "+v"(jm1));
    float pv[WR];
#pragma unroll
    for (int c = 0; c < WR; ++c) pv[c] = slab[c * 64 + lane];
    for (int s = 0; s < nsteps; ++s) {
      const int i = s - t;
      const bool rowv = (i >= 0) && (i <= L1);
      const float* slab_s = slab + (size_t)s * (W * 64);
      int run = shift_up1<G>(lastcnt, 0, t);
      const uint32_t rowbase = (rowv && i >= 1) ? s_rowptr[i - 1] : 0;
#pragma unroll
      for (int c = 0; c < WR; ++c) {
        const float p = pv[c];  // sweep 3 left 0 in every non-entry slot
        if (s + 1 < nsteps) pv[c] = slab_s[(W + c) * 64 + lane];
        const bool entry = p != 0.0f;
        if (entry && ok) {
          const unsigned long long pos = off + rowbase + (uint32_t)run;
          a.ent_col[pos] = (uint32_t)(jm1 + c);
          a.ent_val[pos] = p;
          const unsigned long long tpos = off + nnz + (uint32_t)(colbase[c] + colrun[c]);
          a.ent_col[tpos] = (uint32_t)(i - 1);
          a.ent_val[tpos] = p;
        }
        run += entry ? 1 : 0;
        colrun[c] += entry ? 1 : 0;
      }
      lastcnt = run;
    }
  }
  wave_lds_fence();
  return true;
}

// ---------------------------------------------------------------------------------------------
// host side: choice of the kernel instance for a batch
// ---------------------------------------------------------------------------------------------
struct pair_variant {
  int G, W;
  const void* fn;   // kernel entry (hipFuncGetAttributes / launch)
  int vgprs;        // registers per lane of the code object (0 until queried)
  int occ;          // wavefronts per SIMD the instance was compiled for (__launch_bounds__): stands in without a device
  int lds_static;   // bytes of static LDS of the code object (queried with vgprs)
  bool optin[16];   // lds_optin_once flags
};

// The row pointers of a launch live in LDS: per workgroup 4 wavefronts x 64/G groups x (max_len1 + 1) words, at most
// kPairRowptrLdsMax bytes.  The launches refuse more (DAFS_HIP_ETOOLONG) and pair_choose skips an instance that would
// need more, so first sequences reach 959 residues at G = 16, 1919 at G = 32 and 3839 at G = 64.
constexpr size_t kPairRowptrLdsMax = 60 * 1024;
inline size_t pair_rowptr_lds(int G, uint64_t rp_cap) { return (size_t)(4 * (64 / G) * rp_cap * sizeof(uint32_t)); }

// registers and static LDS from the code object, once per instance
inline void pair_query(pair_variant& v) {
  if (v.vgprs != 0) return;
  hipFuncAttributes at;
  if (hipFuncGetAttributes(&at, v.fn) == hipSuccess && at.numRegs > 0) {
    v.vgprs = at.numRegs;
    v.lds_static = (int)at.sharedSizeBytes;
  } else {
    (void)hipGetLastError();
    v.vgprs = 512 / v.occ / 8 * 8;
    v.lds_static = 4096;
  }
}

// waves per SIMD the register file allows (MI355X_MICROARCH.md, register files: 512 per lane per SIMD, granule 8)
inline int pair_occupancy(int vgprs) {
  const int alloc = (vgprs + 7) / 8 * 8;
  const int w = 512 / (alloc < 64 ? 64 : alloc);
  return w < 1 ? 1 : w;
}

// Sweep 4's staging window (pair_finish): E positions of 8 bytes per (wavefront, group), plus one spare slot per lane.
// E is what the LDS of a CU leaves when as many workgroups are resident as the registers allow: 160 KiB / workgroups
// per CU (one wavefront of a workgroup per SIMD, so that is the instance's wavefronts per SIMD), at most the 64 KiB a
// workgroup gets without opting in, minus the row pointers, the static tables, the spare slots and one allocation
// granule of slack, / (4 wavefronts x 64/G groups x 8 bytes), rounded down to a multiple of G: the window never costs
// a resident wavefront.  Where the row pointers leave less than one window of G positions, E = G and the launch opts
// in to the larger allocation.  DAFS_HIP_EMIT_WINDOW=<positions> (tests and tuning) forces a smaller E: rounded up to
// a multiple of G, capped by the derived one.  Returns the dynamic LDS of the launch in *lds_bytes.
inline uint32_t pair_emit_window(pair_variant& v, size_t rowptr_bytes, size_t* lds_bytes) {
  pair_query(v);
  const long per_wg = (160L * 1024) / pair_occupancy(v.vgprs);
  const long spare = 4L * 64 * 8;  // 4 wavefronts x (64/G groups x G lanes) x 8 bytes
  const long left = (per_wg < 64L * 1024 ? per_wg : 64L * 1024) - 1536 - (long)v.lds_static - (long)rowptr_bytes - spare;
  const long per_pos = 4L * (64 / v.G) * 8;
  long e = left > 0 ? left / per_pos / v.G * v.G : 0;
  if (e < v.G) e = v.G;
  const char* s = getenv("DAFS_HIP_EMIT_WINDOW");
  const long f = s ? atol(s) : 0;
  if (f > 0) {
    const long fr = (f + v.G - 1) / v.G * v.G;
    if (fr < e) e = fr;
  }
  *lds_bytes = rowptr_bytes + (size_t)(e * per_pos + spare);
  return (uint32_t)e;
}

// Picks (G, W) and the number of persistent wavefronts.  The model, fitted to runs of the ProbCons kernel on MI355X
// (profiles/r02_b_variants.txt): a wavefront executes (max_len1 + G) steps, each worth step_cost + cell_cost * (W - 1/2)
// ns of its SIMD's issue time (most waves of a batch run the W-1 instantiation); a SIMD that holds k wavefronts at
// once works at eff(k) = 0.5 / 0.75 / 1 of its issue rate for k = 1 / 2 / 3 or more (the sweeps wait on LDS lookups
// and on their slab); whole-wave groups spend whole_wave_factor of that per step (ProbCons 0.83: no seam, uniform
// pair bounds; CONTRAlign 1); and when the batch needs r > 1 rounds of resident wavefronts the rounds overlap each
// other's memory-bound and issue-bound sweeps (x 1 - round_overlap (1 - 1/r); ProbCons 0.17, CONTRAlign 0: its
// 1.8 us per cell and wavefront hold for every variant measured).  k comes from the code object's register count (hipFuncGetAttributes), not from a guess.
inline int pair_choose(pair_variant* vs, int nv, uint32_t ntasks, uint32_t max_len1, uint32_t max_len2, int planes,
                       double step_cost, double cell_cost, double whole_wave_factor, double round_overlap, dafs_pairhmm_plan* plan) {
  int cus = 256, dev = 0;
  if (hipGetDevice(&dev) == hipSuccess) {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) cus = v;
  } else {
    (void)hipGetLastError();
  }
  const char* e;
  const int force_g = (e = getenv("DAFS_HIP_FORCE_GROUP")) ? atoi(e) : 0;    // tests exercise every group size
  const int force_w = (e = getenv("DAFS_HIP_FORCE_WIDTH")) ? atoi(e) : 0;    // tuning
  const int cap_occ = (e = getenv("DAFS_HIP_WAVES_PER_SIMD")) ? atoi(e) : 0; // tuning: fewer resident wavefronts than the registers allow
  const pair_variant* best = nullptr;
  double best_cost = 0;
  int best_occ = 1;
  for (int k = 0; k < nv; ++k) {
    pair_variant& v = vs[k];
    if ((uint64_t)v.G * v.W < (uint64_t)max_len2 + 1) continue;
    if (force_g && v.G != force_g) continue;
    if (force_w && v.W != force_w) continue;
    if (pair_rowptr_lds(v.G, (uint64_t)max_len1 + 1) > kPairRowptrLdsMax) continue;  // the launch would refuse it
    pair_query(v);
    int occ = pair_occupancy(v.vgprs);
    if (cap_occ > 0 && occ > cap_occ) occ = cap_occ;
    const uint64_t waves = ((uint64_t)ntasks + (64 / v.G) - 1) / (64 / v.G);
    const double n = (double)waves / (4.0 * cus);  // wavefronts per SIMD over the whole batch
    const double kres = n < 1.0 ? 1.0 : (n < occ ? n : (double)occ);  // resident at once
    const double eff = kres < 1.5 ? 0.5 : (kres < 2.5 ? 0.75 : 1.0);
    const double step = (step_cost + cell_cost * (v.W - 0.5)) * (v.G == 64 ? whole_wave_factor : 1.0);
    const double rounds = n > occ ? n / occ : 1.0;
    const double cost = (double)(max_len1 + v.G) * step * (n < 1.0 ? 1.0 : n) / eff * (1.0 - round_overlap * (1.0 - 1.0 / rounds));
    if (!best || cost < best_cost) { best = &v; best_cost = cost; best_occ = occ; }
  }
  if (!best) return DAFS_HIP_ETOOLONG;
  const uint64_t waves = ((uint64_t)ntasks + (64 / best->G) - 1) / (64 / best->G);
  const uint64_t resident = (uint64_t)best_occ * 4 * cus;
  plan->group = best->G;
  plan->width = best->W;
  uint32_t nw = (uint32_t)(waves < resident ? waves : resident);
  nw = (nw + 3) & ~3u;  // whole workgroups of 4 waves
  plan->nwaves = nw;
  plan->slab_steps = max_len1 + best->G;
  plan->scratch_bytes = (uint64_t)nw * plan->slab_steps * best->W * 64 * sizeof(float) * planes;
  return DAFS_HIP_OK;
}

}  // namespace dafs
