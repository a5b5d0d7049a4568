// dafs_amd/csrc/capi_dd.cpp -- L1: the decoder plugins (Fold::Decoder / Align::Decoder,
// reference src/fold.h:47-60, src/align.h:57-65) and the fused per-node solver
// (DAFS::align_alignments + DAFS::solve_by_dd, reference src/dafs.cpp:896-981, 1006-1295).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "../../include/dafs_hip.h"
#include "call_frame.h"
#include "call_host.h"
#include "ctx.h"
#include "dd.h"
#include "hip_util.h"

using namespace dafs;

namespace {

// bump allocator over one device buffer (256-byte aligned pieces)
struct carver {
  uint8_t* base = nullptr;
  size_t used = 0;
  template <class T>
  T* take(size_t n) {
    used = (used + 255) & ~(size_t)255;
    T* p = base ? (T*)(base + used) : nullptr;
    used += n * sizeof(T);
    return p;
  }
};

struct region { size_t off, bytes; int value; };

void carve_nuss(carver& cv, uint32_t L, nuss_ws& w);
// What only the folding DPs touch -- their work arrays (16 L^2 bytes each), the HBM copies of the traceback codes and the
// pair scores in the order the DPs read them (the score copies of the node's plan, plan_node) -- goes into the node's SECOND
// block, which is carved when the consensus-pair count is known: a node that leaves its foldings out (dafs_dd_params::
// skip_uncoupled_folds and no consensus pair) gets none of it, a third of its memory instead of all (27 GB -> 9 GB at the
// 27 000-column root of c5-random).
void carve_folding(carver& cv, dd_node& nd, const dafs_dd_node_plan& pl) {
  const uint32_t sweep[2] = {pl.s_x, pl.s_y}, by_span[2] = {pl.s_xs, pl.s_ys};
  for (dd_fold& f : nd.f) { carve_nuss(cv, f.L, f.w); f.trk = f.w.tr; }  // the L*L uint32 tables double as bifurcation codes
  for (dd_fold& f : nd.f) f.trb = cv.take<uint8_t>((size_t)f.L * f.L / 2 + f.L + 16);
  for (int r = 0; r < 2; ++r) nd.f[r].s = sweep[r] ? cv.take<float>(((size_t)nd.f[r].L + 63) * dd_fold_cols(nd.f[r].L) * 64) : nullptr;
  for (int r = 0; r < 2; ++r) nd.f[r].s_span = by_span[r] ? cv.take<float>((size_t)nd.f[r].L * ((nd.f[r].L + 63) & ~63u) + 64) : nullptr;
}

void carve_nuss(carver& cv, uint32_t L, nuss_ws& w) {
  const size_t LL = (size_t)L * L;
  w.dp = cv.take<float>(LL + 1);
  w.tr = cv.take<uint32_t>(LL + 1);
  w.ck = cv.take<uint32_t>(LL + 2 * (size_t)L + 16);  // doubles as the traceback stack
  w.cv = cv.take<float>(LL + 1);
  w.cc = cv.take<uint32_t>((size_t)L + 1);
}

}  // namespace

extern "C" int dafs_hip_nussinov_decode(dafs_hip_ctx* c, float th, float w, uint32_t L, const float* p, const float* q,
                                        uint32_t* ss, float* score) {
  if (!c || !p || !ss || L == 0) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const size_t LL = (size_t)L * L;
  carver cv;
  for (int pass = 0; pass < 2; ++pass) {
    cv.used = 0;
    float* d_p = cv.take<float>(LL);
    float* d_q = q ? cv.take<float>(LL) : nullptr;
    nuss_ws ws;
    carve_nuss(cv, L, ws);
    uint32_t* d_ss = cv.take<uint32_t>(L);
    float* d_score = cv.take<float>(1);
    if (pass == 0) {
      int rc = c->work.reserve(cv.used + 256);
      if (rc) return rc;
      cv.base = c->work.ptr;
      continue;
    }
    if (hip_check(hipMemcpyAsync(d_p, p, LL * 4, hipMemcpyHostToDevice, c->stream))) return DAFS_HIP_ELAUNCH;
    if (q && hip_check(hipMemcpyAsync(d_q, q, LL * 4, hipMemcpyHostToDevice, c->stream))) return DAFS_HIP_ELAUNCH;
    int rc = nussinov_launch(L, d_p, d_q, w, th, ws, d_ss, d_score, c->stream);
    if (rc) return rc;
    if (hip_check(hipMemcpyAsync(ss, d_ss, (size_t)L * 4, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
    float s = 0;
    if (hip_check(hipMemcpyAsync(&s, d_score, 4, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
    if (hip_check(hipStreamSynchronize(c->stream))) return DAFS_HIP_ELAUNCH;
    if (score) *score = s;
  }
  return DAFS_HIP_OK;
}

static int nw_common(dafs_hip_ctx* c, float th, uint32_t L1, uint32_t L2, const float* p, const float* q, uint32_t* env,
                     int compute_env, int decode, uint32_t* al, float* score) {
  if (!c || !p || !env || L1 == 0 || L2 == 0) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const size_t C = (size_t)L1 * L2, T = (size_t)(L1 + 1) * (L2 + 1);
  carver cv;
  for (int pass = 0; pass < 2; ++pass) {
    cv.used = 0;
    float* d_p = cv.take<float>(C);
    float* d_q = q ? cv.take<float>(C) : nullptr;
    float* d_dp = cv.take<float>(T + L1 + 2);
    uint8_t* d_tr = cv.take<uint8_t>(T);
    uint32_t* d_env = cv.take<uint32_t>(2 * ((size_t)L1 + 1));
    uint32_t* d_al = cv.take<uint32_t>((size_t)L1 + 2);
    float* d_score = cv.take<float>(1);
    if (pass == 0) {
      int rc = c->work.reserve(cv.used + 256);
      if (rc) return rc;
      cv.base = c->work.ptr;
      continue;
    }
    if (hip_check(hipMemcpyAsync(d_p, p, C * 4, hipMemcpyHostToDevice, c->stream))) return DAFS_HIP_ELAUNCH;
    if (q && hip_check(hipMemcpyAsync(d_q, q, C * 4, hipMemcpyHostToDevice, c->stream))) return DAFS_HIP_ELAUNCH;
    if (!compute_env && hip_check(hipMemcpyAsync(d_env, env, 2 * ((size_t)L1 + 1) * 4, hipMemcpyHostToDevice, c->stream))) return DAFS_HIP_ELAUNCH;
    int rc = nw_launch(L1, L2, d_p, d_q, th, d_env, compute_env, d_dp, d_tr, d_al, d_score, c->stream);
    if (rc) return rc;
    if (compute_env && hip_check(hipMemcpyAsync(env, d_env, 2 * ((size_t)L1 + 1) * 4, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
    float s = 0;
    if (decode) {
      if (hip_check(hipMemcpyAsync(al, d_al, (size_t)L1 * 4, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
      if (hip_check(hipMemcpyAsync(&s, d_score, 4, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
    }
    if (hip_check(hipStreamSynchronize(c->stream))) return DAFS_HIP_ELAUNCH;
    if (decode && score) *score = s;
  }
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_nw_envelope(dafs_hip_ctx* c, float th, uint32_t L1, uint32_t L2, const float* p, uint32_t* env) {
  return nw_common(c, th, L1, L2, p, nullptr, env, 1, 0, nullptr, nullptr);
}

extern "C" int dafs_hip_nw_decode(dafs_hip_ctx* c, float th, uint32_t L1, uint32_t L2, const float* p, const float* q,
                                  const uint32_t* env, uint32_t* al, float* score) {
  if (!al) return DAFS_HIP_EINVAL;
  return nw_common(c, th, L1, L2, p, q, (uint32_t*)env, 0, 1, al, score);
}

// The dense decoder classes (reference Nussinov, src/nussinov.cpp:32-204, and NeedlemanWunsch,
// src/needleman_wunsch.cpp:28-196; DAFS itself instantiates the sparse ones, src/dafs.cpp:1692,1759).
extern "C" int dafs_hip_nussinov_decode_dense(dafs_hip_ctx* c, float th, float w, uint32_t L, const float* p, const float* q,
                                              uint32_t* ss, float* score) {
  if (!c || !p || !ss || L == 0) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const size_t LL = (size_t)L * L;
  carver cv;
  for (int pass = 0; pass < 2; ++pass) {
    cv.used = 0;
    float* d_p = cv.take<float>(LL);
    float* d_q = q ? cv.take<float>(LL) : nullptr;
    float* d_dp = cv.take<float>(LL + 1);
    uint32_t* d_tr = cv.take<uint32_t>(LL + 1);
    uint32_t* d_stack = cv.take<uint32_t>(4 * ((size_t)L + 4));
    uint32_t* d_ss = cv.take<uint32_t>(L);
    float* d_score = cv.take<float>(1);
    if (pass == 0) {
      int rc = c->work.reserve(cv.used + 256);
      if (rc) return rc;
      cv.base = c->work.ptr;
      continue;
    }
    if (hip_check(hipMemcpyAsync(d_p, p, LL * 4, hipMemcpyHostToDevice, c->stream))) return DAFS_HIP_ELAUNCH;
    if (q && hip_check(hipMemcpyAsync(d_q, q, LL * 4, hipMemcpyHostToDevice, c->stream))) return DAFS_HIP_ELAUNCH;
    int rc = nussinov_dense_launch(L, d_p, d_q, w, th, d_dp, d_tr, d_stack, d_ss, d_score, c->stream);
    if (rc) return rc;
    if (hip_check(hipMemcpyAsync(ss, d_ss, (size_t)L * 4, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
    float s = 0;
    if (hip_check(hipMemcpyAsync(&s, d_score, 4, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
    if (hip_check(hipStreamSynchronize(c->stream))) return DAFS_HIP_ELAUNCH;
    if (score) *score = s;
  }
  return DAFS_HIP_OK;
}

// NeedlemanWunsch::decode = the sparse decoder's DP with every cell inside the envelope
extern "C" int dafs_hip_nw_decode_dense(dafs_hip_ctx* c, float th, uint32_t L1, uint32_t L2, const float* p, const float* q,
                                        uint32_t* al, float* score) {
  if (!al || !L1 || !L2) return DAFS_HIP_EINVAL;
  std::vector<uint32_t> env(2 * ((size_t)L1 + 1));
  for (uint32_t i = 0; i <= L1; ++i) { env[2 * i] = i ? 1u : 0u; env[2 * i + 1] = L2; }
  return nw_common(c, th, L1, L2, p, q, env.data(), 0, 1, al, score);
}

// ---------------------------------------------------------------------------------------------
// per-node solver
// ---------------------------------------------------------------------------------------------
namespace {

struct geom {  // host-side geometry of one child alignment
  std::vector<uint32_t> rank, idx, idxoff;
};

int make_geom(const dafs_hip_ctx* c, uint32_t n, uint32_t L, const uint32_t* seq, const uint8_t* mask, geom& g) {
  g.rank.assign((size_t)n * L, DAFS_HIP_NONE);
  g.idxoff.resize(n);
  g.idx.clear();
  for (uint32_t r = 0; r < n; ++r) {
    if (seq[r] >= c->len.size()) return DAFS_HIP_EINVAL;
    g.idxoff[r] = (uint32_t)g.idx.size();
    uint32_t k = 0;
    for (uint32_t i = 0; i < L; ++i)
      if (mask[(size_t)r * L + i]) { g.rank[(size_t)r * L + i] = k++; g.idx.push_back(i); }
    if (k != c->len[seq[r]]) return DAFS_HIP_EINVAL;  // the mask must place every residue
  }
  return DAFS_HIP_OK;
}

}  // namespace

extern "C" void dafs_hip_dd_default_params(dafs_dd_params* p) {
  if (!p) return;
  p->w = 4.0f; p->eta0 = 0.5f; p->th_a = 0.01f; p->th_s = 0.2f; p->t_max = 600; p->force_iters = 0; p->skip_uncoupled_folds = 0;  // dafs.cpp:1612-1640
}

namespace {

// The solver's environment switches (tests and tuning aids), read once per call that opens or advances nodes (tests change
// them between calls).  DAFS_HIP_DD_WIDE=1: every node takes the forms of alignments too wide for the on-chip placements
// (foldings span-ordered on HBM tables without sweep-order copies, the alignment DP in panels of 64 columns with its codes in
// HBM slots, row pointers searched in HBM, one averaging row per workgroup).  DAFS_HIP_DD_NWG: no alignment codes in LDS.
// DAFS_HIP_DD_WG=2: every folder takes the workgroup form, whatever its width.  The others turn a form or a placement off.
struct dd_switches { bool wide, span, nwg, wg, wg_force, span_mw, split, avg_coop, stamps, lose_folders; };

dd_switches read_switches() {
  auto val = [](const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; };
  const int wg = val("DAFS_HIP_DD_WG", 1);
  return {val("DAFS_HIP_DD_WIDE", 0) != 0, val("DAFS_HIP_DD_SPAN", 1) != 0, getenv("DAFS_HIP_DD_NWG") != nullptr, wg != 0, wg == 2,
          val("DAFS_HIP_DD_SPAN_MW", 1) != 0, val("DAFS_HIP_DD_SPLIT", 1) != 0, getenv("DAFS_HIP_AVG_COOP0") == nullptr,
          getenv("DAFS_HIP_DD_STAMPS") != nullptr, getenv("DAFS_HIP_DD_LOSE_FOLDERS") != nullptr};
}

dd_params device_params(const dafs_dd_params* prm, const dd_switches& sw) {
  dd_params dp;
  dp.w = prm->w; dp.eta0 = prm->eta0; dp.th_a = prm->th_a; dp.th_s = prm->th_s; dp.t_max = prm->t_max; dp.force_iters = prm->force_iters;
  dp.stamps = sw.stamps; dp.debug_lose_folders = sw.lose_folders; dp.span_one_wave = !sw.span_mw;
  dp.skip_xy = prm->skip_uncoupled_folds ? 1 : 0;
  dp.slice = 0;
  dp.budget = 0; dp.t_ref = nullptr; dp.t_ref_write = 0;
  return dp;
}

// The one place that chooses a node's forms, their LDS bytes (by the kernels' layout, dd_node_lds / dd_folder_lds)
// and the score copies they read.  Foldings without a form here run span-ordered on HBM tables and need no LDS.
dafs_dd_node_plan plan_node(uint32_t L1, uint32_t L2, const dd_switches& sw) {
  dafs_dd_node_plan p = {};
  p.nw_w = sw.wide ? 1u : dd_nw_cols(L2);  // columns per lane of the alignment DP
  auto bytes = [&](uint32_t flags) { return (size_t)dd_node_lds(L1, L2, flags).end * 4; };
  auto folder_bytes = [](uint32_t L, uint32_t form, uint32_t K) { return (size_t)dd_folder_lds(L, form, K).end * 4; };
  auto reg = [](uint32_t L, uint32_t cols) { return dd_fold_cols(L) <= cols; };  // a register form exists for this width
  const bool span_fits = sw.span && L1 <= DD_SPAN_LMAX && L2 <= DD_SPAN_LMAX;
  uint32_t f = 0;
  // the node's workgroup: both span forms (up to ~170 + 170 columns, with the alignment codes on chip too), else both register
  // forms, else one region for x then y, else the same with the codes in HBM; the alignment codes where it runs in one panel
  if (sw.wide) {}
  else if (span_fits && bytes(kLdsSpanXY | kLdsNwTab) <= kDdLdsBudget) f = kLdsSpanXY;
  else if (bytes(kLdsFastX | kLdsFastY) <= kDdLdsBudget) f = kLdsFastX | kLdsFastY;
  else if (reg(L1, DD_WREG) && reg(L2, DD_WREG) && bytes(kLdsShared) <= kDdLdsBudget) f = kLdsShared;
  else if (reg(L1, DD_WFOLD) && reg(L2, DD_WFOLD) && bytes(kLdsShared | kLdsSharedHbm) <= kDdLdsBudget) f = kLdsShared | kLdsSharedHbm;
  if (!sw.wide && !sw.nwg && p.nw_w <= DD_WNW && L2 < 64u * p.nw_w && bytes(f | kLdsNwTab) <= kDdLdsBudget) f |= kLdsNwTab;
  p.lds_flags = f; p.lds = (uint32_t)bytes(f);
  // split plan: each folding on a workgroup of its own, the leader keeping the alignment DP (within p.lds).  Worth it when the
  // two do not run side by side; when their span forms fit a folder but not the node; when the span forms run side by side
  // but have more than one row slot, which a folder shares out to its wavefronts (nuss_span_mw); or without a register form.
  const uint32_t Lm = std::max(L1, L2), Ls[2] = {L1, L2};
  const bool span_folders = span_fits && !sw.wide && folder_bytes(Lm, kFoldSpan, 0) <= kDdLdsBudget &&
                            (!(f & kLdsSpanXY) || (sw.span_mw && Lm > 64));
  if ((!(f & (kLdsFastX | kLdsSpanXY)) || span_folders || sw.wg_force) && !sw.wide) {
    size_t worst = 0;
    for (uint32_t r = 0; r < 2; ++r) {
      const uint32_t L = Ls[r];
      const bool no_reg = !reg(L, DD_WFOLD) || sw.wg_force;
      uint32_t form = 0, K = 0;
      if (span_folders && !sw.wg_force) form = kFoldSpan;
      else if (!no_reg && reg(L, DD_WREG) && folder_bytes(L, kFoldReg, 0) <= kDdLdsBudget) form = kFoldReg;
      else if (!no_reg && folder_bytes(L, kFoldRegHbm, 0) <= kDdLdsBudget) form = kFoldRegHbm;
      else if (no_reg && sw.wg)  // as many candidates per column on chip as fit; beyond ~10 000 columns not even the rolling rows do
        for (uint32_t k : {4u, 2u, 0u})
          if (folder_bytes(L, kFoldWg, k) <= kDdLdsBudget) { form = kFoldWg; K = k; break; }
      p.fold_fast |= dd_fold_bits(r, form, K);
      worst = std::max(worst, folder_bytes(L, form, K));
    }
    if (p.fold_fast || !reg(L1, DD_WFOLD) || !reg(L2, DD_WFOLD)) p.split_lds = (uint32_t)std::max(worst, (size_t)p.lds);
  }
  // the score copies these forms read: sweep order for the register forms, by span for the span and workgroup forms
  const bool span_any = (f & kLdsSpanXY) || ((dd_fold_form(p.fold_fast, 0) | dd_fold_form(p.fold_fast, 1)) & kFoldSpan);
  uint32_t *sweep[2] = {&p.s_x, &p.s_y}, *by_span[2] = {&p.s_xs, &p.s_ys};
  for (uint32_t r = 0; r < 2; ++r) {
    *sweep[r] = reg(Ls[r], DD_WFOLD) && !sw.wide && !(f & kLdsSpanXY);
    *by_span[r] = span_any || (dd_fold_form(p.fold_fast, r) & kFoldWg);
  }
  return p;
}

// Builds nnodes resident nodes (appended to c->dd_open): geometry upload, profile averages, sparse lists and
// consensus constraints (DAFS::align_alignments up to the solve_by_dd call, dafs.cpp:896-960).
// A lane = a stream with the node-descriptor and per-node-word buffers its launches use.  Lane 0 is the context's main
// stream; dafs_hip_nodes_round sets up and starts new nodes on lane 1 while the open ones advance on lane 0.
struct dd_lane { hipStream_t st; dev_buf<dd_node>* d_nodes; dev_buf<uint32_t>* d_paused; int id; };
dd_lane lane_of(dafs_hip_ctx* c, int k) { return k == 0 ? dd_lane{c->stream, &c->d_nodes, &c->d_paused, 0} : dd_lane{c->node_stream, &c->d_nodes2, &c->d_paused2, 1}; }

// What a node's launch would read, checked on the host before anything is enqueued.  Every form of the folding DPs
// reads one of the two score copies (dd_fold::s in sweep order for the column-owning register forms, dd_fold::s_span by span
// for the span form), and nodes_open leaves out the copies no form of the node can use.  A plan that selects a form
// whose copy is absent would make the kernel use a null base + cell offset as an address: that was the memory-access
// fault of round 2 ("the fault at 16 x ~1100 columns": the multiplier updates wrote f[0].s[skew(i, j)] of
// nodes beyond 1024 columns, whose sweep-order copy had just become optional).  The kernel's writes are guarded now; this check
// turns any future mismatch between the carving and the form selection into DAFS_HIP_ELAUNCH instead of a fault.
// folds: this launch runs the node's folding DPs (the kernel's fold_on: not (skip_uncoupled_folds and no consensus pair))
int plan_check(const dd_node& nd, bool split, bool folds) {
  auto bad = [](const char* what) {
    fprintf(stderr, "dafs_hip: node plan refused: %s\n", what);
    return DAFS_HIP_ELAUNCH;
  };
  auto any_null = [](std::initializer_list<const void*> arrays) { return std::find(arrays.begin(), arrays.end(), nullptr) != arrays.end(); };
  if (any_null({nd.p_z, nd.q_z, nd.nw_edge, nd.tr_z, nd.pz_s, nd.qz_s, nd.env, nd.env4, nd.zmap, nd.pz_ptr, nd.pz_k, nd.cz_ptr, nd.cz_k, nd.cz_flag, nd.cbp_cnt,
                nd.cbp, nd.sw, nd.tz, nd.z, nd.score, nd.info, nd.fstate, nd.sync}))
    return bad("a null array in the node descriptor");
  for (const dd_fold& f : nd.f) {
    if (any_null({f.seq, f.rank, f.idx, f.idxoff, f.p, f.q, f.map, f.ptr, f.col, f.cflag, f.tc, f.ss})) return bad("a null array in the node descriptor");
    if (!f.L || !f.n) return bad("empty child alignment");
  }
  if (!folds) return DAFS_HIP_OK;  // nothing below is touched
  for (const dd_fold& f : nd.f)
    if (any_null({f.w.dp, f.w.tr, f.w.ck, f.w.cv, f.w.cc, f.trb, f.trk}))
      return bad("a node that folds without its folding arrays (opened with skip_uncoupled_folds, advanced without?)");
  if (split && (nd.lds_flags & ~kLdsNwTab)) return bad("a split leader keeps the alignment DP only");
  const bool span = !split && (nd.lds_flags & kLdsSpanXY) != 0;
  static_assert(kLdsFastY == kLdsFastX << 1, "the register-form flag of folding r is kLdsFastX << r");
  for (uint32_t r = 0; r < 2; ++r) {
    const dd_fold& f = nd.f[r];
    const bool reg = dd_fold_cols(f.L) <= DD_WFOLD;
    if (!split) {
      if (span && !f.s_span) return bad("span form without the by-span score copies");
      if (span && f.L > DD_SPAN_LMAX) return bad("span form beyond its width");
      if (!span && (nd.lds_flags & ((kLdsFastX << r) | kLdsShared)) && reg && !f.s) return bad("register form of a folding without its sweep-order scores");
    } else {
      const uint32_t form = dd_fold_form(nd.fold_fast, r);
      if (form & kFoldSpan) {
        if (!f.s_span) return bad("span-form folder without the by-span score copy");
        if (f.L > DD_SPAN_LMAX) return bad("span-form folder beyond its width");
      } else if ((form & (kFoldReg | kFoldRegHbm)) && reg && !f.s) return bad("register-form folder without its sweep-order scores");
      if ((form & kFoldWg) && !f.s_span) return bad("workgroup-form folder without the by-span score copy");
    }
  }
  return DAFS_HIP_OK;
}

struct open_blocks {  // device blocks of the nodes an open call has carved so far (given back when the call fails)
  std::vector<uint8_t*> blk0, blk1;
  std::vector<size_t> bytes0, bytes1;
};

// DAFS_HIP_DD_FAIL_OPEN=k (tests): nodes_open fails with DAFS_HIP_ELAUNCH at its k-th stage (1 after the blocks and their
// fills are queued, 2 after the lists, 3 after the second blocks, 4 after everything) -- the late-failure path
bool fail_injected(int stage) {
  const char* e = getenv("DAFS_HIP_DD_FAIL_OPEN");
  return e && atoi(e) == stage;
}

int nodes_open_impl(dafs_hip_ctx* c, const dd_lane& ln, uint32_t nnodes, const dafs_node_input* in, const dd_params& dp, const dd_switches& sw,
                    open_blocks& ob) {
  const mp_store& mps = c->mp[c->cur_mp];
  const bp_store& bps = c->bp[c->cur_bp];
  if (!mps.valid || !bps.valid || mps.n_tasks != c->fam.npairs()) return DAFS_HIP_EINVAL;

  // ---- host geometry ----
  std::vector<geom> g1(nnodes), g2(nnodes);
  for (uint32_t b = 0; b < nnodes; ++b) {
    const dafs_node_input& ni = in[b];
    if (!ni.n1 || !ni.n2 || !ni.len1 || !ni.len2 || !ni.seq1 || !ni.seq2 || !ni.mask1 || !ni.mask2) return DAFS_HIP_EINVAL;
    int rc;
    if ((rc = make_geom(c, ni.n1, ni.len1, ni.seq1, ni.mask1, g1[b]))) return rc;
    if ((rc = make_geom(c, ni.n2, ni.len2, ni.seq2, ni.mask2, g2[b]))) return rc;
    // only pairs within a family exist (dafs_hip_set_families): every row of a node must come from one family
    const uint32_t s0 = ni.seq1[0];
    for (uint32_t r = 0; r < ni.n1; ++r) if (!c->fam.same_family(s0, ni.seq1[r])) return DAFS_HIP_EINVAL;
    for (uint32_t r = 0; r < ni.n2; ++r) if (!c->fam.same_family(s0, ni.seq2[r])) return DAFS_HIP_EINVAL;
  }

  // ---- carve each node's block (two passes: size, then pointers) ----
  std::vector<dd_node> nodes(nnodes);
  std::vector<std::vector<uint8_t>> heads(nnodes);  // upload staging, alive until the first synchronisation below
  std::vector<dafs_dd_node_plan> plans(nnodes);
  ob.blk0.assign(nnodes, nullptr); ob.blk1.assign(nnodes, nullptr);
  ob.bytes0.assign(nnodes, 0); ob.bytes1.assign(nnodes, 0);
  std::vector<uint8_t*>&blk0 = ob.blk0, &blk1 = ob.blk1;
  std::vector<size_t>&blk0_bytes = ob.bytes0, &blk1_bytes = ob.bytes1;
  for (uint32_t b = 0; b < nnodes; ++b) {
    const dafs_node_input& ni = in[b];
    dd_node& nd = nodes[b];
    carver cv;
    std::vector<region> fills;
    const dafs_dd_node_plan& pl = plans[b] = plan_node(ni.len1, ni.len2, sw);
    const geom* g[2] = {&g1[b], &g2[b]};
    for (int pass = 0; pass < 2; ++pass) {
      cv.used = 0;
      fills.clear();
      memset(&nd, 0, sizeof nd);
      const uint32_t L1 = ni.len1, L2 = ni.len2;
      nd.f[0].n = ni.n1; nd.f[1].n = ni.n2; nd.f[0].L = L1; nd.f[1].L = L2;
      const size_t ZZ = (size_t)L1 * L2;
      auto LL = [](const dd_fold& f) { return (size_t)f.L * f.L; };
      for (dd_fold& f : nd.f) f.seq = cv.take<uint32_t>(f.n);
      for (dd_fold& f : nd.f) f.rank = cv.take<uint32_t>((size_t)f.n * f.L);
      for (int r = 0; r < 2; ++r) nd.f[r].idx = cv.take<uint32_t>(g[r]->idx.size() + 1);
      for (dd_fold& f : nd.f) f.idxoff = cv.take<uint32_t>(f.n);
      // zero-filled block: posteriors, multipliers, flags
      const size_t z0 = (cv.used + 255) & ~(size_t)255;
      for (dd_fold& f : nd.f) f.p = cv.take<float>(LL(f));
      nd.p_z = cv.take<float>(ZZ);
      for (dd_fold& f : nd.f) f.q = cv.take<float>(LL(f));
      nd.q_z = cv.take<float>(ZZ);
      nd.cz_flag = cv.take<uint8_t>(ZZ);
      for (dd_fold& f : nd.f) f.cflag = cv.take<uint8_t>(LL(f) / 2 + 2);
      nd.sync = cv.take<uint32_t>(8);
      fills.push_back({z0, cv.used - z0, 0});
      // -1-filled block: dense id maps
      const size_t m0 = (cv.used + 255) & ~(size_t)255;
      for (dd_fold& f : nd.f) f.map = cv.take<int32_t>(LL(f));
      nd.zmap = cv.take<int32_t>(ZZ);
      fills.push_back({m0, cv.used - m0, 0xFF});
      // (the folding DPs' work arrays, codes and score copies are carved into the node's second block, once the
      // consensus-pair count says whether this node folds at all: carve_folding below)
      // the alignment DP: columns per lane, and with them the panels of second alignments beyond 64 nw_w - 1 columns
      nd.nw_w = pl.nw_w; nd.lds_flags = pl.lds_flags; nd.fold_fast = pl.fold_fast;
      const size_t nw_panels = dd_nw_panels(L2, nd.nw_w);
      nd.nw_edge = cv.take<float>(2 * ((size_t)L1 + 2));
      nd.tr_z = cv.take<uint8_t>(nw_panels * (L1 + 1) * 512);  // a 64-bit slot per (panel, row, lane)
      // sweep-order inputs of the alignment DP: steps x columns per lane x 64 lanes, panel by panel
      nd.pz_s = cv.take<float>(nw_panels * ((size_t)L1 + 63) * nd.nw_w * 64); nd.qz_s = cv.take<float>(nw_panels * ((size_t)L1 + 63) * nd.nw_w * 64);
      nd.env = cv.take<uint32_t>(2 * ((size_t)L1 + 1));
      nd.env4 = cv.take<uint32_t>(2 * ((size_t)L1 + 130));
      for (dd_fold& f : nd.f) { f.ptr = cv.take<uint32_t>((size_t)f.L + 2); f.col = cv.take<uint32_t>(LL(f) / 2 + 2); }
      nd.pz_ptr = cv.take<uint32_t>((size_t)L1 + 2); nd.pz_k = cv.take<uint32_t>(ZZ + 1);
      nd.cz_ptr = cv.take<uint32_t>((size_t)L1 + 2); nd.cz_k = cv.take<uint32_t>(ZZ + 1);
      nd.cbp_cnt = cv.take<uint32_t>(LL(nd.f[0]) / 2 + 2);
      for (dd_fold& f : nd.f) f.tc = cv.take<int32_t>(LL(f) / 2 + 2);
      nd.tz = cv.take<int32_t>(ZZ + 1);
      for (dd_fold& f : nd.f) f.ss = cv.take<uint32_t>((size_t)f.L + 2);
      nd.z = cv.take<uint32_t>((size_t)L1 + 2);
      nd.score = cv.take<float>(1); nd.info = cv.take<uint32_t>(16); nd.fstate = cv.take<float>(4);
      if (pass == 0) {
        cv.base = c->dd_alloc(cv.used + 256);
        if (!cv.base) return DAFS_HIP_ENOMEM;
        blk0[b] = cv.base; blk0_bytes[b] = cv.used + 256;
      }
    }
    for (const region& r : fills)
      if (hip_check(hipMemsetAsync(cv.base + r.off, r.value, r.bytes, ln.st))) return DAFS_HIP_ELAUNCH;
    // the geometry arrays were carved first and back to back: one upload of the head of the block brings them all
    {
      const size_t head = (size_t)((const uint8_t*)(nd.f[1].idxoff + ni.n2) - cv.base);
      std::vector<uint8_t>& blob = heads[b];
      blob.assign(head, 0);
      auto put = [&](const void* dst, const void* src, size_t bytes) {
        if (bytes) memcpy(blob.data() + ((const uint8_t*)dst - cv.base), src, bytes);
      };
      const uint32_t* seqs[2] = {ni.seq1, ni.seq2};
      for (int r = 0; r < 2; ++r) {
        const dd_fold& f = nd.f[r];
        put(f.seq, seqs[r], (size_t)f.n * 4);
        put(f.rank, g[r]->rank.data(), g[r]->rank.size() * 4);
        put(f.idx, g[r]->idx.data(), g[r]->idx.size() * 4);
        put(f.idxoff, g[r]->idxoff.data(), (size_t)f.n * 4);
      }
      if (hip_check(hipMemcpyAsync(cv.base, blob.data(), head, hipMemcpyHostToDevice, ln.st))) return DAFS_HIP_ELAUNCH;
    }
  }
  int rc;
  if (fail_injected(1)) return DAFS_HIP_ELAUNCH;
  if ((rc = ln.d_nodes->upload(nodes.data(), nnodes, ln.st))) return rc;  // synchronises: host vectors stay valid until here
  const mp_store_dev mpv = c->mp_view(mps);
  const bp_store_dev bpv = bps.view();
  uint32_t max_len = 0;
  for (uint32_t b = 0; b < nnodes; ++b) max_len = std::max(max_len, std::max(in[b].len1, in[b].len2));
  // few nodes with hundreds of source rows per row of p_z (the top of the guide tree): a workgroup per p_z row
  uint64_t srcs = 0;
  for (uint32_t b = 0; b < nnodes; ++b) srcs = std::max<uint64_t>(srcs, (uint64_t)in[b].n1 * in[b].n2);
  const int coop = (nnodes <= 4 && srcs >= 512 && sw.avg_coop) ? 1 : 0;
  if ((rc = dd_avg_launch(ln.d_nodes->ptr, nnodes, max_len, mpv, bpv, sw.wide ? 1 : 0, coop, ln.st))) return rc;
  for (uint32_t b = 0; b < nnodes; ++b) {  // base-pairing matrices supplied by the caller (--bp-update) replace the averages
    const size_t XX = (size_t)in[b].len1 * in[b].len1, YY = (size_t)in[b].len2 * in[b].len2;
    if (in[b].p_x && hip_check(hipMemcpyAsync(nodes[b].f[0].p, in[b].p_x, XX * 4, hipMemcpyHostToDevice, ln.st))) return DAFS_HIP_ELAUNCH;
    if (in[b].p_y && hip_check(hipMemcpyAsync(nodes[b].f[1].p, in[b].p_y, YY * 4, hipMemcpyHostToDevice, ln.st))) return DAFS_HIP_ELAUNCH;
  }
  if ((rc = ln.d_paused->reserve(nnodes))) return rc;  // doubles as the landing place of the per-node counts
  if ((rc = dd_lists_launch(ln.d_nodes->ptr, nnodes, sw.wide ? 0 : max_len, dp, ln.d_paused->ptr, ln.st))) return rc;
  // ---- consensus base-pair counts -> each node's second block ----
  std::vector<uint32_t> counts(nnodes);
  if (hip_check(hipMemcpyAsync(counts.data(), ln.d_paused->ptr, (size_t)nnodes * 4, hipMemcpyDeviceToHost, ln.st))) return DAFS_HIP_ELAUNCH;
  if (hip_check(hipStreamSynchronize(ln.st))) return DAFS_HIP_ELAUNCH;
  if (fail_injected(2)) return DAFS_HIP_ELAUNCH;
  for (uint32_t b = 0; b < nnodes; ++b) {
    const uint32_t ncbp = counts[b];
    carver cb;
    for (int pass = 0; pass < 2; ++pass) {
      cb.used = 0;
      nodes[b].ncbp_cap = ncbp;
      nodes[b].cbp = cb.take<uint32_t>((size_t)8 * ncbp + 8);
      nodes[b].sw = cb.take<float>((size_t)ncbp + 1);
      if (!(dp.skip_xy && ncbp == 0)) carve_folding(cb, nodes[b], plans[b]);  // the kernel's fold_on
      if (pass == 0) {
        cb.base = c->dd_alloc(cb.used + 256);
        if (!cb.base) return DAFS_HIP_ENOMEM;
        blk1[b] = cb.base; blk1_bytes[b] = cb.used + 256;
      }
    }
  }
  if (fail_injected(3)) return DAFS_HIP_ELAUNCH;
  for (uint32_t b = 0; b < nnodes; ++b)  // both placements a launch may choose for this node, before anything runs on it
    if ((rc = plan_check(nodes[b], false, !(dp.skip_xy && counts[b] == 0)))) return rc;
  if ((rc = ln.d_nodes->upload(nodes.data(), nnodes, ln.st))) return rc;
  if ((rc = dd_cbp_fill_launch(ln.d_nodes->ptr, nnodes, sw.wide ? 0 : max_len, dp, ln.st))) return rc;
  if (fail_injected(4)) return DAFS_HIP_ELAUNCH;
  for (uint32_t b = 0; b < nnodes; ++b) {
    dafs_hip_ctx::dd_open_node on;
    on.nd = nodes[b]; on.lds = plans[b].lds; on.split_lds = plans[b].split_lds;
    on.blk[0] = blk0[b]; on.blk[1] = blk1[b]; on.blk_bytes[0] = blk0_bytes[b]; on.blk_bytes[1] = blk1_bytes[b];
    c->dd_open.push_back(on);
  }
  return DAFS_HIP_OK;
}

// A failed open leaves nothing behind: the fills, uploads and set-up kernels it has queued on the lane's stream may still
// write into the blocks it carved, so the stream is drained before they go back to the free list (the next dd_alloc,
// possibly for the other lane, may hand them out at once), and the nodes it may have appended are dropped.
int nodes_open(dafs_hip_ctx* c, const dd_lane& ln, uint32_t nnodes, const dafs_node_input* in, const dd_params& dp, const dd_switches& sw) {
  const size_t first = c->dd_open.size();
  open_blocks ob;
  const int rc = nodes_open_impl(c, ln, nnodes, in, dp, sw, ob);
  if (rc) {
    (void)hipStreamSynchronize(ln.st);
    c->dd_open.resize(first);
    for (size_t b = 0; b < ob.blk0.size(); ++b) { c->dd_free(ob.blk0[b], ob.bytes0[b]); c->dd_free(ob.blk1[b], ob.bytes1[b]); }
  }
  return rc;
}

// One launch of the subgradient loop over the given resident nodes; finished[k] tells which of them are done.
// In two halves, so that launches on two lanes can be in flight together: advance_launch enqueues the kernel and the
// copy of the per-node words, advance_collect waits for them.
struct advance_state {
  std::vector<uint32_t> who, handles, off;
  const uint32_t* paused = nullptr;
  const uint32_t* packed = nullptr;
  bool launched = false;  // the solver may be running: collect must wait for the lane
  bool complete = false;  // ... and the per-node words are on their way to the landing place
};

int advance_launch(dafs_hip_ctx* c, const dd_lane& ln, uint32_t n, const uint32_t* handles, dd_params dp, const dd_switches& sw,
                   uint32_t max_iterations, uint8_t* finished, advance_state& stt) {
  std::vector<dd_node> nodes;
  std::vector<uint32_t>& who = stt.who;
  who.clear();
  stt.handles.assign(handles, handles + n);
  stt.launched = false;
  stt.complete = false;
  size_t lds_max = 0;
  for (uint32_t k = 0; k < n; ++k) {
    if (handles[k] >= c->dd_open.size()) return DAFS_HIP_EINVAL;
    dafs_hip_ctx::dd_open_node& on = c->dd_open[handles[k]];
    if (finished) finished[k] = on.finished ? 1 : 0;
    if (on.finished) continue;
    nodes.push_back(on.nd);
    who.push_back(k);
  }
  if (nodes.empty()) return DAFS_HIP_OK;
  // split mode (three workgroups per node) when the launch is small enough for all of them to be on the
  // machine at once and some node profits; DAFS_HIP_DD_SPLIT=0 turns it off
  bool split = false;
  // three workgroups per node, one per CU (their LDS does not leave room for a second): all of them must fit the device,
  // next to the workgroups of the other lane's launch when that one is still in flight (dafs_hip_nodes_round)
  const uint32_t other_wgs = c->dd_wgs_in_flight[ln.id ^ 1];
  if (sw.split && (int)(nodes.size() * 3 + other_wgs) <= c->num_cus - 16)
    for (size_t b = 0; b < nodes.size(); ++b) split = split || (c->dd_open[handles[who[b]]].split_lds != 0 && !c->dd_open[handles[who[b]]].no_split);
  for (size_t b = 0; b < nodes.size(); ++b) {
    const dafs_hip_ctx::dd_open_node& on = c->dd_open[handles[who[b]]];
    if (split && on.split_lds && !on.no_split) {
      nodes[b].split = 1;
      nodes[b].lds_flags &= kLdsNwTab;  // the leader keeps the alignment DP only
      lds_max = std::max(lds_max, on.split_lds);
      if (hip_check(hipMemsetAsync(nodes[b].sync, 0, 4, ln.st))) return DAFS_HIP_ELAUNCH;  // clear the exit mark of the last launch
    } else {
      nodes[b].split = 0;
      lds_max = std::max(lds_max, on.lds);
    }
  }
  dp.slice = max_iterations;
  int rc;
  for (size_t b = 0; b < nodes.size(); ++b)  // the form each node takes in THIS launch against what its block holds
    if ((rc = plan_check(nodes[b], nodes[b].split != 0, !(dp.skip_xy && nodes[b].ncbp_cap == 0)))) return rc;
  if ((rc = ln.d_nodes->upload(nodes.data(), nodes.size(), ln.st))) return rc;
  if ((rc = ln.d_paused->reserve(nodes.size()))) return rc;
  for (size_t b = 0; b < nodes.size(); ++b) c->dd_open[handles[who[b]]].in_flight = true;
  c->dd_wgs_in_flight[ln.id] = (uint32_t)nodes.size() * (split ? 3u : 1u);
  stt.launched = true;  // from here on advance_collect has something to wait for, whatever fails below
  if ((rc = dd_solve_launch(ln.d_nodes->ptr, (uint32_t)nodes.size(), dp, lds_max, split, ln.d_paused->ptr, ln.st))) return rc;
  // the result words of every node of the launch come along (one packed copy): a node that finishes here needs no
  // copy and no synchronisation of its own in dafs_hip_nodes_result
  stt.off.assign(nodes.size() + 1, 0);
  for (size_t b = 0; b < nodes.size(); ++b) stt.off[b + 1] = stt.off[b] + (uint32_t)((nodes[b].info + 16) - nodes[b].f[0].ss);
  const size_t total = stt.off[nodes.size()];
  dev_buf<uint32_t>& d_off = c->d_pack_off[ln.id];
  dev_buf<uint32_t>& d_pack = c->d_pack[ln.id];
  if ((rc = d_off.reserve(nodes.size()))) return rc;
  if ((rc = d_pack.reserve(total))) return rc;
  uint32_t* landing = c->pinned_words(ln.id, 2 * nodes.size() + total);
  if (!landing) return DAFS_HIP_ENOMEM;
  memcpy(landing + nodes.size(), stt.off.data(), nodes.size() * 4);  // staged in pinned memory: the upload stays asynchronous
  if (hip_check(hipMemcpyAsync(d_off.ptr, landing + nodes.size(), nodes.size() * 4, hipMemcpyHostToDevice, ln.st))) return DAFS_HIP_ELAUNCH;
  if ((rc = dd_pack_launch(ln.d_nodes->ptr, (uint32_t)nodes.size(), d_off.ptr, d_pack.ptr, ln.st))) return rc;
  stt.paused = landing;
  stt.packed = landing + 2 * nodes.size();
  if (hip_check(hipMemcpyAsync(landing, ln.d_paused->ptr, nodes.size() * 4, hipMemcpyDeviceToHost, ln.st))) return DAFS_HIP_ELAUNCH;
  if (total && hip_check(hipMemcpyAsync(landing + 2 * nodes.size(), d_pack.ptr, total * 4, hipMemcpyDeviceToHost, ln.st))) return DAFS_HIP_ELAUNCH;
  stt.complete = true;
  return DAFS_HIP_OK;
}

int advance_collect(dafs_hip_ctx* c, const dd_lane& ln, advance_state& stt, uint8_t* finished) {
  if (!stt.launched) return DAFS_HIP_OK;
  const bool sync_failed = hip_check(hipStreamSynchronize(ln.st));
  c->dd_wgs_in_flight[ln.id] = 0;
  for (size_t b = 0; b < stt.who.size(); ++b) c->dd_open[stt.handles[stt.who[b]]].in_flight = false;
  stt.launched = false;
  if (sync_failed || !stt.complete) return DAFS_HIP_ELAUNCH;  // a launch that failed half-way: its nodes stay unfinished
  for (size_t b = 0; b < stt.who.size(); ++b) {
    const uint32_t h = stt.handles[stt.who[b]];
    const bool done = stt.paused[b] == 0;
    if (stt.paused[b] == 2 && !c->dd_open[h].no_split) { c->dd_open[h].no_split = true; ++c->dd_demotions; }  // its folders were lost: from now on the one-workgroup form
    c->dd_open[h].finished = done;
    if (done) c->dd_open[h].result.assign(stt.packed + stt.off[b], stt.packed + stt.off[b + 1]);
    if (finished) finished[stt.who[b]] = done ? 1 : 0;
  }
  return DAFS_HIP_OK;
}

int nodes_advance(dafs_hip_ctx* c, uint32_t n, const uint32_t* handles, dd_params dp, const dd_switches& sw, uint32_t max_iterations, uint8_t* finished) {
  advance_state stt;
  const dd_lane ln = lane_of(c, 0);
  const int rc = advance_launch(c, ln, n, handles, dp, sw, max_iterations, finished, stt);
  const int rc2 = advance_collect(c, ln, stt, finished);  // also after a failure: whatever was enqueued is waited for
  return rc ? rc : rc2;
}

int nodes_result(dafs_hip_ctx* c, uint32_t handle, dafs_node_output* out, bool stamps) {
  if (handle >= c->dd_open.size() || !c->dd_open[handle].finished || c->dd_open[handle].released || c->dd_open[handle].in_flight) return DAFS_HIP_EINVAL;
  const dd_node& nd = c->dd_open[handle].nd;
  uint32_t info[16];
  float score = 0.0f;
  // x, y, z, score and info were carved back to back (nodes_open): one copy brings them all
  const dd_fold &fx = nd.f[0], &fy = nd.f[1];
  const uint8_t* lo = (const uint8_t*)fx.ss;
  const uint8_t* hi = (const uint8_t*)(nd.info + 16);
  if (hi <= lo || (size_t)(hi - lo) > ((size_t)2 * fx.L + fy.L + 64) * 4 + 8 * 256) return DAFS_HIP_EINVAL;
  std::vector<uint8_t> blob((size_t)(hi - lo));
  const std::vector<uint32_t>& pre = c->dd_open[handle].result;
  if (pre.size() * 4 == blob.size()) memcpy(blob.data(), pre.data(), blob.size());  // came along with the launch the node finished in
  else if (hip_check(hipMemcpyAsync(blob.data(), lo, blob.size(), hipMemcpyDeviceToHost, c->stream)) || hip_check(hipStreamSynchronize(c->stream)))
    return DAFS_HIP_ELAUNCH;
  auto at = [&](const void* dev_ptr) { return blob.data() + ((const uint8_t*)dev_ptr - lo); };
  if (out->x) memcpy(out->x, at(fx.ss), (size_t)fx.L * 4);
  if (out->y) memcpy(out->y, at(fy.ss), (size_t)fy.L * 4);
  if (out->z) memcpy(out->z, at(nd.z), (size_t)fx.L * 4);
  memcpy(&score, at(nd.score), 4);
  memcpy(info, at(nd.info), sizeof info);
  if (stamps && ((dd_fold_form(nd.fold_fast, 0) | dd_fold_form(nd.fold_fast, 1)) & (kFoldSpan | kFoldWg))) {
    uint32_t sy[8] = {0};
    if (!hip_check(hipMemcpy(sy, nd.sync, sizeof sy, hipMemcpyDeviceToHost)))
      fprintf(stderr, "dd node L1=%u L2=%u folders | us: x-dp %.0f y-dp %.0f tracebacks %.0f\n", fx.L, fy.L, sy[5] / 100.0, sy[6] / 100.0, sy[7] / 100.0);
  }
  if (stamps)
    fprintf(stderr, "dd node L1=%u L2=%u n=%u+%u ncbp=%u iters=%u slow-xy=%u+%u | us: x-dp %.0f x-traceback %.0f wait %.0f cbp %.0f update %.0f tail %.0f | y %.0f z %.0f flags %x\n", fx.L,
            fy.L, fx.n, fy.n, info[0], info[1], info[4], info[5], info[8] / 100.0, info[9] / 100.0, info[10] / 100.0, info[11] / 100.0, info[12] / 100.0,
            info[13] / 100.0, info[14] / 100.0, info[15] / 100.0, nd.lds_flags);
  out->score = score;
  out->ncbp = info[0];
  out->iterations = info[1];
  out->violated = info[2];
  {  // The node's device memory is free for the nodes opened from now on.  Nothing can still use it: a node only becomes
     // `finished` in advance_collect, after its lane's stream has been drained, and a finished node is in no later launch.
     // No other open node may lie in the range (the free list would hand it out a second time).
    dafs_hip_ctx::dd_open_node& on = c->dd_open[handle];
    for (int k = 0; k < 2; ++k) {
      if (on.blk[k] && c->dd_range_live(on.blk[k], on.blk_bytes[k], &on)) {
        fprintf(stderr, "dafs_hip: node %u shares device memory with another open node\n", handle);
        return DAFS_HIP_ELAUNCH;
      }
      c->dd_free(on.blk[k], on.blk_bytes[k]);
    }
    on.released = true;
  }
  return info[3] ? DAFS_HIP_ELAUNCH : DAFS_HIP_OK;  // info[3]: the alignment traceback left the envelope
}

}  // namespace

// ---- resident nodes: the progressive phase without level barriers --------------------------------
// A node opened here stays on the device until dafs_hip_nodes_close.  dafs_hip_nodes_advance runs at
// most max_iterations further subgradient iterations of every listed node in ONE launch and reports
// which of them have finished; unfinished nodes simply take part in the next call, next to whatever
// nodes became ready in the meantime.  A node's results do not depend on how its iterations were cut
// into launches.
extern "C" int dafs_hip_nodes_open(dafs_hip_ctx* c, uint32_t nnodes, const dafs_node_input* in, const dafs_dd_params* prm, uint32_t* handles) {
  if (!c || !in || !prm || !handles || nnodes == 0) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const uint32_t first = (uint32_t)c->dd_open.size();
  const dd_switches sw = read_switches();
  const int rc = nodes_open(c, lane_of(c, 0), nnodes, in, device_params(prm, sw), sw);
  if (rc) return rc;
  for (uint32_t b = 0; b < nnodes; ++b) handles[b] = first + b;
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_nodes_advance(dafs_hip_ctx* c, uint32_t n, const uint32_t* handles, const dafs_dd_params* prm, uint32_t max_iterations,
                                      uint8_t* finished) {
  if (!c || !handles || !prm || n == 0) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const dd_switches sw = read_switches();
  return nodes_advance(c, n, handles, device_params(prm, sw), sw, max_iterations, finished);
}

// One round of the progressive phase in a single call: the open nodes advance (lane 0) while the nodes whose children have
// just finished are set up and started beside them (lane 1) -- their set-up kernels (averages, lists, constraints: ~0.8 ms
// a call, one or two workgroups busy) no longer stand between two launches of the solver.  With budget_us > 0 every node of
// the round also stops at the same moment (dd_params::budget), so the late starters do not stretch the round.
extern "C" int dafs_hip_nodes_round(dafs_hip_ctx* c, uint32_t n_new, const dafs_node_input* in, uint32_t* new_handles, uint32_t n_old,
                                    const uint32_t* old_handles, const dafs_dd_params* prm, uint32_t max_iterations, uint32_t budget_us,
                                    uint8_t* finished_old, uint8_t* finished_new) {
  if (!c || !prm || (n_new && (!in || !new_handles)) || (n_old && !old_handles) || (n_new == 0 && n_old == 0)) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const dd_switches sw = read_switches();
  dd_params dp = device_params(prm, sw);
  dp.budget = (unsigned long long)budget_us * 100ull;  // wall_clock64 ticks at 100 MHz
  int rc = DAFS_HIP_OK;
  advance_state st_old, st_new;
  const dd_lane l0 = lane_of(c, 0);
  // without open nodes there is nothing to overlap with: everything on the main lane
  const dd_lane l1 = n_old ? lane_of(c, 1) : l0;
  if (n_old) {
    if (dp.budget) {
      if ((rc = c->d_tref.reserve(1))) return rc;
      if (hip_check(hipMemsetAsync(c->d_tref.ptr, 0, sizeof(unsigned long long), l0.st))) return DAFS_HIP_ELAUNCH;
      dp.t_ref = c->d_tref.ptr;
      dp.t_ref_write = 1;
    }
    if ((rc = advance_launch(c, l0, n_old, old_handles, dp, sw, max_iterations, finished_old, st_old))) {
      (void)advance_collect(c, l0, st_old, finished_old);  // whatever part of the launch was enqueued is waited for
      return rc;
    }
  }
  if (n_new) {
    const uint32_t first = (uint32_t)c->dd_open.size();
    dd_params dpn = dp;
    dpn.t_ref_write = 0;  // a late starter takes the round's reference tick (none when it runs alone)
    if (!n_old) dpn.t_ref = nullptr;
    rc = nodes_open(c, l1, n_new, in, dpn, sw);
    if (rc) { (void)advance_collect(c, l0, st_old, finished_old); return rc; }
    for (uint32_t b = 0; b < n_new; ++b) new_handles[b] = first + b;
    rc = advance_launch(c, l1, n_new, new_handles, dpn, sw, max_iterations, finished_new, st_new);
  }
  const int rc0 = advance_collect(c, l0, st_old, finished_old);
  const int rc1 = n_new ? advance_collect(c, l1, st_new, finished_new) : DAFS_HIP_OK;
  return rc ? rc : (rc0 ? rc0 : rc1);
}

extern "C" int dafs_hipk_dd_node_plan(uint32_t len1, uint32_t len2, dafs_dd_node_plan* out) {
  if (!out || !len1 || !len2) return DAFS_HIP_EINVAL;
  *out = plan_node(len1, len2, read_switches());
  return DAFS_HIP_OK;
}

extern "C" uint32_t dafs_hipk_dd_lds_words(uint32_t len1, uint32_t len2, uint32_t lds_flags, uint32_t fold_fast, int role) {
  const uint32_t r = role == 2 ? 1 : 0;
  return role ? dd_folder_lds(r ? len2 : len1, dd_fold_form(fold_fast, r), dd_fold_k(fold_fast, r)).end : dd_node_lds(len1, len2, lds_flags).end;
}

extern "C" int dafs_hip_nodes_result(dafs_hip_ctx* c, uint32_t handle, dafs_node_output* out) {
  if (!c || !out) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  return nodes_result(c, handle, out, read_switches().stamps);
}

// A read-only look at what the set-up kernels of nodes_open wrote for one resident node (tests).  The sizes come from the
// descriptor the open call kept (dd_open_node::nd); the lengths of the entry lists from their own last row pointer.
extern "C" int dafs_hip_node_peek(dafs_hip_ctx* c, uint32_t handle, int what, void* dst, uint64_t capacity_bytes, uint64_t* bytes_out) {
  if (!c || !dst || !bytes_out) return DAFS_HIP_EINVAL;
  if (handle >= c->dd_open.size() || c->dd_open[handle].released || c->dd_open[handle].in_flight) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const dd_node& nd = c->dd_open[handle].nd;
  const dd_fold &fx = nd.f[0], &fy = nd.f[1];
  const size_t L1 = fx.L, L2 = fy.L;
  // both lanes: the node may have been opened or advanced on either (dafs_hip_nodes_round)
  if (hip_check(hipStreamSynchronize(c->stream)) || (c->node_stream && hip_check(hipStreamSynchronize(c->node_stream)))) return DAFS_HIP_ELAUNCH;
  const void* src = nullptr;
  size_t bytes = 0;
  const uint32_t* count_at = nullptr;  // entry lists: as many words as this row pointer says
  switch (what) {
    case DAFS_PEEK_P_X: src = fx.p; bytes = L1 * L1 * 4; break;
    case DAFS_PEEK_P_Y: src = fy.p; bytes = L2 * L2 * 4; break;
    case DAFS_PEEK_P_Z: src = nd.p_z; bytes = L1 * L2 * 4; break;
    case DAFS_PEEK_X_PTR: src = fx.ptr; bytes = (L1 + 1) * 4; break;
    case DAFS_PEEK_Y_PTR: src = fy.ptr; bytes = (L2 + 1) * 4; break;
    case DAFS_PEEK_X_COL: src = fx.col; count_at = fx.ptr + L1; break;
    case DAFS_PEEK_Y_COL: src = fy.col; count_at = fy.ptr + L2; break;
    case DAFS_PEEK_X_MAP: src = fx.map; bytes = L1 * L1 * 4; break;
    case DAFS_PEEK_Y_MAP: src = fy.map; bytes = L2 * L2 * 4; break;
    case DAFS_PEEK_PZ_PTR: src = nd.pz_ptr; bytes = (L1 + 1) * 4; break;
    case DAFS_PEEK_PZ_K: src = nd.pz_k; count_at = nd.pz_ptr + L1; break;
    case DAFS_PEEK_CZ_PTR: src = nd.cz_ptr; bytes = (L1 + 1) * 4; break;
    case DAFS_PEEK_CZ_K: src = nd.cz_k; count_at = nd.cz_ptr + L1; break;
    case DAFS_PEEK_ZMAP: src = nd.zmap; bytes = L1 * L2 * 4; break;
    case DAFS_PEEK_ENV: src = nd.env; bytes = 2 * (L1 + 1) * 4; break;
    case DAFS_PEEK_ENV4: src = nd.env4; bytes = 2 * (L1 + 130) * 4; break;
    case DAFS_PEEK_CBP_CNT: src = nd.cbp_cnt; count_at = fx.ptr + L1; break;
    case DAFS_PEEK_CBP:  // carved with the folding arrays' block: a node that does not fold (skip_uncoupled_folds) has no pair and keeps none
      if (!fx.w.dp) return DAFS_HIP_EINVAL;
      src = nd.cbp; bytes = (size_t)nd.ncbp_cap * 32; break;
    default: return DAFS_HIP_EINVAL;
  }
  if (!src) return DAFS_HIP_EINVAL;
  if (count_at) {
    uint32_t n = 0;
    if (hip_check(hipMemcpy(&n, count_at, 4, hipMemcpyDeviceToHost))) return DAFS_HIP_ELAUNCH;
    bytes = (size_t)n * 4;
  }
  if (bytes > capacity_bytes) return DAFS_HIP_EINVAL;
  if (bytes && hip_check(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost))) return DAFS_HIP_ELAUNCH;
  *bytes_out = bytes;
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_nodes_close(dafs_hip_ctx* c) {
  if (!c) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  if (hip_check(hipStreamSynchronize(c->stream))) return DAFS_HIP_ELAUNCH;
  c->dd_reset();
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_nodes_demotions(dafs_hip_ctx* c, uint32_t* n) {
  if (!c || !n) return DAFS_HIP_EINVAL;
  *n = c->dd_demotions;
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_nodes_memory(dafs_hip_ctx* c, uint64_t* reserved, uint64_t* in_use, uint64_t* peak) {
  if (!c) return DAFS_HIP_EINVAL;
  uint64_t r = 0;
  for (const dafs_hip_ctx::dd_chunk& ch : c->dd_chunks) r += ch.cap;
  if (reserved) *reserved = r;
  if (in_use) *in_use = c->dd_in_use;
  if (peak) *peak = c->dd_peak;
  return DAFS_HIP_OK;
}

// One batch of independent nodes, start to finish (the level-synchronous form; also what the refinement
// steps use).  Not to be mixed with open resident nodes.
extern "C" int dafs_hip_solve_nodes(dafs_hip_ctx* c, uint32_t nnodes, const dafs_node_input* in, const dafs_dd_params* prm,
                                    dafs_node_output* out) {
  if (!c || !in || !prm || !out || nnodes == 0) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  if (!c->dd_open.empty()) return DAFS_HIP_EINVAL;
  const dd_switches sw = read_switches();
  const dd_params dp = device_params(prm, sw);
  int rc = nodes_open(c, lane_of(c, 0), nnodes, in, dp, sw);
  std::vector<uint32_t> handles(nnodes);
  for (uint32_t b = 0; b < nnodes; ++b) handles[b] = b;
  // one launch runs every node to its end -- unless a split node lost its folding workgroups and was parked for the
  // one-workgroup form (k_dd_solve): then the unfinished nodes go round again
  std::vector<uint8_t> fin(nnodes, 0);
  for (int round = 0; !rc && round < 4; ++round) {
    rc = nodes_advance(c, nnodes, handles.data(), dp, sw, 0, fin.data());
    if (std::all_of(fin.begin(), fin.end(), [](uint8_t f) { return f != 0; })) break;
  }
  if (!rc && !std::all_of(fin.begin(), fin.end(), [](uint8_t f) { return f != 0; })) rc = DAFS_HIP_ELAUNCH;
  for (uint32_t b = 0; b < nnodes && !rc; ++b) rc = nodes_result(c, b, &out[b], dp.stamps != 0);
  (void)hipStreamSynchronize(c->stream);
  c->dd_reset();
  return rc;
}

// Averaged base-pairing matrix of an alignment and its MEA structure: the final step of
// DAFS::run (dafs.cpp:1857-1871) without the RNAalifold term.  p_out (len*len,
// optional) receives the averaged matrix.
// bps: the store to average; by_row: its index is the alignment row (dafs_hip_update_basepairing) instead of the sequence.
// decode = false stops after the average (ss / score untouched).
static int average_and_decode(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint32_t* seq, const uint8_t* mask, const bp_store& bps, bool by_row,
                              bool decode, float th, uint32_t* ss, float* score, float* p_out) {
  if (!c || !n || !len || !seq || !mask || (decode && !ss)) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  if (!bps.valid) return DAFS_HIP_EINVAL;
  geom g;
  int rc;
  if ((rc = make_geom(c, n, len, seq, mask, g))) return rc;
  dd_node nd;
  dd_fold& f = nd.f[0];  // the one alignment; the node has no second one and no z
  carver cv;
  const size_t LL = (size_t)len * len;
  uint32_t* d_ss = nullptr;
  for (int pass = 0; pass < 2; ++pass) {
    cv.used = 0;
    memset(&nd, 0, sizeof nd);
    f.n = n; f.L = len;
    f.seq = cv.take<uint32_t>(n);
    f.rank = cv.take<uint32_t>((size_t)n * len);
    f.idx = cv.take<uint32_t>(g.idx.size() + 1);
    f.idxoff = cv.take<uint32_t>(n);
    f.p = cv.take<float>(LL);
    carve_nuss(cv, len, f.w);
    d_ss = cv.take<uint32_t>((size_t)len + 1);
    nd.score = cv.take<float>(1);
    if (pass == 0) {
      if ((rc = c->work.reserve(cv.used + 256))) return rc;
      cv.base = c->work.ptr;
    }
  }
  if (hip_check(hipMemsetAsync(f.p, 0, LL * 4, c->stream))) return DAFS_HIP_ELAUNCH;
  std::vector<uint32_t> rows(n);
  for (uint32_t r = 0; r < n; ++r) rows[r] = by_row ? r : seq[r];
  if (hip_check(hipMemcpyAsync((void*)f.seq, rows.data(), n * 4, hipMemcpyHostToDevice, c->stream))) return DAFS_HIP_ELAUNCH;
  if (hip_check(hipMemcpyAsync((void*)f.rank, g.rank.data(), g.rank.size() * 4, hipMemcpyHostToDevice, c->stream))) return DAFS_HIP_ELAUNCH;
  if (hip_check(hipMemcpyAsync((void*)f.idx, g.idx.data(), g.idx.size() * 4, hipMemcpyHostToDevice, c->stream))) return DAFS_HIP_ELAUNCH;
  if (hip_check(hipMemcpyAsync((void*)f.idxoff, g.idxoff.data(), n * 4, hipMemcpyHostToDevice, c->stream))) return DAFS_HIP_ELAUNCH;
  if ((rc = c->d_nodes.upload(&nd, 1, c->stream))) return rc;
  mp_store_dev none;
  memset(&none, 0, sizeof none);
  if ((rc = dd_avg_launch(c->d_nodes.ptr, 1, len, none, bps.view(), 0, 0, c->stream))) return rc;
  float s = 0;
  if (decode) {
    if ((rc = nussinov_launch(len, f.p, nullptr, 0.0f, th, f.w, d_ss, nd.score, c->stream))) return rc;
    if (hip_check(hipMemcpyAsync(ss, d_ss, (size_t)len * 4, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
    if (hip_check(hipMemcpyAsync(&s, nd.score, 4, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
  }
  if (p_out && hip_check(hipMemcpyAsync(p_out, f.p, LL * 4, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
  if (hip_check(hipStreamSynchronize(c->stream))) return DAFS_HIP_ELAUNCH;
  if (score) *score = s;
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_consensus_structure(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint32_t* seq, const uint8_t* mask,
                                            float th, uint32_t* ss, float* score, float* p_out) {
  if (!c) return DAFS_HIP_EINVAL;
  return average_and_decode(c, n, len, seq, mask, c->bp[c->cur_bp], false, true, th, ss, score, p_out);
}

// Many alignments in one call.  Per chunk (greedy in input order under a byte budget): every alignment
// is carved out of c->work as average_and_decode carves its one -- the small arrays of all of them first, so that one upload
// brings the geometry, the node and the decoder descriptors, and the structures and scores back to back, so that one copy
// brings the results -- then, size class by size class, one dd_avg_launch over the class's nodes and one k_nussinov_batch
// over its descriptors.  Each alignment takes the form nussinov_launch gives its width, so its bits are the single call's.
namespace {

struct cs_class { uint32_t threads; size_t lds_cap; };
// Size classes of a launch.  The decoder takes ~130 VGPRs, three wavefronts per SIMD, so registers admit twelve wavefronts per
// CU whatever the workgroup size.  Up to 256 columns one wavefront sweeps a span in one step: 64
// threads, twelve workgroups per CU.  Up to 48 KB of LDS (~1 000 columns) 256 threads, three workgroups per CU by registers
// and by LDS alike.  Wider: the 512 threads of the single decoder, one workgroup per CU (opt-in above 64 KB).  The form on
// global tables (no LDS) has the last class to itself, so that a 12 000-column alignment does not set the averaging
// kernel's row length for a class of narrow ones.
constexpr uint32_t kCsClassCount = 4, kCsGlobalClass = 3;
const cs_class kCsClasses[kCsClassCount] = {{64, 12320}, {256, 48 * 1024}, {512, kDdLdsBudget}, {512, 0}};
const uint32_t kCsMaxLaunch = 32768;  // alignments per chunk: the averaging kernel's grid has one y per node

uint32_t cs_class_of(uint32_t L, uint32_t form, size_t lds) {
  if (form == DAFS_HIP_NONE) return kCsGlobalClass;
  if (L <= 256 && lds <= kCsClasses[0].lds_cap) return 0;
  return lds <= kCsClasses[1].lds_cap ? 1 : 2;
}

// The level loop of a chunk over m alignments whose matrices stand on the device, in class order.
struct lv_run {
  uint32_t m, K;
  const float* th;           // [K]
  const uint32_t* first_of;  // [kCsClassCount + 1]: the classes' ranges of the m alignments
  const size_t* lds_of;      // per class
  const uint32_t* len_of;
  const cs_desc* descs;      // host, [m]: ss = the level's own array, score = the first of the alignment's K scores
  const lv_desc* d_lv;       // device, [m]
  uint8_t* d_up;             // device, lv_up_bytes(m, C): the descriptors and indices of the alignments still going, per level
  uint32_t* d_flags;         // device, [K][m]
  // thresholds chosen by pseudo-expected accuracy; C = 0: they are given, th[K], and the rest is unused
  uint32_t C;
  const float* cand;         // [C]
  const pea_desc* pea;       // host, [m]
  const pea_desc* d_pea;     // device, [m]
};
size_t lv_up_bytes(uint32_t m, uint32_t C) { return (size_t)m * ((C ? C : 1) * sizeof(cs_desc) + 4); }

// What the choice of section 27 keeps per chunk beside the structures: the sums and the chosen candidates of its m alignments,
// carved back to back behind the scores, so that one fill clears them and the results' one copy brings them, and the
// candidates' scores.
struct pea_arrays {
  uint64_t *sum = nullptr, *tp = nullptr, *ctp = nullptr, *base = nullptr;
  uint32_t *chosen = nullptr, *np = nullptr, *cnp = nullptr;
  float* cscore = nullptr;
  size_t fill_bytes = 0;
  void carve_results(carver& cv, size_t m, uint32_t K, uint32_t C) {
    sum = cv.take<uint64_t>(m);
    tp = cv.take<uint64_t>(m * K);
    ctp = cv.take<uint64_t>(m * K * C);
    chosen = cv.take<uint32_t>(m * K);
    np = cv.take<uint32_t>(m * K);
    cnp = cv.take<uint32_t>(m * K * C);
    base = cv.take<uint64_t>(m * 2);
    // the one fill: from the first of these arrays to the end of the last (the carver only moves forward; the padding
    // between them belongs to nobody).  Null in the sizing pass, where nothing is filled.
    fill_bytes = sum ? (size_t)((const uint8_t*)(base + m * 2) - (const uint8_t*)sum) : 0;
  }
  void carve_scores(carver& cv, size_t m, uint32_t C) { cscore = cv.take<float>(m * C); }
  // alignment j's descriptor; the caller sets css
  pea_desc desc(size_t j, uint32_t K, uint32_t C, uint32_t L, const float* p, uint32_t* lss, float* score) const {
    pea_desc d;
    memset(&d, 0, sizeof d);
    d.L = L; d.p = p; d.lss = lss; d.score = score; d.cscore = cscore + j * C;
    d.sum = sum + j; d.base = base + 2 * j; d.tp = tp + j * K; d.ctp = ctp + j * K * C;
    d.chosen = chosen + j * K; d.np = np + j * K; d.cnp = cnp + j * K * C;
    return d;
  }
};

// the caller's arrays of the choice; each may be null
struct pea_out { uint32_t* chosen; uint64_t* sum_p; uint64_t* tp; uint32_t* npairs; uint64_t* cand_tp; uint32_t* cand_pairs; };

// Alignment j's part of the copied results (`at` maps a device pointer to its bytes) into the caller's arrays at alignment a.
// ran: the levels it was launched at; the others chose nothing.
template <class At>
void pea_results(const pea_arrays& pa, const At& at, size_t j, size_t a, uint32_t K, uint32_t C, uint32_t ran, const pea_out& o) {
  if (o.sum_p) memcpy(o.sum_p + a, at(pa.sum + j), 8);
  if (o.tp) memcpy(o.tp + a * K, at(pa.tp + j * K), (size_t)K * 8);
  if (o.npairs) memcpy(o.npairs + a * K, at(pa.np + j * K), (size_t)K * 4);
  if (o.cand_tp) memcpy(o.cand_tp + a * K * C, at(pa.ctp + j * K * C), (size_t)K * C * 8);
  if (o.cand_pairs) memcpy(o.cand_pairs + a * K * C, at(pa.cnp + j * K * C), (size_t)K * C * 4);
  if (o.chosen) {
    memcpy(o.chosen + a * K, at(pa.chosen + j * K), (size_t)ran * 4);
    for (uint32_t k = ran; k < K; ++k) o.chosen[a * K + k] = DAFS_HIP_NONE;
  }
}

// Level 0 decodes every alignment; level k > 0 those with a pair at level k - 1, after the mask of that level.  One copy up
// per level (descriptors with the level's score slot, and the indices), one copy of m flags down between two levels.
// With candidates (r.C): S of every matrix before the first mask; per level the decoder once per candidate, each into its
// own structure and score through its own descriptors (the work tables are shared: the launches follow one another), then
// k_pea_pick, which leaves the chosen one where the merge reads the level's structure.
// ran[j]: the levels alignment j was launched at.  up, flags: host buffers that must outlive the frame.
int run_levels(call_frame& f, const lv_run& r, std::vector<uint8_t>& up, std::vector<uint32_t>& flags, std::vector<uint32_t>& ran) {
  const uint32_t m = r.m;
  std::vector<uint32_t> act(m);
  for (uint32_t j = 0; j < m; ++j) act[j] = j;
  ran.assign(m, 0);
  flags.assign(m, 0);
  const uint32_t W = r.C ? r.C : 1;  // decodes per level; descriptors candidate by candidate, m apart
  cs_desc* d_cs = (cs_desc*)r.d_up;
  const size_t act_off = (size_t)m * W * sizeof(cs_desc);
  uint32_t* d_act = (uint32_t*)(r.d_up + act_off);
  int rc;
  for (uint32_t k = 0; k < r.K && !act.empty(); ++k) {
    const uint32_t n = (uint32_t)act.size();
    up.resize(lv_up_bytes(m, r.C));
    uint32_t first[kCsClassCount + 1] = {0};  // the classes' ranges of the active ones (act keeps the class order)
    for (uint32_t x = 0, cls = 0; x < n; ++x) {
      cs_desc d = r.descs[act[x]];
      d.score += k;
      for (uint32_t c = 0; c < W; ++c) {
        if (r.C) { d.ss = const_cast<uint32_t*>(r.pea[act[x]].css) + (size_t)c * (d.L + 1); d.score = const_cast<float*>(r.pea[act[x]].cscore) + c; }
        memcpy(up.data() + ((size_t)c * m + x) * sizeof(cs_desc), &d, sizeof d);
      }
      while (act[x] >= r.first_of[cls + 1]) ++cls;
      ++first[cls + 1];
      ++ran[act[x]];
    }
    for (uint32_t cls = 0; cls < kCsClassCount; ++cls) first[cls + 1] += first[cls];
    memcpy(up.data() + act_off, act.data(), (size_t)n * 4);
    if (f.up(d_cs, up.data(), ((size_t)(W - 1) * m + n) * sizeof(cs_desc)) || f.up(d_act, up.data() + act_off, (size_t)n * 4)) return DAFS_HIP_ELAUNCH;
    for (uint32_t cls = 0; cls < kCsClassCount; ++cls) {
      const uint32_t nc = first[cls + 1] - first[cls];
      if (!nc) continue;
      if (k && (rc = levels_mask_launch(r.d_lv, d_act + first[cls], nc, r.len_of[cls], f.st))) return rc;
      if (r.C && !k && (rc = pea_total_launch(r.d_pea, d_act + first[cls], nc, r.len_of[cls], f.st))) return rc;
      for (uint32_t c = 0; c < W; ++c)
        if ((rc = nussinov_batch_launch(d_cs + (size_t)c * m + first[cls], nc, r.C ? r.cand[c] : r.th[k], kCsClasses[cls].threads, r.lds_of[cls], f.st))) return rc;
    }
    if (r.C && (rc = pea_pick_launch(r.d_pea, d_act, n, k, r.C, f.st))) return rc;
    const bool more = k + 1 < r.K;
    if ((rc = levels_merge_launch(r.d_lv, d_act, n, k, more, f.st))) return rc;
    if (!more) break;
    if (f.down(flags.data(), r.d_flags + (size_t)k * m, (size_t)m * 4)) return DAFS_HIP_ELAUNCH;
    if ((rc = f.finish())) return rc;  // the one wait between two levels: `up` is rewritten, the next launch list depends on the flags
    std::vector<uint32_t> next;
    for (uint32_t j : act)
      if (flags[j]) next.push_back(j);
    act.swap(next);
  }
  return DAFS_HIP_OK;
}

}  // namespace

// nlevels = 0: the plain call (one decode, straight into the results).  nlevels >= 1: the level-by-level decode of section 25,
// whose level 0 is that same decode into the level's own array, merged by k_levels_merge.  ncand >= 1 (with nlevels >= 1):
// ths are the candidates every level chooses its threshold from (section 27), and po receives what the choice kept.
static int consensus_structures_impl(dafs_hip_ctx* c, uint32_t nalign, const uint32_t* n_rows, const uint32_t* len, const uint32_t* seq,
                                     const uint8_t* mask, uint32_t nlevels, const float* ths, uint32_t* ss, uint8_t* level, float* score,
                                     uint32_t ncand = 0, const pea_out* po = nullptr) {
  if (!c) return DAFS_HIP_EINVAL;
  const bool levels = nlevels != 0;
  const uint32_t C = ncand;
  const uint32_t K = levels ? nlevels : 1;
  const float th = ths[0];
  if (nalign == 0) return DAFS_HIP_OK;
  if (!n_rows || !len || !seq || !mask || !ss) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const bp_store& bps = c->bp[c->cur_bp];
  if (!bps.valid || c->fold_pending) return DAFS_HIP_EINVAL;
  // ---- everything the launches will read, checked on the host first ----
  std::vector<geom> g(nalign);
  std::vector<size_t> row0(nalign + 1, 0), mask0(nalign + 1, 0), col0(nalign + 1, 0);
  std::vector<uint64_t> bytes(nalign);
  for (uint32_t a = 0; a < nalign; ++a) {
    if (!n_rows[a] || !len[a]) return DAFS_HIP_EINVAL;
    row0[a + 1] = row0[a] + n_rows[a];
    mask0[a + 1] = mask0[a] + (size_t)n_rows[a] * len[a];
    col0[a + 1] = col0[a] + len[a];
    bytes[a] = C        ? dafs_host_structure_auto_bytes(n_rows[a], len[a], C)
               : levels ? dafs_host_structure_levels_bytes(n_rows[a], len[a])
                        : dafs_host_structure_bytes(n_rows[a], len[a]);
  }
  for (uint32_t a = 0; a < nalign; ++a) {
    const int rc = make_geom(c, n_rows[a], len[a], seq + row0[a], mask + mask0[a], g[a]);
    if (rc) return rc;
  }
  // tests: budgets that put every alignment in a chunk of its own
  const uint64_t budget = env_uint("DAFS_HIP_CS_BATCH_BYTES", 0, UINT64_MAX, dafs_host_structures_batch_bytes());
  std::vector<uint32_t> chunk_of(nalign);
  int rc;
  if ((rc = dafs_host_pack_greedy(nalign, bytes.data(), budget, chunk_of.data()))) return rc;

  mp_store_dev none;
  memset(&none, 0, sizeof none);
  const bp_store_dev bpv = bps.view();
  std::vector<uint32_t> order;
  std::vector<dd_node> nodes;
  std::vector<cs_desc> descs;
  std::vector<uint8_t> head, out, lv_up;
  std::vector<lv_desc> lv;
  std::vector<uint32_t> lv_flags, lv_ran;
  std::vector<pea_desc> pea;
  call_frame f(c);  // `head`, `out` and the level buffers are in flight when an error ends a chunk early
  for (uint32_t a0 = 0; a0 < nalign;) {
    uint32_t a1 = a0;
    while (a1 < nalign && chunk_of[a1] == chunk_of[a0] && a1 - a0 < kCsMaxLaunch) ++a1;
    const uint32_t m = a1 - a0;
    // the chunk's alignments class by class, input order inside a class
    std::vector<uint32_t> cls(m), form(m);
    uint32_t first_of[kCsClassCount + 1] = {0};
    size_t lds_of[kCsClassCount] = {0};
    uint32_t len_of[kCsClassCount] = {0};
    for (uint32_t k = 0; k < m; ++k) {
      size_t lds = 0;
      form[k] = nussinov_form(len[a0 + k], &lds);
      cls[k] = cs_class_of(len[a0 + k], form[k], lds);
      ++first_of[cls[k] + 1];
      lds_of[cls[k]] = std::max(lds_of[cls[k]], lds);
      len_of[cls[k]] = std::max(len_of[cls[k]], len[a0 + k]);
    }
    for (uint32_t k = 0; k < kCsClassCount; ++k) first_of[k + 1] += first_of[k];
    order.assign(m, 0);
    {
      uint32_t at[kCsClassCount];
      std::copy(first_of, first_of + kCsClassCount, at);
      for (uint32_t k = 0; k < m; ++k) order[at[cls[k]]++] = k;
    }
    // ---- carve: head (uploaded), results (copied back), then the matrices and tables ----
    nodes.assign(m, dd_node());
    descs.assign(m, cs_desc());
    carver cv;
    dd_node* d_nodes = nullptr;
    cs_desc* d_descs = nullptr;
    size_t head_bytes = 0, out_off = 0, out_bytes = 0;
    std::vector<size_t> ss_off(m), level_off(m);
    float* d_scores = nullptr;
    lv_desc* d_lv = nullptr;
    uint8_t* d_lv_up = nullptr;
    uint32_t* d_flags = nullptr;
    pea_desc* d_pea = nullptr;
    pea_arrays pa;
    if (levels) lv.assign(m, lv_desc());
    if (C) pea.assign(m, pea_desc());
    for (int pass = 0; pass < 2; ++pass) {
      cv.used = 0;
      d_nodes = cv.take<dd_node>(m);
      if (levels) d_lv = cv.take<lv_desc>(m);  // the decoder descriptors then go up level by level (run_levels)
      else d_descs = cv.take<cs_desc>(m);
      if (C) d_pea = cv.take<pea_desc>(m);
      for (uint32_t j = 0; j < m; ++j) {
        const uint32_t k = order[j], a = a0 + k;
        dd_node& nd = nodes[j];
        memset(&nd, 0, sizeof nd);
        dd_fold& f = nd.f[0];  // the one alignment; the node has no second one and no z
        f.n = n_rows[a]; f.L = len[a];
        f.seq = cv.take<uint32_t>(f.n);
        f.rank = cv.take<uint32_t>((size_t)f.n * f.L);
        f.idx = cv.take<uint32_t>(g[a].idx.size() + 1);
        f.idxoff = cv.take<uint32_t>(f.n);
      }
      head_bytes = cv.used;
      out_off = (cv.used + 255) & ~(size_t)255;
      for (uint32_t j = 0; j < m; ++j) {
        uint32_t* p = cv.take<uint32_t>((size_t)len[a0 + order[j]] + 1);
        descs[j].ss = p;
        ss_off[j] = (size_t)((uint8_t*)p - cv.base);
        if (levels) {
          lv[j].ss = p;
          lv[j].level = cv.take<uint8_t>(len[a0 + order[j]]);
          level_off[j] = (size_t)(lv[j].level - cv.base);
        }
      }
      d_scores = cv.take<float>((size_t)m * K);
      if (C) pa.carve_results(cv, m, K, C);
      out_bytes = cv.used - out_off;
      if (levels) {
        d_lv_up = cv.take<uint8_t>(lv_up_bytes(m, C));
        d_flags = cv.take<uint32_t>((size_t)m * K);
      }
      if (C) pa.carve_scores(cv, m, C);
      for (uint32_t j = 0; j < m; ++j) {
        const uint32_t L = len[a0 + order[j]];
        dd_fold& f = nodes[j].f[0];
        f.p = cv.take<float>((size_t)L * L);
        carve_nuss(cv, L, f.w);
        nodes[j].score = d_scores + (size_t)j * K;
        descs[j].L = L; descs[j].form = form[order[j]]; descs[j].p = f.p; descs[j].ws = f.w; descs[j].score = d_scores + (size_t)j * K;
        if (levels) {  // the decodes write the level's own array, the merge the results
          uint32_t* lss = cv.take<uint32_t>((size_t)L + 1);
          descs[j].ss = lss;
          lv[j].L = L; lv[j].flag_stride = m; lv[j].p = f.p; lv[j].lss = lss; lv[j].key = cv.take<uint32_t>(L); lv[j].flag = d_flags + j;
          if (C) {
            pea[j] = pa.desc(j, K, C, L, f.p, lss, d_scores + (size_t)j * K);
            pea[j].css = cv.take<uint32_t>((size_t)C * (L + 1));
          }
        }
      }
      if (pass == 0) {
        uint64_t estimate = 0;
        for (uint32_t a = a0; a < a1; ++a) estimate += bytes[a];
        if (cv.used + 256 > estimate) {  // dafs_host_structure_bytes is the bound of this carving
          fprintf(stderr, "dafs_hip: a chunk of %u alignments takes %zu bytes, over its estimate of %llu\n", m, cv.used + 256, (unsigned long long)estimate);
          return DAFS_HIP_ELAUNCH;
        }
        if ((rc = c->work.reserve(cv.used + 256))) return rc;
        cv.base = c->work.ptr;
      }
    }
    head.assign(head_bytes, 0);
    auto put = [&](const void* dst, const void* src, size_t n) {
      if (n) memcpy(head.data() + ((const uint8_t*)dst - cv.base), src, n);
    };
    put(d_nodes, nodes.data(), (size_t)m * sizeof(dd_node));
    if (levels) put(d_lv, lv.data(), (size_t)m * sizeof(lv_desc));
    else put(d_descs, descs.data(), (size_t)m * sizeof(cs_desc));
    if (C) put(d_pea, pea.data(), (size_t)m * sizeof(pea_desc));
    for (uint32_t j = 0; j < m; ++j) {
      const uint32_t a = a0 + order[j];
      const dd_fold& f = nodes[j].f[0];
      put(f.seq, seq + row0[a], (size_t)f.n * 4);
      put(f.rank, g[a].rank.data(), g[a].rank.size() * 4);
      put(f.idx, g[a].idx.data(), g[a].idx.size() * 4);
      put(f.idxoff, g[a].idxoff.data(), (size_t)f.n * 4);
    }
    if (f.up(cv.base, head.data(), head_bytes)) return DAFS_HIP_ELAUNCH;
    // (no fill of the matrices: k_node_avg writes every cell of every row of p)
    for (uint32_t k = 0; k < kCsClassCount; ++k) {
      const uint32_t n = first_of[k + 1] - first_of[k];
      if (!n) continue;
      if ((rc = dd_avg_launch(d_nodes + first_of[k], n, len_of[k], none, bpv, 0, 0, f.st))) return rc;
      if (!levels && (rc = nussinov_batch_launch(d_descs + first_of[k], n, th, kCsClasses[k].threads, lds_of[k], f.st))) return rc;
    }
    if (levels) {
      if (C && f.fill(pa.sum, 0, pa.fill_bytes)) return DAFS_HIP_ELAUNCH;
      const lv_run run = {m, K, ths, first_of, lds_of, len_of, descs.data(), d_lv, d_lv_up, d_flags, C, ths, pea.data(), d_pea};
      if ((rc = run_levels(f, run, lv_up, lv_flags, lv_ran))) return rc;
    }
    out.resize(out_bytes);
    if (f.down(out.data(), cv.base + out_off, out_bytes)) return DAFS_HIP_ELAUNCH;
    if ((rc = f.finish())) return rc;  // per chunk: the next one rewrites `head`
    for (uint32_t j = 0; j < m; ++j) {
      const uint32_t a = a0 + order[j];
      memcpy(ss + col0[a], out.data() + (ss_off[j] - out_off), (size_t)len[a] * 4);
      if (levels && level) memcpy(level + col0[a], out.data() + (level_off[j] - out_off), len[a]);
      if (C && po) pea_results(pa, [&](const void* dev) { return out.data() + ((size_t)((const uint8_t*)dev - cv.base) - out_off); }, j, a, K, C, lv_ran[j], *po);
      if (!score) continue;
      const uint8_t* got = out.data() + ((size_t)((uint8_t*)(d_scores + (size_t)j * K) - cv.base) - out_off);
      const uint32_t ran = levels ? lv_ran[j] : 1;  // the levels this alignment was launched at; the others are empty
      memcpy(score + (size_t)a * K, got, (size_t)ran * 4);
      for (uint32_t k = ran; k < K; ++k) score[(size_t)a * K + k] = 0.0f;
    }
    a0 = a1;
  }
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_consensus_structures(dafs_hip_ctx* c, uint32_t nalign, const uint32_t* n_rows, const uint32_t* len, const uint32_t* seq,
                                             const uint8_t* mask, float th, uint32_t* ss, float* score) {
  return consensus_structures_impl(c, nalign, n_rows, len, seq, mask, 0, &th, ss, nullptr, score);
}

// the candidates of section 27: 1..16 thresholds inside (0, 1), strictly decreasing
static bool auto_args_ok(uint32_t nlevels, uint32_t ncand, const float* cand) {
  if (nlevels < 1 || nlevels > DAFS_HIP_MAX_LEVELS || ncand < 1 || ncand > DAFS_HIP_MAX_CANDIDATES || !cand) return false;
  for (uint32_t c = 0; c < ncand; ++c)
    if (!(cand[c] > 0.0f && cand[c] < 1.0f) || (c && !(cand[c] < cand[c - 1]))) return false;
  return true;
}

static bool levels_args_ok(uint32_t nlevels, const float* th) {
  if (nlevels < 1 || nlevels > DAFS_HIP_MAX_LEVELS || !th) return false;
  for (uint32_t k = 1; k < nlevels; ++k)
    if (!(th[k] > 0.0f)) return false;  // a masked cell (0) must never be a candidate
  return true;
}

extern "C" int dafs_hip_consensus_structures_levels(dafs_hip_ctx* c, uint32_t nalign, const uint32_t* n_rows, const uint32_t* len,
                                                    const uint32_t* seq, const uint8_t* mask, uint32_t nlevels, const float* th, uint32_t* ss,
                                                    uint8_t* level, float* score) {
  if (!c || !levels_args_ok(nlevels, th)) return DAFS_HIP_EINVAL;
  return consensus_structures_impl(c, nalign, n_rows, len, seq, mask, nlevels, th, ss, level, score);
}

extern "C" int dafs_hip_consensus_structures_auto(dafs_hip_ctx* c, uint32_t nalign, const uint32_t* n_rows, const uint32_t* len, const uint32_t* seq,
                                                  const uint8_t* mask, uint32_t nlevels, uint32_t ncand, const float* cand, uint32_t* ss,
                                                  uint8_t* level, float* score, uint32_t* chosen, uint64_t* sum_p, uint64_t* tp,
                                                  uint32_t* npairs, uint64_t* cand_tp, uint32_t* cand_pairs) {
  if (!c || !auto_args_ok(nlevels, ncand, cand)) return DAFS_HIP_EINVAL;
  const pea_out po = {chosen, sum_p, tp, npairs, cand_tp, cand_pairs};
  return consensus_structures_impl(c, nalign, n_rows, len, seq, mask, nlevels, cand, ss, level, score, ncand, &po);
}

// The same decode of one dense host matrix (no store, no average): the matrix goes up as it is and is masked on the device.
// ncand >= 1: th are the candidates, as in consensus_structures_impl.
static int decode_levels_impl(dafs_hip_ctx* c, uint32_t nlevels, const float* th, uint32_t L, const float* p, uint32_t* ss, uint8_t* level,
                              float* score, uint32_t C, const pea_out* po) {
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const size_t LL = (size_t)L * L;
  const uint32_t K = nlevels;
  size_t lds = 0;
  cs_desc desc;
  lv_desc lv;
  memset(&desc, 0, sizeof desc);
  memset(&lv, 0, sizeof lv);
  desc.L = lv.L = L;
  desc.form = nussinov_form(L, &lds);
  const uint32_t cls = cs_class_of(L, desc.form, lds);
  uint32_t first_of[kCsClassCount + 1], len_of[kCsClassCount] = {0};
  size_t lds_of[kCsClassCount] = {0};
  for (uint32_t k = 0; k <= kCsClassCount; ++k) first_of[k] = k > cls ? 1 : 0;
  lds_of[cls] = lds; len_of[cls] = L;
  carver cv;
  lv_desc* d_lv = nullptr;
  uint8_t* d_lv_up = nullptr;
  uint32_t* d_flags = nullptr;
  pea_desc pea;
  pea_desc* d_pea = nullptr;
  pea_arrays pa;
  memset(&pea, 0, sizeof pea);
  size_t out_off = 0, out_bytes = 0;
  for (int pass = 0; pass < 2; ++pass) {
    cv.used = 0;
    d_lv = cv.take<lv_desc>(1);
    d_lv_up = cv.take<uint8_t>(lv_up_bytes(1, C));
    d_flags = cv.take<uint32_t>(K);
    if (C) d_pea = cv.take<pea_desc>(1);
    out_off = (cv.used + 255) & ~(size_t)255;
    lv.ss = cv.take<uint32_t>((size_t)L + 1);
    lv.level = cv.take<uint8_t>(L);
    desc.score = cv.take<float>(K);
    if (C) pa.carve_results(cv, 1, K, C);
    out_bytes = cv.used - out_off;
    if (C) pa.carve_scores(cv, 1, C);
    lv.p = cv.take<float>(LL);
    desc.p = lv.p;
    carve_nuss(cv, L, desc.ws);
    uint32_t* lss = cv.take<uint32_t>((size_t)L + 1);
    desc.ss = lss; lv.lss = lss;
    lv.key = cv.take<uint32_t>(L);
    lv.flag = d_flags; lv.flag_stride = 1;
    if (C) {
      pea = pa.desc(0, K, C, L, lv.p, lss, desc.score);
      pea.css = cv.take<uint32_t>((size_t)C * (L + 1));
    }
    if (pass == 0) {
      const int rc = c->work.reserve(cv.used + 256);
      if (rc) return rc;
      cv.base = c->work.ptr;
    }
  }
  std::vector<uint8_t> out(out_bytes), lv_up;
  std::vector<uint32_t> lv_flags, lv_ran;
  call_frame f(c);
  if (f.up(lv.p, p, LL * 4) || f.up(d_lv, &lv, sizeof lv)) return DAFS_HIP_ELAUNCH;
  if (C && (f.up(d_pea, &pea, sizeof pea) || f.fill(pa.sum, 0, pa.fill_bytes))) return DAFS_HIP_ELAUNCH;
  const lv_run run = {1, K, th, first_of, lds_of, len_of, &desc, d_lv, d_lv_up, d_flags, C, th, &pea, d_pea};
  int rc;
  if ((rc = run_levels(f, run, lv_up, lv_flags, lv_ran))) return rc;
  if (f.down(out.data(), cv.base + out_off, out_bytes)) return DAFS_HIP_ELAUNCH;
  if ((rc = f.finish())) return rc;
  memcpy(ss, out.data() + ((uint8_t*)lv.ss - cv.base - out_off), (size_t)L * 4);
  if (level) memcpy(level, out.data() + (lv.level - cv.base - out_off), L);
  if (score) {
    memcpy(score, out.data() + ((uint8_t*)desc.score - cv.base - out_off), (size_t)lv_ran[0] * 4);
    for (uint32_t k = lv_ran[0]; k < K; ++k) score[k] = 0.0f;
  }
  if (C && po) pea_results(pa, [&](const void* dev) { return out.data() + ((size_t)((const uint8_t*)dev - cv.base) - out_off); }, 0, 0, K, C, lv_ran[0], *po);
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_nussinov_decode_levels(dafs_hip_ctx* c, uint32_t nlevels, const float* th, uint32_t L, const float* p, uint32_t* ss,
                                               uint8_t* level, float* score) {
  if (!c || !p || !ss || L == 0 || !levels_args_ok(nlevels, th)) return DAFS_HIP_EINVAL;
  return decode_levels_impl(c, nlevels, th, L, p, ss, level, score, 0, nullptr);
}

extern "C" int dafs_hip_nussinov_decode_auto(dafs_hip_ctx* c, uint32_t nlevels, uint32_t ncand, const float* cand, uint32_t L, const float* p,
                                             uint32_t* ss, uint8_t* level, float* score, uint32_t* chosen, uint64_t* sum_p, uint64_t* tp,
                                             uint32_t* npairs, uint64_t* cand_tp, uint32_t* cand_pairs) {
  if (!c || !p || !ss || L == 0 || !auto_args_ok(nlevels, ncand, cand)) return DAFS_HIP_EINVAL;
  const pea_out po = {chosen, sum_p, tp, npairs, cand_tp, cand_pairs};
  return decode_levels_impl(c, nlevels, cand, L, p, ss, level, score, ncand, &po);
}

// DAFS::update_basepairing_probability (dafs.cpp:609-712, options --bp-update / --bp-update1; no RNAalifold term, one level
// of brackets): every sequence of the alignment is folded again under the constraint that the common structure ss puts on
// it -- paired columns whose two residues exist in the row become '(' and ')', everything else stays free -- and the
// constrained posteriors (> CUTOFF) are averaged over the rows like the unconstrained ones, cut off at CUTOFF.
// The constraint strings are host work (index mapping); the folds run as one batch, the average on the device.
extern "C" int dafs_hip_update_basepairing(dafs_hip_ctx* c, uint32_t n, uint32_t len, const uint32_t* seq, const uint8_t* mask,
                                           const uint32_t* ss, float* p_out) {
  if (!c || !n || !len || !seq || !mask || !ss || !p_out) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  std::vector<char> str((size_t)len + 1);
  dafs_hip_make_brackets(len, ss, str.data());
  std::vector<std::string> cons(n);
  std::vector<uint32_t> rev(len);
  for (uint32_t r = 0; r < n; ++r) {
    if (seq[r] >= c->len.size()) return DAFS_HIP_EINVAL;
    uint32_t k = 0;
    for (uint32_t i = 0; i < len; ++i) rev[i] = mask[(size_t)r * len + i] ? k++ : DAFS_HIP_NONE;
    if (k != c->len[seq[r]]) return DAFS_HIP_EINVAL;
    std::string& con = cons[r];
    con.assign(k, '?');
    for (uint32_t i = 0; i < len; ++i)
      if (ss[i] != DAFS_HIP_NONE && ss[i] < len && rev[i] != DAFS_HIP_NONE && rev[ss[i]] != DAFS_HIP_NONE) {  // :640-652
        if (str[i] == '(') { con[rev[i]] = '('; con[rev[ss[i]]] = ')'; }
        else { con[rev[i]] = '.'; con[rev[ss[i]]] = '.'; }
      }
  }
  int rc = dafs_fold_rows_constrained(c, n, seq, cons, 0.01f, c->bp_rows);  // CONTRAfold(CUTOFF), dafs.cpp:1704
  if (rc) return rc;
  return average_and_decode(c, n, len, seq, mask, c->bp_rows, true, false, 0.0f, nullptr, nullptr, p_out);
}
