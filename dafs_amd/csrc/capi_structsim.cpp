// dafs_amd/csrc/capi_structsim.cpp -- dafs_hip_structure_scores, dafs_hip_similarity_scored, dafs_hip_get_pair_scores and the
// two host formulas of the structural pair score (structsim.hip; the contract, to the bit).  The
// reference has no counterpart for the score.
//
// Host work: the checks, the task -> (x, y) table of a resident store, the scatter of a launch's {T, terms} into pair order,
// the refusal of a pair with 2^24 terms or more, and the float matrices from the integers.  The device arrays of a launch
// are pieces of the context's work block, which grows once and is reused by every range of a pass.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <functional>
#include <vector>

#include "../../include/dafs_hip.h"
#include "call_host.h"
#include "ctx.h"
#include "hip_util.h"
#include "structsim.h"

using namespace dafs;

extern "C" float dafs_host_structure_score(uint64_t T, uint64_t Wx, uint64_t Wy) {
  const uint64_t w = Wx < Wy ? Wx : Wy;
  if (w == 0) return 0.0f;
  const double s = (double)T / (double)w;
  return (float)(s < 1.0 ? s : 1.0);
}

extern "C" float dafs_host_mix_score(float sim, float str, float w) { return (float)((double)sim + (double)w * ((double)str - (double)sim)); }

namespace {

// {T, terms} of every pair of the resident un-relaxed store st, in the store's pair order (that of dafs_hip_align_fetch)
int score_store(dafs_hip_ctx* c, const mp_store& st, std::vector<uint64_t>& T, std::vector<uint64_t>& terms) {
  const uint64_t np = st.n_tasks;
  T.assign(np, 0);
  terms.assign(np, 0);
  if (np == 0) return DAFS_HIP_OK;
  std::vector<uint2> xy(np);
  for (uint64_t p = 0; p < np; ++p) xy[st.task_of_pair[p]] = make_uint2(st.pair_x[p], st.pair_y[p]);
  std::vector<ulonglong2> out(np);
  carve cv;
  const size_t o_xy = cv.take(np * sizeof(uint2)), o_out = cv.take(np * sizeof(ulonglong2));
  int rc;
  if ((rc = c->work.reserve(cv.reserve_bytes()))) return rc;
  uint2* d_xy = (uint2*)(c->work.ptr + o_xy);
  ulonglong2* d_out = (ulonglong2*)(c->work.ptr + o_out);
  if (hip_check(hipMemcpyAsync(d_xy, xy.data(), np * sizeof(uint2), hipMemcpyHostToDevice, c->stream))) return DAFS_HIP_ELAUNCH;
  // DAFS_HIP_STRUCT_LDS=0 (read per call): no row is copied into LDS (tests reach that form at a small size)
  const uint32_t lds_words = env_off("DAFS_HIP_STRUCT_LDS") ? 0 : (uint32_t)env_uint("DAFS_HIP_STRUCT_LDS_WORDS", 0, kStructLdsWords, kStructLdsWords);
  rc = struct_sim_launch(c->mp_view(st), c->bp[0].view(), d_xy, (uint32_t)np, lds_words, d_out, c->stream);
  if (!rc && hip_check(hipMemcpyAsync(out.data(), d_out, np * sizeof(ulonglong2), hipMemcpyDeviceToHost, c->stream))) rc = DAFS_HIP_ELAUNCH;
  if (hip_check(hipStreamSynchronize(c->stream)) && !rc) rc = DAFS_HIP_ELAUNCH;  // xy and out are read and written until here
  if (rc) return rc;
  for (uint64_t p = 0; p < np; ++p) {
    const ulonglong2 o = out[st.task_of_pair[p]];
    if (o.y >= kStructMaxTerms) {
      char msg[160];
      snprintf(msg, sizeof msg, "structure scores: the pair of sequences %u and %u has %llu terms, the sum takes fewer than %llu", st.pair_x[p],
               st.pair_y[p], o.y, (unsigned long long)kStructMaxTerms);
      set_last_error(msg);
      return DAFS_HIP_EOVERFLOW;
    }
    T[p] = o.x;
    terms[p] = o.y;
  }
  return DAFS_HIP_OK;
}

// W of every sequence from the un-relaxed base-pairing store
int sequence_weights(dafs_hip_ctx* c, std::vector<uint64_t>& W) {
  const uint32_t n = (uint32_t)c->len.size();
  W.assign(n, 0);
  carve cv;
  const size_t o_w = cv.take((size_t)n * 8);
  int rc;
  if ((rc = c->work.reserve(cv.reserve_bytes()))) return rc;
  unsigned long long* d_w = (unsigned long long*)(c->work.ptr + o_w);
  rc = struct_w_launch(c->bp[0].view(), c->d_len.ptr, n, d_w, c->stream);
  if (!rc && hip_check(hipMemcpyAsync(W.data(), d_w, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream))) rc = DAFS_HIP_ELAUNCH;
  if (hip_check(hipStreamSynchronize(c->stream)) && !rc) rc = DAFS_HIP_ELAUNCH;
  return rc;
}

}  // namespace

extern "C" int dafs_hip_structure_scores(dafs_hip_ctx* c, uint64_t* T, uint64_t* terms, uint64_t* W) {
  if (!c || c->len.empty()) return refuse("structure_scores: no context, or a context without sequences");
  if (c->fam.nfam() != 1) return refuse("structure_scores: the context holds several families");
  if (!c->mp[0].valid) return refuse("structure_scores: no un-relaxed matching store (dafs_hip_align_posteriors or dafs_hip_set_mp first)");
  if (!c->bp[0].valid) return refuse("structure_scores: no un-relaxed base-pairing store (dafs_hip_fold_posteriors or dafs_hip_set_bp first)");
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  std::vector<uint64_t> t, k, w;
  int rc;
  if ((rc = score_store(c, c->mp[0], t, k))) return rc;
  if (W && (rc = sequence_weights(c, w))) return rc;
  if (T && !t.empty()) memcpy(T, t.data(), t.size() * 8);
  if (terms && !k.empty()) memcpy(terms, k.data(), k.size() * 8);
  if (W) memcpy(W, w.data(), w.size() * 8);
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_similarity_scored(dafs_hip_ctx* c, int model, float th, uint64_t max_bytes, int kind, float weight, uint64_t* n_ranges_out) {
  if (kind == DAFS_SCORE_SEQUENCE) return dafs_hip_similarity(c, model, th, max_bytes, n_ranges_out);
  if (kind != DAFS_SCORE_STRUCTURE && kind != DAFS_SCORE_MIX) return refuse("similarity_scored: unknown kind of score");
  if (kind == DAFS_SCORE_MIX && !(weight >= 0.0f && weight <= 1.0f)) return refuse("similarity_scored: the weight of the mix must lie in 0 .. 1");
  if (!c || c->len.size() < 2 || c->fam.nfam() != 1) return refuse("similarity_scored: a context of one family of two sequences or more");
  if (!c->bp[0].valid) return refuse("similarity_scored: no un-relaxed base-pairing store (dafs_hip_fold_posteriors or dafs_hip_set_bp first)");
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  const uint32_t n = (uint32_t)c->len.size();
  std::vector<uint64_t> W, T, terms;
  int rc;
  if ((rc = sequence_weights(c, W))) return rc;  // once per call, not once per range
  std::vector<float> str((size_t)n * n, 0.0f);
  for (uint32_t i = 0; i < n; ++i) str[(size_t)i * n + i] = 1.0f;
  const std::function<int(const mp_store&)> per_range = [&](const mp_store& st) {
    const int r = score_store(c, st, T, terms);
    if (r) return r;
    for (uint64_t p = 0; p < st.n_tasks; ++p) {
      const uint32_t x = st.pair_x[p], y = st.pair_y[p];
      str[(size_t)x * n + y] = str[(size_t)y * n + x] = dafs_host_structure_score(T[p], W[x], W[y]);
    }
    return (int)DAFS_HIP_OK;
  };
  if ((rc = dafs_similarity_pass(c, model, th, max_bytes, n_ranges_out, &per_range))) return rc;
  // the pass left the sequence matrix in the similarity block: keep it, and put the chosen matrix in its place
  c->pair_seq = c->sim;
  c->pair_str.swap(str);
  if (kind == DAFS_SCORE_STRUCTURE) {
    c->sim = c->pair_str;
  } else {
    for (uint32_t x = 0; x < n; ++x)
      for (uint32_t y = 0; y < n; ++y)
        if (x != y) c->sim[(size_t)x * n + y] = dafs_host_mix_score(c->pair_seq[(size_t)x * n + y], c->pair_str[(size_t)x * n + y], weight);
  }
  if ((rc = c->d_sim.upload(c->sim.data(), c->sim.size(), c->stream))) {
    c->sim.clear(); c->pair_seq.clear(); c->pair_str.clear();
    return rc;
  }
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_get_pair_scores(dafs_hip_ctx* c, float* seq, float* str) {
  if (!c || c->pair_seq.empty()) return refuse("get_pair_scores: no dafs_hip_similarity_scored pass with a structural kind since the sequences were set");
  if (seq) memcpy(seq, c->pair_seq.data(), c->pair_seq.size() * sizeof(float));
  if (str) memcpy(str, c->pair_str.data(), c->pair_str.size() * sizeof(float));
  return DAFS_HIP_OK;
}
