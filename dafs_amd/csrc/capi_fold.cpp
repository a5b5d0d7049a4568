// dafs_amd/csrc/capi_fold.cpp -- L1: base-pairing posteriors with the CONTRAfold model
// (Fold::Model::calculate, reference src/fold.cpp:60-68, 174-207).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/dafs_hip.h"
#include "contrafold.h"
#include "contrafold_params.h"
#include "ctx.h"
#include "hip_util.h"
#include "last_error.h"

namespace dafs {

// LoadValues + InitializeCache (reference src/contrafold/InferenceEngine.ipp:1385-1397, 1106-1335):
// prefix sums of the *_at_least families, in float, in the reference's order.
void contrafold_default_params(cf_params* p) {
  memcpy(p->base_pair, cf_base_pair, sizeof p->base_pair);
  memcpy(p->terminal_mismatch, cf_terminal_mismatch, sizeof p->terminal_mismatch);
  memcpy(p->helix_stacking, cf_helix_stacking, sizeof p->helix_stacking);
  memcpy(p->helix_closing, cf_helix_closing, sizeof p->helix_closing);
  memcpy(p->dangle_left, cf_dangle_left, sizeof p->dangle_left);
  memcpy(p->dangle_right, cf_dangle_right, sizeof p->dangle_right);
  memcpy(p->bulge_0x1, cf_bulge_0x1_nucleotides, sizeof p->bulge_0x1);
  memcpy(p->bulge_1x0, cf_bulge_1x0_nucleotides, sizeof p->bulge_1x0);
  memcpy(p->internal_1x1, cf_internal_1x1_nucleotides, sizeof p->internal_1x1);
  p->multi_base = cf_multi_base; p->multi_unpaired = cf_multi_unpaired; p->multi_paired = cf_multi_paired;
  p->external_unpaired = cf_external_unpaired; p->external_paired = cf_external_paired;
  p->cache_hairpin[0] = cf_hairpin_length_at_least[0];
  for (int i = 1; i <= 30; i++) p->cache_hairpin[i] = p->cache_hairpin[i - 1] + cf_hairpin_length_at_least[i];
  float bulge[31], internal[31], sym[16], asym[29];
  bulge[0] = cf_bulge_length_at_least[0];
  for (int i = 1; i <= 30; i++) bulge[i] = bulge[i - 1] + cf_bulge_length_at_least[i];
  internal[0] = cf_internal_length_at_least[0];
  for (int i = 1; i <= 30; i++) internal[i] = internal[i - 1] + cf_internal_length_at_least[i];
  sym[0] = cf_internal_symmetric_length_at_least[0];
  for (int i = 1; i <= 15; i++) sym[i] = sym[i - 1] + cf_internal_symmetric_length_at_least[i];
  asym[0] = cf_internal_asymmetry_at_least[0];
  for (int i = 1; i <= 28; i++) asym[i] = asym[i - 1] + cf_internal_asymmetry_at_least[i];
  for (int l1 = 0; l1 <= 30; l1++)
    for (int l2 = 0; l2 <= 30; l2++) {
      float v = 0.0f;
      if (l1 + l2 <= 30 && !(l1 == 0 && l2 == 0)) {
        if (l1 == 0 || l2 == 0) {
          v += bulge[std::min(30, l1 + l2)];
        } else {
          if (l1 <= 4 && l2 <= 4) v += cf_internal_explicit[l1][l2];
          v += internal[std::min(30, l1 + l2)];
          if (l1 == l2) v += sym[std::min(15, l1)];
          v += asym[std::min(28, l1 > l2 ? l1 - l2 : l2 - l1)];
        }
      }
      p->cache_single[l1 * 31 + l2] = v;
    }
}

}  // namespace dafs

using namespace dafs;

namespace {

// SStruct::ConvertParensToMapping (reference src/contrafold/SStruct.cpp:389-417; '-' reads as '.').  why (optional): what was
// wrong with a refused string.
int parse_constraint(const char* cons, uint32_t L, std::vector<int>& map, const char** why = nullptr) {
  const char* dummy;
  if (!why) why = &dummy;
  map.assign(L + 1, -1);
  std::vector<int> stack;
  for (uint32_t i = 1; i <= L; ++i) {
    const char ch = cons[i - 1];
    if (ch == '?') continue;
    if (ch == '.' || ch == '-') map[i] = 0;
    else if (ch == '(') stack.push_back((int)i);
    else if (ch == ')') {
      if (stack.empty()) { *why = "unbalanced brackets"; return DAFS_HIP_EINVAL; }
      map[i] = stack.back();
      map[stack.back()] = (int)i;
      stack.pop_back();
    } else { *why = "a character that is none of \"?.()\""; return DAFS_HIP_EINVAL; }
  }
  if (!stack.empty()) *why = "unbalanced brackets";
  return stack.empty() ? DAFS_HIP_OK : DAFS_HIP_EINVAL;
}

struct fold_job {
  std::vector<cf_seq> seqs;
  uint64_t iws = 0, fws = 0, post = 0;
  void add(uint32_t len, uint32_t code_off, bool has_cons, uint32_t cons_off) {
    cf_seq s;
    memset(&s, 0, sizeof s);
    s.len = len; s.code_off = code_off; s.has_constraint = has_cons ? 1u : 0u; s.cons_off = cons_off;
    const uint64_t S = (uint64_t)(len + 1) * (len + 2) / 2;
    s.iws_off = iws; iws += 12ull * (len + 2);
    s.fws_off = fws; fws += 7 * S + 2ull * (len + 1);
    s.post_off = post; post += S;
    seqs.push_back(s);
  }
};

int ensure_params(dafs_hip_ctx* c, hipStream_t st) {
  if (c->cf_params_ready) return DAFS_HIP_OK;
  cf_params p;
  contrafold_default_params(&p);
  int rc = c->d_cf_params.upload((const uint8_t*)&p, sizeof p, st);
  if (rc) return rc;
  c->cf_params_ready = true;
  return DAFS_HIP_OK;
}

int run_job(dafs_hip_ctx* c, const fold_job& job, const uint8_t* d_codes, const int* d_cons, cf_batch* out, hipStream_t st) {
  int rc;
  if ((rc = ensure_params(c, st))) return rc;
  if ((rc = c->cf_seqs.upload((const uint8_t*)job.seqs.data(), job.seqs.size() * sizeof(cf_seq), st))) return rc;
  if ((rc = c->cf_iws.reserve(job.iws))) return rc;
  if ((rc = c->cf_fws.reserve(job.fws))) return rc;
  if ((rc = c->cf_post.reserve(job.post))) return rc;
  if ((rc = c->cf_logz.reserve(job.seqs.size()))) return rc;
  cf_batch B;
  B.params = (const cf_params*)c->d_cf_params.ptr;
  B.seqs = (const cf_seq*)c->cf_seqs.ptr;
  B.codes = d_codes;
  B.cons = d_cons;
  B.iws = c->cf_iws.ptr;
  B.fws = c->cf_fws.ptr;
  B.post = c->cf_post.ptr;
  B.logz = c->cf_logz.ptr;
  B.stamps = nullptr;
  if (getenv("DAFS_HIP_CF_STAMPS")) {
    if ((rc = c->cf_stamps.reserve(8))) return rc;
    B.stamps = c->cf_stamps.ptr;
  }
  *out = B;
  uint32_t max_len = 0;
  for (const cf_seq& q : job.seqs) max_len = std::max(max_len, q.len);
  rc = contrafold_launch(B, (uint32_t)job.seqs.size(), max_len, st);
  if (!rc && B.stamps) {
    unsigned long long h[8] = {0};
    if (!hip_check(hipMemcpy(h, B.stamps, sizeof h, hipMemcpyDeviceToHost)))
      fprintf(stderr, "k_contrafold block 0 (us): inside %.0f (terms %.0f) | F5i %.0f | F5o %.0f | outside %.0f (terms %.0f)\n", (h[1] - h[0]) / 100.0,
              h[5] / 100.0, (h[2] - h[1]) / 100.0, (h[3] - h[2]) / 100.0, (h[4] - h[3]) / 100.0, h[6] / 100.0);
  }
  return rc;
}

// The posteriors of a finished job of n sequences compacted with threshold th into st (rows with p > th), whose row pointers
// lie at rp_off[0..n]; the entry arrays start at 8 entries per residue and grow when the kernel reports an overflow.
// first (optional; a job of several folds per sequence): sequence x owns the folds first[x] .. first[x + 1],
// and k_bp_compact_levels merges them; nullptr: one fold per sequence, k_bp_compact.
int compact_job(dafs_hip_ctx* c, const cf_batch& B, uint32_t n, float th, const uint64_t* rp_off, uint64_t residues, bp_store& st,
                const uint32_t* first = nullptr) {
  int rc;
  if (first && (rc = c->cf_first.upload(first, n + 1, c->stream))) return rc;
  if ((rc = st.rowptr.reserve(rp_off[n]))) return rc;
  if ((rc = st.nnz.reserve(n))) return rc;
  if ((rc = st.bp_off.reserve(n + 1))) return rc;
  if ((rc = st.rp_off.upload(rp_off, n + 1, c->stream))) return rc;
  if ((rc = c->counters.reserve(4))) return rc;
  uint64_t cap = 8ull * residues + 1024;
  for (int attempt = 0;; ++attempt) {
    if ((rc = st.col.reserve(cap))) return rc;
    if ((rc = st.val.reserve(cap))) return rc;
    if (hip_check(hipMemsetAsync(c->counters.ptr, 0, 4 * sizeof(unsigned long long), c->stream))) return DAFS_HIP_ELAUNCH;
    rc = first ? bp_compact_levels_launch(B, n, th, c->cf_first.ptr, st.rp_off.ptr, st.rowptr.ptr, st.col.ptr, st.val.ptr, st.bp_off.ptr, st.nnz.ptr,
                                          c->counters.ptr, cap, (int*)(c->counters.ptr + 2), c->stream)
               : bp_compact_launch(B, n, th, st.rp_off.ptr, st.rowptr.ptr, st.col.ptr, st.val.ptr, st.bp_off.ptr, st.nnz.ptr, c->counters.ptr, cap,
                                   (int*)(c->counters.ptr + 2), c->stream);
    if (rc) return rc;
    unsigned long long h[4];
    if (hip_check(hipMemcpyAsync(h, c->counters.ptr, sizeof h, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
    if (hip_check(hipStreamSynchronize(c->stream))) return DAFS_HIP_ELAUNCH;
    const int status = (int)(h[2] & 0xffffffffu);
    if (status == 0) { st.total_nnz = h[0]; st.valid = true; return DAFS_HIP_OK; }
    if (status != DAFS_HIP_EOVERFLOW || attempt >= 4) return status;
    cap = std::max<uint64_t>(h[0], cap * 2);
  }
}

// One fold of the context's sequence x into the job: under con (nullptr or empty: free), whose map joins maps.  A refused
// string leaves the reason in *why.  check_pairs: a forced pair must be one CONTRAfold can form.
int add_fold(const dafs_hip_ctx* c, uint32_t x, const char* con, bool check_pairs, fold_job& job, std::vector<int>& maps, const char** why) {
  if (x >= c->len.size()) { *why = "an unknown sequence"; return DAFS_HIP_EINVAL; }
  const uint32_t L = c->len[x];
  if (!con || !con[0]) {  // empty = unconstrained (wrapper.cpp:188)
    job.add(L, c->off[x], false, 0);
    return DAFS_HIP_OK;
  }
  if (strnlen(con, L) < L) { *why = "a constraint shorter than its sequence"; return DAFS_HIP_EINVAL; }
  std::vector<int> one;
  const int rc = parse_constraint(con, L, one, why);
  if (rc) return rc;
  for (uint32_t i = 1; check_pairs && i <= L; ++i)
    if (one[i] > (int)i && !dafs_host_fold_complementary(c->seq[c->off[x] + i - 1], c->seq[c->off[x] + one[i] - 1])) {
      *why = "a forced pair of residues that CONTRAfold cannot pair";
      return DAFS_HIP_EINVAL;
    }
  job.add(L, c->off[x], true, (uint32_t)maps.size());
  maps.insert(maps.end(), one.begin(), one.end());
  return DAFS_HIP_OK;
}

// The job of folding the context's sequences seq[0..n) (seq nullptr: 0 .. n-1), sequence r under cons[r] (nullptr or empty:
// free), and the constraint maps of the constrained ones one after another.  A refused string leaves its row in *bad and the
// reason in *why.  check_pairs: a forced pair must be one CONTRAfold can form.
int make_job(const dafs_hip_ctx* c, uint32_t n, const uint32_t* seq, const char* const* cons, bool check_pairs, fold_job& job,
             std::vector<int>& maps, uint32_t* bad, const char** why) {
  for (uint32_t r = 0; r < n; ++r) {
    *bad = r;
    const int rc = add_fold(c, seq ? seq[r] : r, cons ? cons[r] : nullptr, check_pairs, job, maps, why);
    if (rc) return rc;
  }
  return DAFS_HIP_OK;
}

// the job in flight on the folding stream: _end compacts it
void fold_started(dafs_hip_ctx* c, const cf_batch& B, float th) {
  c->fold_batch.assign((const uint8_t*)&B, (const uint8_t*)&B + sizeof B);
  c->fold_pending = true;
  c->fold_th = th;
  c->bp[0].valid = false;
  c->bp[1].valid = false;
  c->cur_bp = 0;
}

}  // namespace

// Batch hook: Fold::Model::calculate(const vector<Fasta>&, vector<BP>&) for -s CONTRAfold, each sequence free or under a
// constraint string of its own (Fold::Model::calculate(seq, str, bp), fold.cpp:191-207).
// Result: the context's un-relaxed base-pairing store (rows with p > th; reference CUTOFF 0.01).
// _begin enqueues the inside/outside/posterior kernels on the context's folding stream and returns; the pair
// posteriors and the matching-probability transform do not depend on them and may run meanwhile.  _end waits
// for the kernels and compacts the posteriors into the store.
extern "C" int dafs_hip_fold_posteriors_constrained_begin(dafs_hip_ctx* c, int model, float th, const char* const* constraints) {
  if (!c || c->len.empty() || model != DAFS_FOLD_CONTRAFOLD) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  if (c->fold_pending) return DAFS_HIP_EINVAL;
  const uint32_t n = (uint32_t)c->len.size();
  fold_job job;
  std::vector<int> maps;
  uint32_t bad = 0;
  const char* why = "";
  int rc = make_job(c, n, nullptr, constraints, true, job, maps, &bad, &why);
  if (rc) {
    set_last_error(("fold constraints: sequence " + std::to_string(bad) + ": " + why).c_str());
    return rc;
  }
  // the maps travel on the folding stream, in front of the kernels that read them (upload waits for the copy)
  if (!maps.empty() && (rc = c->cf_cons.upload(maps.data(), maps.size(), c->fold_stream))) return rc;
  cf_batch B;
  rc = run_job(c, job, c->codes.ptr, maps.empty() ? nullptr : c->cf_cons.ptr, &B, c->fold_stream);
  if (rc) return rc;
  c->fold_first.clear();
  fold_started(c, B, th);
  return DAFS_HIP_OK;
}

// Several folds per sequence in one batch (DAFS::update_basepairing_probability, dafs.cpp:635-661, folds
// a row once per level): the folds of sequence x lie one after another in the job and share its codes; _end merges them.
extern "C" int dafs_hip_fold_posteriors_levels_begin(dafs_hip_ctx* c, int model, float th, uint32_t nlevels, const char* const* constraints) {
  if (!c || c->len.empty() || model != DAFS_FOLD_CONTRAFOLD) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  if (c->fold_pending) return DAFS_HIP_EINVAL;
  if (nlevels < 1 || nlevels > DAFS_HIP_MAX_LEVELS) {
    set_last_error(("fold constraints: " + std::to_string(nlevels) + " levels; a sequence has 1 to " + std::to_string(DAFS_HIP_MAX_LEVELS)).c_str());
    return DAFS_HIP_EINVAL;
  }
  const uint32_t n = (uint32_t)c->len.size();
  fold_job job;
  std::vector<int> maps;
  std::vector<uint32_t> first(n + 1, 0);
  int rc;
  for (uint32_t x = 0; x < n; ++x) {
    first[x] = (uint32_t)job.seqs.size();
    for (uint32_t k = 0; constraints && k < nlevels; ++k) {
      const char* con = constraints[(size_t)x * nlevels + k];
      if (!con || !con[0]) continue;  // no fold of x at level k
      const char* why = "";
      if ((rc = add_fold(c, x, con, true, job, maps, &why))) {
        set_last_error(("fold constraints: sequence " + std::to_string(x) + ", level " + std::to_string(k) + ": " + why).c_str());
        return rc;
      }
    }
    if (job.seqs.size() == first[x]) job.add(c->len[x], c->off[x], false, 0);  // no string at all: once, free
  }
  first[n] = (uint32_t)job.seqs.size();
  if (!maps.empty() && (rc = c->cf_cons.upload(maps.data(), maps.size(), c->fold_stream))) return rc;
  cf_batch B;
  if ((rc = run_job(c, job, c->codes.ptr, maps.empty() ? nullptr : c->cf_cons.ptr, &B, c->fold_stream))) return rc;
  c->fold_first.swap(first);
  fold_started(c, B, th);
  return DAFS_HIP_OK;
}

extern "C" int dafs_hip_fold_posteriors_levels(dafs_hip_ctx* c, int model, float th, uint32_t nlevels, const char* const* constraints) {
  const int rc = dafs_hip_fold_posteriors_levels_begin(c, model, th, nlevels, constraints);
  return rc ? rc : dafs_hip_fold_posteriors_end(c);
}

extern "C" int dafs_hip_fold_posteriors_begin(dafs_hip_ctx* c, int model, float th) {
  return dafs_hip_fold_posteriors_constrained_begin(c, model, th, nullptr);
}

extern "C" int dafs_hip_fold_posteriors_end(dafs_hip_ctx* c) {
  if (!c || !c->fold_pending || c->fold_batch.size() != sizeof(cf_batch)) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  c->fold_pending = false;
  if (hip_check(hipStreamSynchronize(c->fold_stream))) return DAFS_HIP_ELAUNCH;
  cf_batch B;
  memcpy(&B, c->fold_batch.data(), sizeof B);
  const uint32_t n = (uint32_t)c->len.size();
  return compact_job(c, B, n, c->fold_th, c->seq_rp_off.data(), c->off[n], c->bp[0], c->fold_first.empty() ? nullptr : c->fold_first.data());
}

extern "C" int dafs_hip_fold_posteriors_constrained(dafs_hip_ctx* c, int model, float th, const char* const* constraints) {
  const int rc = dafs_hip_fold_posteriors_constrained_begin(c, model, th, constraints);
  return rc ? rc : dafs_hip_fold_posteriors_end(c);
}

extern "C" int dafs_hip_fold_posteriors(dafs_hip_ctx* c, int model, float th) {
  return dafs_hip_fold_posteriors_constrained(c, model, th, nullptr);
}

// Constrained posteriors of the rows of one alignment (DAFS::update_basepairing_probability, dafs.cpp:657-663: one
// s_model_->calculate(seq, con, bp) per sequence), as one batch; the result is a store whose index is the row.
int dafs_fold_rows_constrained(dafs_hip_ctx* c, uint32_t n, const uint32_t* seq, const std::vector<std::string>& cons, float th, dafs::bp_store& st) {
  if (!c || !n || !seq || cons.size() != n || c->fold_pending) return DAFS_HIP_EINVAL;
  st.valid = false;
  fold_job job;
  std::vector<int> maps;
  std::vector<const char*> strs(n);
  std::vector<uint64_t> rp_off(n + 1, 0);
  uint64_t residues = 0;
  for (uint32_t r = 0; r < n; ++r) {
    if (seq[r] >= c->len.size() || cons[r].empty()) return DAFS_HIP_EINVAL;  // every row is constrained here
    strs[r] = cons[r].c_str();
    rp_off[r + 1] = rp_off[r] + c->len[seq[r]] + 1;
    residues += c->len[seq[r]];
  }
  uint32_t bad = 0;
  const char* why = "";
  int rc = make_job(c, n, seq, strs.data(), false, job, maps, &bad, &why);
  if (rc) return rc;
  if ((rc = c->cf_cons.upload(maps.data(), maps.size(), c->stream))) return rc;
  cf_batch B;
  if ((rc = run_job(c, job, c->codes.ptr, c->cf_cons.ptr, &B, c->stream))) return rc;
  return compact_job(c, B, n, th, rp_off.data(), residues, st);
}

// Single-sequence plugin call: CONTRAfold<float>::ComputePosterior (reference
// src/contrafold/wrapper.cpp:181-200), optionally under a constraint string of len chars from
// "?.()" (Fold::Model::calculate(seq, str, bp), src/fold.cpp:191-207).  post receives the
// (len+1)(len+2)/2 triangular posteriors in the reference's layout.
extern "C" int dafs_hip_fold_posterior_dense(dafs_hip_ctx* c, const char* seq, uint32_t len, const char* constraint, float* post,
                                             float* logz) {
  if (!c || !seq || !len || !post) return DAFS_HIP_EINVAL;
  if (hip_check(hipSetDevice(c->device))) return DAFS_HIP_ENODEV;
  if (constraint && !constraint[0]) constraint = nullptr;  // empty = unconstrained (wrapper.cpp:188)
  std::vector<uint8_t> codes(len);
  for (uint32_t i = 0; i < len; ++i) codes[i] = dafs_hip_residue_code(seq[i]);
  std::vector<int> map;
  if (constraint) {
    if (strlen(constraint) < len) return DAFS_HIP_EINVAL;
    int rc = parse_constraint(constraint, len, map);
    if (rc) return rc;
  }
  int rc;
  if ((rc = c->cf_codes.upload(codes.data(), len, c->stream))) return rc;
  if (constraint && (rc = c->cf_cons.upload(map.data(), map.size(), c->stream))) return rc;
  fold_job job;
  job.add(len, 0, constraint != nullptr, 0);
  cf_batch B;
  if (c->fold_pending) return DAFS_HIP_EINVAL;  // the batch in flight owns the folding workspaces
  if ((rc = run_job(c, job, c->cf_codes.ptr, constraint ? c->cf_cons.ptr : nullptr, &B, c->stream))) return rc;
  const uint64_t S = (uint64_t)(len + 1) * (len + 2) / 2;
  if (hip_check(hipMemcpyAsync(post, B.post, S * 4, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
  float z = 0;
  if (hip_check(hipMemcpyAsync(&z, B.logz, 4, hipMemcpyDeviceToHost, c->stream))) return DAFS_HIP_ELAUNCH;
  if (hip_check(hipStreamSynchronize(c->stream))) return DAFS_HIP_ELAUNCH;
  if (logz) *logz = z;
  return DAFS_HIP_OK;
}
