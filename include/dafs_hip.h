/* include/dafs_hip.h -- C ABI of libdafs_hip.so, the MI355X (gfx950) implementation of the
 * DAFS probability-matrix + dual-decomposition hot path.
 *
 * Two layers, both plain C (pointers + sizes, no C++/torch types):
 *
 *  L1 "plugin" entry points (dafs_hip_*): host buffers in, host buffers out.  These are what the
 *     reference's four plugin interfaces would bind (reference src/align.h:34-66,
 *     src/fold.h:30-61) -- see INTEGRATION.md for the C++ shim a DAFS maintainer would add.
 *     They own their device workspace and synchronise before returning.
 *
 *  L0 "launch" entry points (dafs_hipk_*): device pointers + a HIP stream, no allocation, no
 *     synchronisation.  Used by L1 and by callers that keep data resident in HBM (bench.py
 *     allocates with torch and passes tensor.data_ptr()).
 *
 * All functions return 0 on success or a negative DAFS_HIP_E* code; no exception crosses the
 * ABI.  dafs_hip_strerror() gives the message the C++ shim throws as `const char*`, the
 * reference's error convention (reference src/dafs.cpp:1893-1910).
 * Indices are uint32; "none" is 0xFFFFFFFF (the reference's -1u, src/nussinov.cpp:267).
 */
#ifndef DAFS_HIP_H
#define DAFS_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DAFS_HIP_NONE 0xFFFFFFFFu

enum {
  DAFS_HIP_OK = 0,
  DAFS_HIP_EINVAL = -1,    /* bad argument (NULL, empty sequence, unknown model) */
  DAFS_HIP_ENODEV = -2,    /* no usable HIP device / HIP runtime error */
  DAFS_HIP_ENOMEM = -3,    /* device or host allocation failed */
  DAFS_HIP_ETOOLONG = -4,  /* sequence longer than the kernels support */
  DAFS_HIP_EOVERFLOW = -5, /* sparse output pool too small (retry with a larger pool) */
  DAFS_HIP_ELAUNCH = -6,   /* kernel launch / execution failure */
  DAFS_HIP_ECOMM = -7      /* the caller's collective (dafs_allgather_fn) reported a failure */
};
const char* dafs_hip_strerror(int code);
/* last HIP runtime error text seen by this thread (diagnostics), or the message of the last refusal of a host text function */
const char* dafs_hip_last_error(void);

/* Alignment models: reference -a ProbCons | CONTRAlign (src/dafs.cpp:1683-1690) */
enum { DAFS_ALIGN_PROBCONS = 0, DAFS_ALIGN_CONTRALIGN = 1 };
/* Folding models: reference -s CONTRAfold (src/dafs.cpp:1703).  Boltzmann/Vienna need
 * ViennaRNA arithmetic that is not in the reference tree: not provided. */
enum { DAFS_FOLD_CONTRAFOLD = 0 };

/* ------------------------------------------------------------------------------------------
 * L0: pair-HMM posterior kernel (ProbCons 3-state model)
 * Replaces, per pair: PROBCONS::Probcons::ComputePosterior (src/probconsRNA/wrapper.cpp:101-131)
 * + ProbCons::calculate's dense->sparse step (src/align.cpp:60-79) + transpose_mp
 * (src/dafs.cpp:155-167) + calculate_similarity_score (src/dafs.cpp:713-764).
 * ---------------------------------------------------------------------------------------- */

/* One pair job: offsets/lengths of the two residue-code strings inside `codes`. */
typedef struct {
  uint32_t off1, len1; /* sequence x (rows)    */
  uint32_t off2, len2; /* sequence y (columns) */
} dafs_pair_task;

/* Launch geometry chosen by dafs_hipk_pairhmm_plan for a batch.  A caller may lower nwaves to any positive multiple
 * of 4 before the launch: the wavefronts are persistent and then take more batches of 64/group pairs each, on the
 * first nwaves regions of the same scratch.  The launches return DAFS_HIP_EINVAL for nwaves == 0, for nwaves % 4 != 0
 * and for an nwaves whose scratch (nwaves * slab_steps * width * 64 * 4 bytes * planes; 2 planes ProbCons, 5
 * CONTRAlign) scratch_bytes does not cover.  The scratch may hold anything when a launch starts. */
typedef struct {
  uint32_t group;        /* lanes cooperating on one pair: 16, 32 or 64           */
  uint32_t width;        /* columns owned by each lane                              */
  uint32_t nwaves;       /* persistent wavefronts launched (4 per workgroup)        */
  uint32_t slab_steps;   /* wavefront steps one slab holds = max(len1)+group        */
  uint64_t scratch_bytes;/* bytes of `scratch` the launch needs                     */
} dafs_pairhmm_plan;

/* 7 residue classes: A C G U T N other ('other' includes the reference's '~' sentinel). */
typedef struct {
  float init[3];     /* log initial distribution M, X, Y   (Defaults.h:19)                  */
  float trans[3][3]; /* log transition [from][to]          (ProbabilisticModel.h:59-79)     */
  float match[7][8]; /* log pair emission, row stride 8    (Defaults.h:30-37)               */
  float ins[8];      /* log single emission                (Defaults.h:26-28)               */
} dafs_pairhmm3_model;

typedef struct {
  const uint8_t* codes;        /* [device] residue class codes 0..6, all sequences concatenated */
  const dafs_pair_task* tasks; /* [device] ntasks jobs, in processing order (longest first)      */
  uint32_t ntasks;
  float th;                    /* keep posterior > th (reference -u, default 0.01)               */
  float* scratch;              /* [device] plan.scratch_bytes                                     */
  uint32_t* queue;             /* [device] one zeroed uint32: dynamic work counter                */
  /* outputs, all [device].  Pair t owns rowptr_pool[rp_off[t] .. +len1+1) (row pointers of
   * mp[x][y], relative to the pair's base) followed by len2+1 row pointers of mp[y][x];
   * entries live at ent_col/ent_val[pair_off[t] .. +nnz) (mp[x][y], rows ascending, columns
   * ascending) and [pair_off[t]+nnz .. +2nnz) (mp[y][x]).  pair_off is assigned by a device-side
   * bump allocator on *pool_top, so pool order is unspecified; contents are deterministic. */
  const uint64_t* rp_off;
  uint32_t* rowptr_pool;
  uint32_t* ent_col;
  float* ent_val;
  unsigned long long* pool_top; /* zeroed before launch */
  uint64_t pool_cap;            /* capacity of ent_col/ent_val in entries */
  uint64_t* pair_off;
  uint32_t* pair_nnz;
  float* sim;                   /* similarity score per task (dafs.cpp:763) */
  int* status;                  /* zeroed; set to DAFS_HIP_EOVERFLOW when the pool is exhausted */
  dafs_pairhmm3_model model;
} dafs_pairhmm3_args;

int dafs_hipk_pairhmm_plan(uint32_t ntasks, uint32_t max_len1, uint32_t max_len2, dafs_pairhmm_plan* plan);
int dafs_hipk_pairhmm3_launch(const dafs_pairhmm3_args* args, const dafs_pairhmm_plan* plan, void* hip_stream);
/* The cut of the launch's candidate pick: a value c <= -0.5 such that every float v with -16 < v < c has EXP(v) <= th
 * (EXP: ScoreType.h:37-57), i.e. no cell whose log posterior lies below c can be an entry.  Host arithmetic only. */
float dafs_hip_pair_cut(float th);
/* Host-side model tables: log of the ProbCons defaults, computed with logf like the reference
 * constructor (ProbabilisticModel.h:55-88). */
void dafs_hip_pairhmm3_default_model(dafs_pairhmm3_model* m);
/* residue byte -> class code (wrapper.cpp:157-170: case-insensitive "ACGUTN", else 'other') */
uint8_t dafs_hip_residue_code(char c);

/* ------------------------------------------------------------------------------------------
 * L0: pair-CRF posterior kernel (CONTRAlign 5-state model).
 * Replaces, per pair: CONTRALIGN::CONTRAlign<float>::ComputePosterior
 * (src/contralign/wrapper.cpp:81-97) + CONTRAlign::calculate's dense->sparse step
 * (src/align.cpp:87-106) + transpose_mp + calculate_similarity_score.  Same argument layout and
 * outputs as the ProbCons kernel; the scratch holds five planes (dafs_hipk_pairhmm5_plan).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  float match[5][5]; /* symbol 0..3 = A C G U, 4 = anything else (scores 0), Defaults.ipp:393-402 */
  float insert[5];   /* Defaults.ipp:403-406 */
  float single[5];   /* per state MATCH, INS_X, INS_Y, INS2_X, INS2_Y, Defaults.ipp:407-409 */
  float pair[5][5];  /* transition [from][to], Defaults.ipp:410-416 */
} dafs_pairhmm5_model;

typedef struct {
  const uint8_t* codes;
  const dafs_pair_task* tasks;
  uint32_t ntasks;
  float th;
  float* scratch;
  uint32_t* queue;
  const uint64_t* rp_off;
  uint32_t* rowptr_pool;
  uint32_t* ent_col;
  float* ent_val;
  unsigned long long* pool_top;
  uint64_t pool_cap;
  uint64_t* pair_off;
  uint32_t* pair_nnz;
  float* sim;
  int* status;
  dafs_pairhmm5_model model;
} dafs_pairhmm5_args;

int dafs_hipk_pairhmm5_plan(uint32_t ntasks, uint32_t max_len1, uint32_t max_len2, dafs_pairhmm_plan* plan);
int dafs_hipk_pairhmm5_launch(const dafs_pairhmm5_args* args, const dafs_pairhmm_plan* plan, void* hip_stream);
void dafs_hip_pairhmm5_default_model(dafs_pairhmm5_model* m);

/* ------------------------------------------------------------------------------------------
 * L1: batch alignment-posterior plugin.
 * Replaces Align::Model::calculate(const vector<Fasta>&, vector<vector<MP>>&)
 * (src/align.cpp:35-52) for -a ProbCons / -a CONTRAlign, plus the transposes (src/dafs.cpp:1797-1799) and
 * sim_ (src/dafs.cpp:1813-1819), for the pair-index shard [pair_begin, pair_end) of the
 * row-major (i<j) pair enumeration (pair_end = 0 means all pairs).
 * ---------------------------------------------------------------------------------------- */
typedef struct dafs_hip_ctx dafs_hip_ctx;
int dafs_hip_create(int device, dafs_hip_ctx** ctx);
void dafs_hip_destroy(dafs_hip_ctx* ctx);

int dafs_hip_set_sequences(dafs_hip_ctx* ctx, uint32_t nseq, const char* const* seqs, const uint32_t* lens);
/* Family partition (many independent alignments in one context): family f holds the sequences first[f] .. first[f+1]-1;
 * first[0] = 0, first[nfam] = nseq, strictly increasing (families of one sequence are allowed).  Every stage then works
 * within each family and batches across them: only pairs within a family exist, numbered family by family and row-major
 * inside each (the pair order of dafs_hip_align_posteriors' [pair_begin, pair_end), of the fetches and of the stores); the
 * similarity scores are one n_f x n_f block per family (dafs_hip_get_sim); the consistency transforms sum over the output
 * pair's family with its size in the weights; a progressive node whose rows span two families is refused (EINVAL).
 * Call after dafs_hip_set_sequences (which sets one family of all sequences); it invalidates the stores.
 * dafs_hip_set_mp, dafs_hip_mp_install, dafs_hip_mp_install_dev and dafs_hip_phase1_sharded need a single family. */
int dafs_hip_set_families(dafs_hip_ctx* ctx, uint32_t nfam, const uint32_t* first);
int dafs_hip_align_posteriors(dafs_hip_ctx* ctx, int model, float th, uint64_t pair_begin, uint64_t pair_end);
/* sizes of the result held in the context */
int dafs_hip_align_result_size(dafs_hip_ctx* ctx, uint64_t* npairs, uint64_t* total_nnz, uint64_t* total_rowptr);
/* Copy out, pairs in shard order p = pair_begin..: pair_x/pair_y[npairs]; sim[npairs];
 * nnz[npairs]; rowptr: for each pair len_x+1 entries (relative) then len_y+1 (transposed);
 * col/val: for each pair nnz entries of mp[x][y] then nnz of mp[y][x]. Any pointer may be NULL. */
int dafs_hip_align_fetch(dafs_hip_ctx* ctx, uint32_t* pair_x, uint32_t* pair_y, float* sim, uint32_t* nnz,
                         uint32_t* rowptr, uint32_t* col, float* val);

/* Generic access to the matching-probability stores: relaxed = 0 as computed by the alignment
 * model, 1 after dafs_hip_consistency (layout as dafs_hip_align_fetch). */
int dafs_hip_mp_result_size(dafs_hip_ctx* ctx, int relaxed, uint64_t* npairs, uint64_t* total_nnz, uint64_t* total_rowptr);
int dafs_hip_mp_fetch(dafs_hip_ctx* ctx, int relaxed, uint32_t* pair_x, uint32_t* pair_y, uint32_t* nnz,
                      uint32_t* rowptr, uint32_t* col, float* val);
/* Supplied matching probabilities instead of a model: AUXAlign::calculate (src/align.cpp:204-246, --align-aux), and
 * the hand-over after an all-gather of shards.  For every pair x < y in row-major order: nnz[p] entries, len[x]+1 row
 * pointers relative to the pair's first entry (concatenated), then all (col ascending within a row, val) entries
 * concatenated.  Lays out the transposes (transpose_mp, src/dafs.cpp:155-167) and computes the similarity scores
 * (calculate_similarity_score, :713-764) on the device. */
int dafs_hip_set_mp(dafs_hip_ctx* ctx, const uint32_t* nnz, const uint32_t* rowptr, const uint32_t* col, const float* val);
/* A whole store from arrays in the layout of dafs_hip_mp_fetch / dafs_hip_align_fetch (both directions of every pair; no
 * recomputation, uploads only): how the ranks of a multi-GPU run take their gathered shards back in.  relaxed = 0: the
 * models' posteriors, with sim[npairs] = the similarity score of every pair (src/dafs.cpp:763) as the shard kernels
 * computed them; relaxed = 1: the consistency transform's result, on top of an un-relaxed store (sim may be NULL). */
int dafs_hip_mp_install(dafs_hip_ctx* ctx, int relaxed, const uint32_t* nnz, const uint32_t* rowptr, const uint32_t* col,
                        const float* val, const float* sim);
/* sim_ (src/dafs.cpp:1813-1819): N*N floats, unit diagonal -- with families, the n_f*n_f blocks one after another; needs a
 * full-pair-set align_posteriors, dafs_hip_set_mp or dafs_hip_mp_install. */
int dafs_hip_get_sim(dafs_hip_ctx* ctx, float* sim);
/* The similarity scores of a set too large to hold all its posteriors at once (dafs --cluster, pipeline.cluster; DESIGN.md
 * section 20).  On a one-family context of N >= 2 sequences (after dafs_hip_set_sequences) the row-major pair enumeration is
 * walked in the ranges of dafs_host_similarity_ranges(N, lens, max_bytes): each range is one dafs_hip_align_posteriors launch
 * into the context's buffers, which the next range reuses, and its scores go into the similarity block.  Afterwards
 * dafs_hip_get_sim returns, bit for bit, what it returns after a full-pair-set dafs_hip_align_posteriors, whatever the
 * budget; both matching stores are marked invalid in every case, also when one range held every pair, so that no caller comes
 * to depend on the budget (a transform or a fetch is refused, DAFS_HIP_EINVAL).  max_bytes = 0: dafs_host_batch_bytes().
 * n_ranges_out (may be NULL): the launches made.  DAFS_HIP_EINVAL: more than one family, fewer than two sequences, an unknown
 * model, th < 0; DAFS_HIP_ETOOLONG as dafs_hip_align_posteriors. */
int dafs_hip_similarity(dafs_hip_ctx* ctx, int model, float th, uint64_t max_bytes, uint64_t* n_ranges_out);
/* Host-side helper (no device work): the ranges dafs_hip_similarity walks for n sequences of lengths lens.  The pairs x < y, in
 * row-major order, are packed greedily under max_bytes (0: dafs_host_batch_bytes()) of estimated device memory; a pair over the
 * budget is a range of its own, and a range holds fewer than 2^32 pairs.  The estimate of a pair is what
 * dafs_hip_align_posteriors starts its entry pool from, 2 * min(len_x, len_y) * 24 entries of 8 bytes (column and value), plus
 * its len_x + 1 + len_y + 1 row pointers of 4 bytes.  The launch's scratch planes depend on the launch plan and not on the
 * number of pairs, and are left out.  *n_ranges: the number of ranges (0 for n < 2); range r is [end[r - 1], end[r]) with
 * end[-1] = 0, and the first min(*n_ranges, cap) entries of end are written (end may be NULL with cap = 0: the count alone). */
int dafs_host_similarity_ranges(uint32_t n, const uint32_t* lens, uint64_t max_bytes, uint64_t* end, uint64_t cap, uint64_t* n_ranges);

/* ------------------------------------------------------------------------------------------
 * L1: the structural pair score (no counterpart in the reference; the contract, to the bit, in DESIGN.md section 24;
 * `dafs --cluster-score`, pipeline.cluster(score=...)).  It is the quantity relax_basepairing_probability sums (reference
 * src/dafs.cpp:349-361) reduced to one scalar per pair and taken on integers, so that no order of summation, lane mapping or
 * range budget changes a bit.  With c(v) the stored float as a double clamped into [0, 1] (NaN: 0), a base pair (i, j, p) of x,
 * a base pair (k, l, q) of y, and the entries (k, a) of row i and (l, b) of row j of mp[x][y]:
 *   term = (uint64) floor(((c(p) * c(q)) * (c(a) * c(b))) * 2^40)      (doubles, this bracketing; only k < l occurs)
 *   T(x, y) = the sum of the terms, terms(x, y) = their number (zero terms counted)
 *   W(x) = the sum over the base pairs of x of (uint64) floor(c(p) * 2^40)
 * ---------------------------------------------------------------------------------------- */
/* T and terms of every pair of the un-relaxed matching store that is valid now, in the pair order of dafs_hip_align_fetch
 * (npairs of dafs_hip_align_result_size entries each), and W of every sequence (nseq entries) from the un-relaxed base-pairing
 * store.  Stores installed with dafs_hip_set_mp / dafs_hip_set_bp count like computed ones.  Any output may be NULL.  Both
 * stores are left as they are.  DAFS_HIP_EINVAL with a message in dafs_hip_last_error: either store missing, several families,
 * no sequences.  DAFS_HIP_EOVERFLOW with a message naming the pair: a pair with 2^24 terms or more (below that T < 2^64 and
 * the sum is exact); nothing is written then. */
int dafs_hip_structure_scores(dafs_hip_ctx* ctx, uint64_t* T, uint64_t* terms, uint64_t* W);
/* The two formulas on the host (no device work), the one copy the library, the tests and both drivers use:
 * (float) min(1.0, (double)T / (double)min(Wx, Wy)), 0.0f when min(Wx, Wy) = 0; and
 * (float)((double)sim + (double)w * ((double)str - (double)sim)). */
float dafs_host_structure_score(uint64_t T, uint64_t Wx, uint64_t Wy);
float dafs_host_mix_score(float sim, float str, float w);
/* dafs_hip_similarity with a choice of score: the same range loop, and for the structural kinds one launch of the scoring
 * kernel over each range while its rows are resident (W once per call).  kind DAFS_SCORE_SEQUENCE is dafs_hip_similarity itself
 * (weight unread, no base-pairing store needed).  DAFS_SCORE_STRUCTURE: struct(x, y) = dafs_host_structure_score(T, W(x), W(y)),
 * unit diagonal.  DAFS_SCORE_MIX: dafs_host_mix_score(sim, struct, weight) per entry, weight in [0, 1].  The chosen matrix is
 * left in the context's similarity block, host and device: dafs_hip_get_sim and dafs_hip_linkage_tree with a NULL matrix see
 * it.  The raw sequence matrix and the structure matrix are kept for dafs_hip_get_pair_scores.  Both matching stores are
 * invalid afterwards, as after dafs_hip_similarity; the base-pairing store stays valid.  DAFS_HIP_EINVAL with a message,
 * the context unchanged and usable: an unknown kind, a weight outside [0, 1] (or NaN) with MIX, and for the structural kinds
 * no valid un-relaxed base-pairing store (dafs_hip_fold_posteriors or dafs_hip_set_bp after dafs_hip_set_sequences), several
 * families, fewer than two sequences.  DAFS_HIP_EOVERFLOW as dafs_hip_structure_scores; otherwise as dafs_hip_similarity. */
enum { DAFS_SCORE_SEQUENCE = 0, DAFS_SCORE_STRUCTURE = 1, DAFS_SCORE_MIX = 2 };
int dafs_hip_similarity_scored(dafs_hip_ctx* ctx, int model, float th, uint64_t max_bytes, int kind, float weight, uint64_t* n_ranges_out);
/* The two n x n matrices of the last dafs_hip_similarity_scored pass with a structural kind: seq is, bit for bit, what
 * dafs_hip_similarity leaves in the similarity block, str the structure matrix.  Either may be NULL.  DAFS_HIP_EINVAL with a
 * message when there was no such pass since dafs_hip_set_sequences (a later dafs_hip_similarity forgets them too). */
int dafs_hip_get_pair_scores(dafs_hip_ctx* ctx, float* seq, float* str);

/* ------------------------------------------------------------------------------------------
 * L1: base-pairing probabilities.
 * dafs_hip_set_bp replaces AUXFold::calculate (src/fold.cpp:261-278, --fold-aux): the caller
 * supplies BP rows.  rowptr: per sequence len+1 entries relative to that sequence's first entry,
 * concatenated in input order; col/val: entries (j > i, p) of all sequences concatenated.
 * ---------------------------------------------------------------------------------------- */
int dafs_hip_set_bp(dafs_hip_ctx* ctx, const uint32_t* rowptr, const uint32_t* col, const float* val);
int dafs_hip_bp_result_size(dafs_hip_ctx* ctx, int relaxed, uint64_t* total_nnz, uint64_t* total_rowptr);
int dafs_hip_bp_fetch(dafs_hip_ctx* ctx, int relaxed, uint32_t* rowptr, uint32_t* col, float* val);

/* Batch hook replacing Fold::Model::calculate(const vector<Fasta>&, vector<BP>&)
 * (src/fold.cpp:60-68) for -s CONTRAfold (CONTRAfold::calculate, src/fold.cpp:174-189): inside /
 * outside / posterior of every sequence on the device, rows with p > th kept (reference CUTOFF
 * 0.01, src/dafs.cpp:1704).  Fills the same store dafs_hip_set_bp fills. */
int dafs_hip_fold_posteriors(dafs_hip_ctx* ctx, int model, float th);
/* The same in two halves: _begin enqueues the folding kernels on a stream of their own and returns, _end waits and
 * fills the store.  Between them the calls that do not need base-pairing probabilities may run (the all-pairs
 * alignment posteriors, dafs_hip_consistency_match): the folding occupies one workgroup per sequence, which leaves
 * most of the device idle at N < #CUs. */
int dafs_hip_fold_posteriors_begin(dafs_hip_ctx* ctx, int model, float th);
int dafs_hip_fold_posteriors_end(dafs_hip_ctx* ctx);
/* The same under per-sequence constraints: constraints[x] NULL or empty folds sequence x free, exactly
 * as dafs_hip_fold_posteriors_begin does (which is the case constraints = NULL); otherwise it is len[x] characters of "?.()"
 * as in dafs_hip_fold_posterior_dense.  _end is shared.  DAFS_HIP_EINVAL, with the sequence index in dafs_hip_last_error, for a
 * short string, an unknown character, unbalanced brackets, and a forced pair whose residues CONTRAfold cannot pair
 * (dafs_host_fold_complementary): the recursions exclude such a pair and the posterior is then no probability.  The context
 * stays usable after a refusal. */
int dafs_hip_fold_posteriors_constrained_begin(dafs_hip_ctx* ctx, int model, float th, const char* const* constraints);
int dafs_hip_fold_posteriors_constrained(dafs_hip_ctx* ctx, int model, float th, const char* const* constraints);
/* Several constraints per sequence: the per-level folds of DAFS::update_basepairing_probability
 * (src/dafs.cpp:635-661, one s_model_->calculate(seq, con, bp) per level) for every sequence of the context, all in one batch
 * of the folding kernels.  constraints[x * nlevels + k], 1 <= nlevels <= 4: NULL or empty for no fold of sequence x at level k,
 * otherwise as in dafs_hip_fold_posteriors_constrained_begin; a sequence without any string is folded once, free.  Row x of the
 * store holds, per cell, the maximum over x's folds of the posterior, kept where it exceeds th, in ascending column order (the
 * reference sums the levels into a dense matrix instead; --bp-update keeps doing that).  _end is shared.  With nlevels = 1 the
 * store is dafs_hip_fold_posteriors_constrained's bit for bit.  DAFS_HIP_EINVAL, with sequence and level in
 * dafs_hip_last_error and the context still usable: nlevels outside 1..4 and what dafs_hip_fold_posteriors_constrained_begin
 * refuses. */
int dafs_hip_fold_posteriors_levels_begin(dafs_hip_ctx* ctx, int model, float th, uint32_t nlevels, const char* const* constraints);
int dafs_hip_fold_posteriors_levels(dafs_hip_ctx* ctx, int model, float th, uint32_t nlevels, const char* const* constraints);
/* Single-sequence call replacing CONTRAfold<float>::ComputePosterior (src/contrafold/wrapper.cpp:181-200)
 * and, with a constraint string of len chars from "?.()" ('?' free, '.' unpaired, brackets forced),
 * Fold::Model::calculate(seq, str, bp) (src/fold.cpp:191-207).  post: (len+1)(len+2)/2 floats,
 * upper-triangular rows i = 0..len, columns j = i..len; logz (optional): log partition function. */
int dafs_hip_fold_posterior_dense(dafs_hip_ctx* ctx, const char* seq, uint32_t len, const char* constraint, float* post,
                                  float* logz);

/* Host-side helper (no device work): DAFS::build_tree (src/dafs.cpp:446-492) on the N*N similarity matrix.
 * score/left/right: 2N-1 entries; leaves have left = right = -1, node N+k is the k-th join of slots left, right. */
int dafs_host_build_tree(uint32_t n, const float* sim, float* score, int32_t* left, int32_t* right);
/* Host-side helper (no device work): the cut of a guide tree of n leaves (the arrays of dafs_host_build_tree) into clusters
 * (dafs --cluster, pipeline.cluster).  mode DAFS_CLUSTER_THRESHOLD: a join is kept when its score is >=
 * threshold and every join below it is kept.  mode DAFS_CLUSTER_COUNT: the count - 1 joins with the highest node indices are
 * undone and all others are kept, which leaves exactly `count` clusters.  A cluster is the leaf set of a maximal kept join, or
 * a single leaf.  labels[n]: the cluster of every leaf; the clusters are numbered from 0 by their smallest leaf.  *n_clusters:
 * their number.  n = 1 gives one cluster.  The argument that the mode does not read is ignored.  DAFS_HIP_EINVAL (message in
 * dafs_hip_last_error): n = 0, a null pointer, an unknown mode, a NaN threshold, a count outside 1..n, a malformed tree (a leaf
 * with a child; a join whose children are not two different earlier nodes; a node that is a child twice or, the root apart,
 * never). */
enum { DAFS_CLUSTER_THRESHOLD = 0, DAFS_CLUSTER_COUNT = 1 };
int dafs_host_cluster_cut(uint32_t n, const float* score, const int32_t* left, const int32_t* right, int mode, float threshold,
                          uint32_t count, uint32_t* labels, uint32_t* n_clusters);

/* Single, complete and average linkage (UPGMA) of an n x n similarity matrix, joined on the device (no counterpart in the
 * reference; the contract, to the bit; `dafs --cluster-linkage`, pipeline.cluster(linkage=...)).
 * score/left/right: 2n-1 entries in the layout of dafs_host_build_tree, so dafs_host_cluster_cut and dafs_host_cluster_table
 * take them unchanged.  Join t (node n + t) takes the pair of active slots a < b with the highest current similarity (compared
 * as floats; among equals the smallest a, then the smallest b), and slot a then holds the joined cluster with, for every other
 * active slot k, p = S(a,k), q = S(b,k): single p >= q ? p : q, complete p <= q ? p : q, average
 * (float)(((double)n_a * p + (double)n_b * q) / (double)(n_a + n_b)).  Join scores never rise.
 * sim: a host n x n matrix of which only the entries x < y are read, all of them finite; or NULL for the context's own
 * similarity block (a one-family context of n sequences after dafs_hip_similarity, a full-pair-set dafs_hip_align_posteriors,
 * dafs_hip_set_mp or dafs_hip_mp_install), read from its device copy without a download and left untouched, as are the stores.
 * n = 1 gives the one-leaf tree without a launch.  n up to 65 536 (a working copy of n * n floats on the device).
 * DAFS_HIP_EINVAL with a message in dafs_hip_last_error, outputs untouched and the context usable: a null pointer, an unknown
 * linkage, n = 0 or above 65 536, a non-finite entry above the diagonal (no join runs), sim = NULL on a context without a
 * similarity block, with several families or with another number of sequences.  DAFS_HIP_ENOMEM: the device allocation
 * failed. */
enum { DAFS_LINKAGE_SINGLE = 1, DAFS_LINKAGE_COMPLETE = 2, DAFS_LINKAGE_AVERAGE = 3 };
int dafs_hip_linkage_tree(dafs_hip_ctx* ctx, int linkage, uint32_t n, const float* sim, float* score, int32_t* left, int32_t* right);
/* L0 of the same (no counterpart in the reference): the caller's device matrix d_sim (n x n floats, the
 * entries x < y read, left untouched), the caller's workspace of dafs_hipk_linkage_workspace(n) bytes (256-byte aligned; 0 for
 * n = 0 or above 65 536) and device outputs of 2n-1 entries; two kernels on hip_stream, no allocation and no wait.  n >= 2.
 * When the stream has drained the workspace begins with { uint32 nonfinite; uint32 joins; uint64 rescans }: nonfinite > 0 is
 * the refusal of a non-finite entry above the diagonal, after which no join ran and only the leaves are written; otherwise
 * joins = n - 1.  DAFS_HIP_LINKAGE_LDS=0 (read per call, here and in dafs_hip_linkage_tree) keeps the per-row state in the
 * workspace at every n instead of in LDS up to n = 10 224; it changes no result. */
size_t dafs_hipk_linkage_workspace(uint32_t n);
int dafs_hipk_linkage(int linkage, uint32_t n, const float* d_sim, void* d_workspace, float* d_score, int32_t* d_left, int32_t* d_right,
                      void* hip_stream);

/* The neighbour-joining tree (Saitou & Nei in the Studier-Keppler form) of an n x n distance matrix, joined on the device (no
 * counterpart in the reference; the contract, to the bit; `dafs --phylogeny`, `--cov-tree nj`,
 * Context.nj_tree).  dist: a host n x n matrix of doubles of which only the entries x < y are read, all of them finite; the rest
 * may hold anything.  left/right: 2n-1 entries in the layout of dafs_host_build_tree, so dafs_hip_alignment_covariation_null,
 * dafs_host_cluster_table and dafs_host_newick take them unchanged.  length[2n-1]: the length of the branch above each node, 0.0
 * at the root; the last join puts the root in the middle of the last edge.  With m active slots, R[k] the running sum of row k
 * and D symmetric, join t (node n + t) takes the active pair a < b with the smallest
 * Q = ((double)(m - 2) * D(a,b) - R[a]) - R[b] (compared as doubles; among equals the smallest a, then the smallest b), writes
 * la = 0.5 * D(a,b) + (R[a] - R[b]) / (2.0 * (double)(m - 2)) (0.5 * D(a,b) when m = 2) and lb = D(a,b) - la as they are
 * computed (negative lengths are not clamped), and slot a then holds the join with, for every other active k,
 * D(a,k) = 0.5 * ((D(a,k) + D(b,k)) - D(a,b)).  n = 1 gives the one-leaf tree without a launch.  n up to 16 384 (a working copy
 * of n * n doubles on the device).
 * DAFS_HIP_EINVAL with a message in dafs_hip_last_error, outputs untouched and the context usable: a null pointer, n = 0 or
 * above 16 384, a non-finite entry above the diagonal (no join runs), and any non-finite value that the joins write into the
 * distances, the row sums or the lengths (overflow: the joins run to their end and the call then refuses).  DAFS_HIP_ENOMEM: the
 * device allocation failed. */
int dafs_hip_nj_tree(dafs_hip_ctx* ctx, uint32_t n, const double* dist, int32_t* left, int32_t* right, double* length);
/* L0 of the same: the caller's device matrix d_dist (n x n doubles, the entries x < y read, left
 * untouched), the caller's workspace of dafs_hipk_nj_workspace(n) bytes (256-byte aligned; 0 for n = 0 or above 16 384) and
 * device outputs of 2n-1 entries; 2 + 2 (n - 1) kernels on hip_stream, no allocation and no wait.  n >= 2.  When the stream has
 * drained the workspace begins with { uint32 nonfinite; uint32 written; uint32 joins; uint32 fault }: nonfinite > 0 is the
 * refusal of a non-finite entry above the diagonal, after which no join ran and only the leaves are written; written > 0 is the
 * refusal of an overflow (the outputs are then to be discarded); otherwise joins = n - 1 and fault = 0. */
size_t dafs_hipk_nj_workspace(uint32_t n);
int dafs_hipk_nj(uint32_t n, const double* d_dist, void* d_workspace, int32_t* d_left, int32_t* d_right, double* d_length,
                 void* hip_stream);
/* Host-side helper (no device work): the distances of an alignment's rows for the call above, from the n x n integer matrices
 * of dafs_hip_alignment_identity.  For r != s, comp = aligned(r,s) and mism = comp - ident(r,s): a letter
 * outside ACGU is aligned and identical to nothing, so it counts as a difference.  DAFS_NJ_P: (double)mism / (double)comp, 1.0
 * when comp = 0.  DAFS_NJ_JC (Jukes-Cantor): 3.0 when comp = 0 or 4 mism >= 3 comp (in uint64); otherwise, with
 * x = 1.0 - (4.0 * (double)mism) / (3.0 * (double)comp) and k = floor(-0.75 * log(x) * 1048576.0 + 0.5), the value
 * min(k, 3 * 2^20) / 1048576.0.  dist[n * n] is written whole, 0.0 on the diagonal.  DAFS_HIP_EINVAL: a null pointer, n = 0, an
 * unknown model, ident(r,s) > aligned(r,s). */
enum { DAFS_NJ_P = 0, DAFS_NJ_JC = 1 };
int dafs_host_nj_distances(uint32_t n, const uint32_t* ident, const uint32_t* aligned, int model, double* dist);
/* Host-side helper (no device work): a tree of n leaves (the arrays of dafs_host_build_tree) as one Newick line into *out
 * (dafs_host_free).  A join is "(L:len,R:len)" with the left child first, nested; the root carries no length and the text
 * ends in ";\n"; lengths are written as %.9g; length = NULL writes the topology only.  A name holding any of ()[]':;, or white
 * space is put in single quotes with every ' doubled.  n = 1 gives "name;\n".  The walk keeps its own stack: a chain of any
 * depth uses none of the call stack.  DAFS_HIP_EINVAL (message in dafs_hip_last_error): n = 0, a null pointer or name, and a
 * malformed tree by the checks of dafs_host_cluster_cut. */
int dafs_host_newick(uint32_t n, const char* const* names, const int32_t* left, const int32_t* right, const double* length, char** out);
/* What both drivers say when they refuse a combination of the phylogeny options */
enum {
  DAFS_PHYLOGENY_NO_PAIRWISE = 0,      /* a tree asked of pairwise alignments */
  DAFS_PHYLOGENY_NO_SEED_EACH,         /* a tree asked of per-sequence placements */
  DAFS_PHYLOGENY_TOO_MANY_ROWS,        /* more than 16 384 rows */
  DAFS_PHYLOGENY_MODEL_NEEDS_TREE,     /* --phylogeny-model without --phylogeny */
  DAFS_PHYLOGENY_UNKNOWN_MODEL,        /* a model that is neither jc nor p */
  DAFS_PHYLOGENY_COV_TREE_NEEDS_NULL,  /* --cov-tree without --cov-null tree */
  DAFS_PHYLOGENY_UNKNOWN_COV_TREE      /* a tree that is neither average nor nj */
};
const char* dafs_host_phylogeny_refusal(int which);
/* What both drivers say when they refuse a combination of the bootstrap options.  The texts have a
 * function of their own: dafs_host_phylogeny_refusal answers "" to every number above its seven, and keeps doing so. */
enum {
  DAFS_BOOTSTRAP_NEEDS_TREE = 0,      /* a bootstrap option without --phylogeny */
  DAFS_BOOTSTRAP_COUNT,               /* a number of replicates outside 1 .. 65 536 */
  DAFS_BOOTSTRAP_NEEDS_REPLICATES,    /* the seed or the support table without replicates */
  DAFS_BOOTSTRAP_NO_COLUMN            /* replicates of an alignment without a used column */
};
const char* dafs_host_bootstrap_refusal(int which);

/* Bootstrap support of a neighbour-joining tree (Felsenstein's bootstrap; no counterpart in the reference; the contract, to the
 * bit; tests/bootstrap_ref.py restates it).
 *
 * dafs_hip_nj_trees: `count` neighbour-joining trees in one call.  dist: host matrices [count][n][n], each read and joined as
 * dafs_hip_nj_tree reads and joins its one; left/right/length: [count][2n-1].  Up to 2 048 rows all joins of a matrix run in one
 * workgroup and all matrices in one launch (k_nj_batch); above that, or when DAFS_NJ_BATCH_MAX_N (tests only; 0: never) lowers the
 * limit, the matrices go one by one through the kernels of dafs_hip_nj_tree.  Both forms give identical arrays.  The refusals
 * of dafs_hip_nj_tree, with the matrix named; count = 0 is refused too.
 * L0 dafs_hipk_nj_batch: device matrices, the caller's workspace of dafs_hipk_nj_batch_workspace(n, count) bytes (256-byte
 * aligned; 0 for n < 2, n above 16 384 or count = 0) and device outputs, on hip_stream without allocation or wait.  The
 * workspace begins with `count` heads { uint32 nonfinite, written, joins, fault } as in dafs_hipk_nj. */
int dafs_hip_nj_trees(dafs_hip_ctx* ctx, uint32_t n, uint32_t count, const double* dist, int32_t* left, int32_t* right, double* length);
size_t dafs_hipk_nj_batch_workspace(uint32_t n, uint32_t count);
int dafs_hipk_nj_batch(uint32_t n, uint32_t count, const double* d_dist, void* d_workspace, int32_t* d_left, int32_t* d_right,
                       double* d_length, void* hip_stream);
/* dafs_hip_alignment_bootstrap: B replicate alignments of the used columns of cell[n][len] (codes of dafs_hip_alignment_identity;
 * use: len bytes or NULL), drawn with replacement: with U used columns cols[0..U) ascending, mix and GOLDEN of section 13 and
 * base_k = mix(seed + GOLDEN * (k + 1)), column i of replicate k is cols[((mix(base_k + i) >> 32) * U) >> 32].  Every replicate
 * gets the distances of dafs_host_nj_distances under `model` (DAFS_NJ_JC / DAFS_NJ_P) from its own counts and the tree of
 * dafs_hip_nj_tree.  support[2n-1]: per node of the main tree (main_left, main_right: the tree of the same rows, any well-formed
 * tree) the number of replicate trees that hold the node's split (the leaves below it, or the rest if leaf 0 is among them); -1
 * for the root and for a split with fewer than two leaves on a side; the two children of the root get the same count.
 * rep_left / rep_right (both or neither; [B][2n-1]) receive the replicate trees.  n <= 3: all -1, nothing drawn or launched,
 * the replicate arrays are filled with -1.  A row that a replicate leaves without a residue is not refused: its pairs have
 * comp = 0.  DAFS_HIP_EINVAL with a message, outputs untouched, context usable: a null pointer, n = 0 or above 16 384, len = 0,
 * B = 0 or above 65 536, no used column, a code above 5, an unknown model, a malformed main tree (the checks of
 * dafs_host_cluster_cut), and the refusals of dafs_hip_nj_tree for any replicate.  Tests-only switches that change no result:
 * DAFS_NJ_BOOT_BYTES (device bytes per chunk of replicates), DAFS_NJ_BOOT_GUARD (how near an integer the quantised Jukes-Cantor
 * value may come before the host recomputes the entry; 0.5: every entry), DAFS_NJ_BOOT_FIXUPS (the capacity of that list),
 * DAFS_NJ_BATCH_MAX_N. */
int dafs_hip_alignment_bootstrap(dafs_hip_ctx* ctx, uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use, int model, uint32_t B,
                                 uint64_t seed, const int32_t* main_left, const int32_t* main_right, int32_t* support, int32_t* rep_left,
                                 int32_t* rep_right);
/* Replicate k of the call above as cells: out_cell[n][U], packed and read back through the device path of the call. */
int dafs_hip_bootstrap_alignment(dafs_hip_ctx* ctx, uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use, uint64_t seed, uint32_t k,
                                 uint8_t* out_cell);
/* How many fix-up entries the last dafs_hip_alignment_bootstrap of this thread sent through the host (measurement aid). */
uint64_t dafs_hip_bootstrap_fixups(void);
/* Host-side helper (no device work): support[2n-1] of a main tree against B replicate trees ([B][2n-1] each) as defined above,
 * exact, without recursion.  DAFS_HIP_EINVAL: a null pointer, n = 0, a malformed tree (the replicate is named). */
int dafs_host_tree_support(uint32_t n, const int32_t* left, const int32_t* right, uint32_t B, const int32_t* rep_left,
                           const int32_t* rep_right, int32_t* support);
/* Host-side helper: dafs_host_newick's line with the support in percent, (200 * support + B) / (2 * B) in integer division, as
 * the label of every join whose support is >= 0: "(A:0.1,B:0.2)87:0.05".  The split of the root's two children is labelled
 * once: on the left child if that is a join, otherwise on the right child.  With every support at -1 the text is
 * dafs_host_newick's.  DAFS_HIP_EINVAL also for B = 0 and a support above B. */
int dafs_host_newick_support(uint32_t n, const char* const* names, const int32_t* left, const int32_t* right, const double* length,
                             const int32_t* support, uint32_t B, char** out);
/* Host-side helper: the table of --phylogeny-support.  "# rows n replicates B seed S model M", then per non-trivial split of the
 * main tree, in node order and once per split (the rule above), tab-separated: node (1-based) support B percent size leaves;
 * size and leaves (names, comma-separated, in row order) are those of the side without the first row. */
int dafs_host_support_table(uint32_t n, const char* const* names, const int32_t* left, const int32_t* right, const int32_t* support,
                            uint32_t B, uint64_t seed, int model, char** out);

/* Transfer bootstrap of a neighbour-joining tree (the transfer bootstrap expectation of Lemoine et al., Nature 2018; no counterpart
 * in the reference; the contract, to the bit and in integers only; tests/transfer_ref.py restates it).
 * Sides, trivial splits and the root's two children are those of dafs_hip_alignment_bootstrap.  For a node v of the main tree with
 * a non-trivial split, depth(v) = min(|side(v)|, n - |side(v)|), and for a replicate tree T the transfer index phi(v, T) is the
 * minimum over all nodes u of T below its root, leaves included, of min(H, n - H) with H = |side(v) xor side(u)|: an integer in
 * 0 .. depth(v) - 1, 0 exactly when T holds the split.  transfer[v] is the sum of phi(v, T_k) over the B replicates; -1 for the
 * root and for trivial splits; both children of the root get the same sum.
 *
 * dafs_hip_tree_transfer: host trees, main (left, right)[2n-1] and replicates [B][2n-1], compared on the device
 * (tree_transfer.hip) in chunks under the byte budget of dafs_hip_alignment_bootstrap (DAFS_NJ_BOOT_BYTES shrinks them too).
 * transfer[2n-1]; transfer_each: NULL or [B][2n-1], phi per replicate, -1 where transfer is -1.  n <= 3: all -1, nothing
 * launched.  DAFS_HIP_EINVAL with a message, outputs untouched, context usable: a null pointer, n = 0 or above 16 384, B = 0 or
 * above 65 536, a malformed main tree, a malformed replicate tree (the replicate is named).
 *
 * L0 dafs_hipk_tree_transfer: `count` (1 to 32 768) device replicate trees d_left / d_right [count][2n-1] of n >= 4 leaves, on
 * hip_stream without allocation or wait.  d_pos[n]: the position of every leaf in the walk of the main tree, leaf 0 at position 0;
 * d_split: `splits` pairs (lo, len) of uint32, the sides of the main tree as runs [lo, lo + len) of positions, lo >= 1, len >= 2;
 * dafs_host_transfer_runs forms both from a host tree (pos[n], and per node lo and len, len = 0 for the root and trivial
 * splits).  d_transfer[splits]: 64-bit sums that the call ADDS to (the caller zeroes them before the first chunk); d_each: NULL
 * or [count][splits].  The workspace of dafs_hipk_tree_transfer_workspace(n, count) bytes (256-byte aligned; 0 for n < 4, n above
 * 16 384, count = 0 or above 32 768) begins with `count` heads { uint32 bad_tree, bad_split }, zeroed by the call: what the
 * kernels refuse (a leaf with a child, a child that is not an earlier node, a position that is not below n; a run that does not
 * lie in 1 .. n).  A refused replicate adds nothing and no index of it leaves its arrays. */
int dafs_hip_tree_transfer(dafs_hip_ctx* ctx, uint32_t n, const int32_t* main_left, const int32_t* main_right, uint32_t B,
                           const int32_t* rep_left, const int32_t* rep_right, int64_t* transfer, int32_t* transfer_each);
size_t dafs_hipk_tree_transfer_workspace(uint32_t n, uint32_t count);
int dafs_hipk_tree_transfer(uint32_t n, uint32_t count, uint32_t splits, const uint32_t* d_pos, const uint32_t* d_split, const int32_t* d_left,
                            const int32_t* d_right, void* d_workspace, uint64_t* d_transfer, int32_t* d_each, void* hip_stream);
int dafs_host_transfer_runs(uint32_t n, const int32_t* left, const int32_t* right, uint32_t* pos, uint32_t* lo, uint32_t* len);
/* dafs_hip_alignment_bootstrap with the transfer sums beside the counts: the same arguments, results and refusals, and
 * transfer[2n-1] (not NULL).  Per chunk the kernels run on the replicate trees where the joins left them, on the same stream;
 * only the sums come back, at the end. */
int dafs_hip_alignment_bootstrap_transfer(dafs_hip_ctx* ctx, uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use, int model,
                                          uint32_t B, uint64_t seed, const int32_t* main_left, const int32_t* main_right, int32_t* support,
                                          int32_t* rep_left, int32_t* rep_right, int64_t* transfer);
/* Host-side helpers.  dafs_host_split_depth: depth[2n-1], -1 for the root and trivial splits.  dafs_host_transfer_percent: the
 * transfer bootstrap expectation in percent, (200 * (M - transfer) + M) / (2 * M) with M = B * (depth - 1) in integer division
 * (halves round up, as the percent of dafs_host_newick_support); -1 for depth < 2, B = 0 or a sum outside 0 .. M.
 * dafs_host_newick_transfer: dafs_host_newick_support's text with that percent as the labels, under the same root-child rule.
 * dafs_host_transfer_table: "# rows n replicates B seed S model M measure transfer", then per non-trivial split the six fields of
 * dafs_host_support_table and depth, transfer, tbe.  dafs_host_transfer_refusal: what both drivers say when they refuse the
 * option; a function of its own, as dafs_host_bootstrap_refusal answers "" above its four. */
enum {
  DAFS_TRANSFER_NEEDS_REPLICATES = 0  /* --phylogeny-transfer without --phylogeny-bootstrap */
};
const char* dafs_host_transfer_refusal(int which);
int dafs_host_split_depth(uint32_t n, const int32_t* left, const int32_t* right, int32_t* depth);
int32_t dafs_host_transfer_percent(int64_t transfer, uint32_t depth, uint32_t B);
int dafs_host_newick_transfer(uint32_t n, const char* const* names, const int32_t* left, const int32_t* right, const double* length,
                              const int64_t* transfer, uint32_t B, char** out);
int dafs_host_transfer_table(uint32_t n, const char* const* names, const int32_t* left, const int32_t* right, const int32_t* support,
                             const int64_t* transfer, uint32_t B, uint64_t seed, int model, char** out);

/* Host-side helper (no device work): the merge of `dafs --seed` and pipeline.add, k new sequences
 * placed into a fixed seed alignment of C columns.  lens: k sequence lengths; z: their column maps from the k nodes (leaf j
 * against the seed) concatenated, per residue a seed column or DAFS_HIP_NONE, the seed columns strictly increasing within
 * each sequence (else DAFS_HIP_EINVAL).  A matched residue goes in its seed column; an unmatched one is anchored after the
 * seed column of the nearest earlier matched residue of its sequence, or at the start (anchor -1).  The merged alignment is,
 * for c = -1, 0, ..., C-1: seed column c (c >= 0), then max_j (residues of j anchored at c) insert columns, which every
 * sequence fills from the left.  For k = 1 this is DAFS::project_alignment((leaf), seed, z) (src/dafs.cpp:766-825).
 * seed_col[C]: the merged column of each seed column; res_col[sum lens]: the merged column of each residue, sequence after
 * sequence; *width: the number of merged columns. */
int dafs_host_merge_added(uint32_t C, uint32_t k, const uint32_t* lens, const uint32_t* z, uint32_t* seed_col, uint32_t* res_col,
                          uint32_t* width);

/* ------------------------------------------------------------------------------------------
 * Host text (no device work; dafs_amd/csrc/host_text.cpp): the text formats and memory estimates that the `dafs` command line
 * and the Python driver share, each defined once.  Returned text (the char** argument) is allocated by the library and freed
 * by the caller with dafs_host_free; a list of strings comes back joined by '\n' (no name or row holds one).  DAFS_HIP_EINVAL
 * leaves its message in dafs_hip_last_error(): for the seed reader it is the refusal the user sees.
 * ---------------------------------------------------------------------------------------- */
void dafs_host_free(void* text);
/* Infernal's PP character: '*' for p >= 0.95, else the digit floor(p * 10 + 0.5) */
char dafs_host_pp_char(double p);
/* Stockholm names of n FASTA headers: the first word, "seq<k>" (k 1-based) for an empty header, ".2", ".3", ... for repeats */
int dafs_host_stockholm_names(uint32_t n, const char* const* headers, char** names);
/* One alignment as a Stockholm block (DESIGN.md "Alignment reliability"): n rows of len columns in printed order ('-' for
 * gaps), residue_rel[r] the reliabilities of row r's residues, col_rel[len] per column, ss the bracket string.  Optional
 * (NULL: no such line): tree_line ("#=GF CC"), rf[len] ("#=GC RF": 'x' where nonzero), cov ("#=GC cov_SS_cons"). */
int dafs_host_stockholm_block(const char* tree_line, uint32_t n, uint32_t len, const char* const* names, const char* const* rows,
                              const double* const* residue_rel, const double* col_rel, const char* ss, const uint8_t* rf,
                              const char* cov, char** block);
/* The same block with per-row structures: row_ss[r] (NULL array: none, the block of
 * dafs_host_stockholm_block) is row r's structure laid into its columns -- a bracket character of dafs_hip_make_brackets at a
 * residue's column, '.' elsewhere -- and is written as "#=GR <name> SS" after the row's PP line.  A string whose length is
 * not len, or with anything but '.' at a gap column, is refused (DAFS_HIP_EINVAL). */
int dafs_host_stockholm_block_rows(const char* tree_line, uint32_t n, uint32_t len, const char* const* names, const char* const* rows,
                                   const double* const* residue_rel, const double* col_rel, const char* ss, const uint8_t* rf,
                                   const char* cov, const char* const* row_ss, char** block);
/* The merged alignment of a --seed-each run as one Stockholm block: the n rows, then a "#=GR <name> PP"
 * line for every row r with residue_rel[r] not NULL (the placed rows; a seed row has none), "#=GC SS_cons", "#=GC PP_cons",
 * "#=GC RF" ('x' where rf is nonzero) and "//"; no "#=GF CC" line.  PP_cons: per column the mean of the values that the rows
 * with a PP line hold there, a running double sum in row order; '.' for a column where none of them has a residue.  col_rel
 * (len entries, or NULL) receives those means, NaN for a '.' column.  The labels are padded to the longest of the names, the
 * "#=GR <name> PP" labels that are written and the "#=GC" labels, plus one. */
int dafs_host_stockholm_block_merged(uint32_t n, uint32_t len, const char* const* names, const char* const* rows,
                                     const double* const* residue_rel, const char* ss, const uint8_t* rf, double* col_rel, char** block);
/* What both drivers say when a merged alignment is asked for without the seed's structure */
const char* dafs_host_merged_refusal(void);
/* The code of a residue for dafs_hip_alignment_covariation: A 0, C 1, G 2, U / T 3 in either case, everything else 4 */
uint8_t dafs_host_cov_code(char residue);
/* The cov_SS_cons characters: '2' at both columns of every pair of ss with pair_e <= e_max (a NaN never is), '.' elsewhere */
int dafs_host_cov_ss_cons(uint32_t len, const uint32_t* ss, const double* pair_e, double e_max, char** chars);
/* The --covariation table of the rows' codes code[n * len], the structure ss and the arrays
 * dafs_hip_alignment_covariation returned: the pairs of ss (kind ss), then every other pair {c, best[c]} with best_e <= 0.05 */
int dafs_host_covariation_table(uint32_t n, uint32_t len, const uint8_t* code, const uint32_t* ss, const uint32_t* best,
                                const double* best_score, const double* best_e, const double* pair_score, const double* pair_e,
                                const uint32_t* pair_rows, const uint32_t* pair_canonical, const uint32_t* pair_types, char** table);
/* The --pairwise-scores table: per pair k the line "x+1 y+1 names[x] names[y] sim score iterations", tab-separated, floats as
 * %.9g; iterations is signed (-1: a pair that was not asked) */
int dafs_host_pairwise_table(uint64_t npairs, const uint32_t* x, const uint32_t* y, uint32_t nnames, const char* const* names,
                             const double* sim, const double* score, const int64_t* iterations, char** table);
/* The --cluster-table table: per sequence i the line "i+1 name length cluster size join nearest_in sim_in
 * nearest_out sim_out", tab-separated, floats as %.9g; the names are dafs_host_stockholm_names of the n headers.  labels: the
 * clusters of dafs_host_cluster_cut on the tree score / left / right (cluster is labels[i] + 1, size its number of members, join
 * the score of the join whose leaves are the cluster, "nan" for a cluster of one); sim: the n x n similarity matrix.  nearest_in
 * / nearest_out: the most similar other sequence inside / outside i's cluster (1-based, the smallest index among equals) and
 * that similarity; "0" and "nan" where there is none.  Refused (DAFS_HIP_EINVAL): a cluster that is not the leaf set of one
 * node of the tree. */
int dafs_host_cluster_table(uint32_t n, const char* const* headers, const uint32_t* length, const uint32_t* labels, const float* score,
                            const int32_t* left, const int32_t* right, const float* sim, char** table);
/* The --seed-scores table of a --seed-each run: per new sequence j the line "j+1 name length matched
 * length-matched score iterations", tab-separated, floats as %.9g; the names are dafs_host_stockholm_names of the n headers.
 * matched[j] > length[j] is refused (DAFS_HIP_EINVAL). */
int dafs_host_seed_table(uint32_t n, const char* const* headers, const uint32_t* length, const uint32_t* matched, const double* score,
                         const int64_t* iterations, char** table);
/* The seed reader of --seed.  _parse: the bytes of a Stockholm or aligned-FASTA file into *n names and
 * rows as the file holds them.  _clean: the checks (an empty seed, rows of unequal length, a character that is neither a letter
 * nor a gap, a row without residues), then the rows without their all-gap columns, '-' for every gap. */
int dafs_host_seed_parse(const char* text, size_t bytes, uint32_t* n, char** names, char** rows);
int dafs_host_seed_clean(uint32_t n, const char* const* names, const char* const* rows, char** cleaned);
/* The same reader with the seed's consensus structure.  _parse_structure: also the structure's characters
 * as the file holds them -- the "#=GC SS_cons" lines of a Stockholm seed's first alignment, concatenated over its blocks in
 * order; the record named SS_cons of an aligned-FASTA seed -- and *has_structure = 1, or an empty text and 0 when the file has
 * none.  _clean_structure: dafs_host_seed_clean's checks and rows; then the structure over the cleaned columns into ss (room
 * for strlen(rows[0]) entries; the first *columns are written): the partner column at the left column of a pair,
 * DAFS_HIP_NONE elsewhere.  "()", "<>", "[]", "{}" are pairs, each kind matched with its own kind; letters and ". , : _ - ~"
 * are unpaired; a pair that loses a column with the all-gap columns is dropped.  Refused (DAFS_HIP_EINVAL, message in
 * dafs_hip_last_error): any other character, a length that is not the rows', an unbalanced kind, pairs that cross once all
 * kinds are merged. */
int dafs_host_seed_parse_structure(const char* text, size_t bytes, uint32_t* n, int* has_structure, char** names, char** rows,
                                   char** structure);
int dafs_host_seed_clean_structure(uint32_t n, const char* const* names, const char* const* rows, const char* structure,
                                   uint32_t* ss, uint32_t* columns, char** cleaned);
/* 1 when CONTRAfold can pair the two residues: AU, UA, GC, CG, GU, UG in either case.  Its alphabet is "ACGU": T is not U
 * there, so a pair with a T is not complementary (dafs_amd/csrc/contrafold.hip, cf_comp on the loaded symbols). */
int dafs_host_fold_complementary(char a, char b);
/* The folding constraint that the structure ss (len columns, as above) puts on one row: mask_row[len]
 * marks the row's residues, residues holds them (as many characters as mask_row has non-zero bytes, else DAFS_HIP_EINVAL), out
 * receives one character per residue and a NUL.  '?' everywhere; '(' and ')' at the two residues of a pair of ss when the row
 * holds both, they are complementary (dafs_host_fold_complementary) and at least 4 residues apart (j - i >= 4). */
int dafs_host_row_constraint(uint32_t len, const uint8_t* mask_row, const uint32_t* ss, const char* residues, char* out);
/* The seed reader for a consensus structure whose pairs may cross (`dafs --knots`).  As
 * dafs_host_seed_clean_structure, with level (room for strlen(rows[0]) bytes): the pair's level at both of its columns, 0xFF at
 * unpaired columns, the convention of dafs_hip_consensus_structures_levels.  Groups, in this order: "()", "[]", "{}", "<>", then
 * the letters 'A'..'Z', an upper-case letter opening and the same letter in lower case closing; each group is matched
 * last-in-first-out with itself; ". , : _ - ~" are unpaired.  A pair that loses a column with the all-gap columns is dropped;
 * then, group after group, a non-empty group goes to the lowest level at which none of its pairs crosses (a < i < b < j or
 * i < a < j < b) a pair already placed there.  Refused (DAFS_HIP_EINVAL, message in dafs_hip_last_error): any other character,
 * a length that is not the rows', an unbalanced group (a lower-case letter that closes nothing and an upper-case letter never
 * closed among them), and a group that would need a level beyond DAFS_HIP_MAX_LEVELS, which the message names. */
int dafs_host_seed_clean_structure_levels(uint32_t n, const char* const* names, const char* const* rows, const char* structure,
                                          uint32_t* ss, uint8_t* level, uint32_t* columns, char** cleaned);
/* dafs_host_row_constraint once per level of a structure with levels (the reference makes these strings in
 * DAFS::update_basepairing_probability, src/dafs.cpp:635-653).  level[len] as above (NULL: every pair of level 0), 1 <= nlevels <=
 * DAFS_HIP_MAX_LEVELS, every pair's level below nlevels and equal at both columns (else DAFS_HIP_EINVAL).  out: nlevels strings,
 * string k at out + k * (residues + 1).  String k: '?' everywhere; a pair of level k as dafs_host_row_constraint writes it; a pair
 * of another level whose two residues the row holds '.' at both, complementary or not (src/dafs.cpp:650); a pair the row holds
 * one residue of stays '?'.  A string k >= 1 without a '(' is left empty: the row is not folded for that level.  With
 * nlevels = 1 the one string is dafs_host_row_constraint's. */
int dafs_host_row_constraint_levels(uint32_t len, const uint8_t* mask_row, const uint32_t* ss, const uint8_t* level, uint32_t nlevels,
                                    const char* residues, char* out);
/* dafs_host_seed_table with the structure support of every placed sequence (dafs_hip_structure_support) as four more columns,
 * "pairs canonical half expected" (expected as %.9g); all four arrays NULL: the table of dafs_host_seed_table. */
int dafs_host_seed_table_support(uint32_t n, const char* const* headers, const uint32_t* length, const uint32_t* matched,
                                 const double* score, const int64_t* iterations, const uint32_t* both, const uint32_t* canonical,
                                 const uint32_t* half, const double* expected, char** table);
/* Estimated device memory (bytes) of one family's phase-1 stores and of one resident node; the default budget of a sub-batch
 * of families or a chunk of pairs.  _pack_greedy: group_of[k] is the group of item k, groups filled in input order up to
 * max_bytes, an item over the budget alone. */
uint64_t dafs_host_family_bytes(uint32_t n, const uint32_t* lens);
uint64_t dafs_host_node_bytes(uint32_t len1, uint32_t len2);
uint64_t dafs_host_batch_bytes(void);
/* Estimated device memory (bytes) of one new sequence of a --seed-each run: dafs_host_family_bytes of the m seed lengths and
 * new_len, plus dafs_host_node_bytes(new_len, seed_columns) */
uint64_t dafs_host_seed_each_bytes(uint32_t m, const uint32_t* seed_lens, uint32_t seed_columns, uint32_t new_len);
/* Estimated device memory (bytes) of one alignment of n_rows rows and len columns inside dafs_hip_consensus_structures, and the
 * default budget of one of its chunks. */
uint64_t dafs_host_structure_bytes(uint32_t n_rows, uint32_t len);
uint64_t dafs_host_structures_batch_bytes(void);
/* The same estimate inside dafs_hip_consensus_structures_levels: the level's own structure, the column
 * keys, the level bytes, the per-level descriptors, flags and scores on top of dafs_host_structure_bytes. */
uint64_t dafs_host_structure_levels_bytes(uint32_t n_rows, uint32_t len);
/* The same inside dafs_hip_consensus_structures_auto with ncand candidates: on top of the levels'
 * estimate, every candidate's structure, score and decoder descriptor, and the sums. */
uint64_t dafs_host_structure_auto_bytes(uint32_t n_rows, uint32_t len, uint32_t ncand);
/* The same two for dafs_hip_alignment_reliabilities. */
uint64_t dafs_host_reliability_bytes(uint32_t n_rows, uint32_t len);
uint64_t dafs_host_reliability_batch_bytes(void);
int dafs_host_pack_greedy(uint32_t n, const uint64_t* sizes, uint64_t max_bytes, uint32_t* group_of);

/* ------------------------------------------------------------------------------------------
 * L1: probabilistic consistency transforms.
 * Replaces DAFS::relax_basepairing_probability (src/dafs.cpp:326-375) and
 * DAFS::relax_matching_probability (src/dafs.cpp:258-324) as called from DAFS::run
 * (src/dafs.cpp:1822-1827): both read the un-relaxed stores; weight 0 skips a transform.
 * ---------------------------------------------------------------------------------------- */
int dafs_hip_consistency(dafs_hip_ctx* ctx, float w_pct_a, float w_pct_s);
/* the two transforms separately (each reads un-relaxed stores only) */
int dafs_hip_consistency_match(dafs_hip_ctx* ctx, float w_pct_a);
int dafs_hip_consistency_bp(dafs_hip_ctx* ctx, float w_pct_s);
/* DAFS::relax_fourway_consistency (src/dafs.cpp:377-444; option -f, called at :1808-1809 between the alignment model and
 * the similarity scores): the un-relaxed matching store is replaced by its mix with the stacking evidence of the un-relaxed
 * base-pairing store (dafs_hip_fold_posteriors / dafs_hip_set_bp must have run), and the similarity scores are recomputed
 * from the result.  Call before dafs_hip_get_sim / dafs_hip_consistency*.  w_pct_f = 0 does nothing, like the reference. */
int dafs_hip_fourway_consistency(dafs_hip_ctx* ctx, float w_pct_f);
/* relax_matching_probability for the output pairs [pair_begin, pair_end) of the row-major pair enumeration only (every
 * output pair is independent of the others, src/dafs.cpp:265-315): the shard of one rank of a multi-GPU run.  The
 * other pairs of the relaxed store stay empty until the gathered whole is installed with dafs_hip_mp_install. */
int dafs_hip_consistency_match_range(dafs_hip_ctx* ctx, float w_pct_a, uint64_t pair_begin, uint64_t pair_end);
/* The same for a list of output pairs: npairs >= 1 strictly ascending pair ids of the context (families one after another,
 * row-major inside each).  The listed pairs' relaxed rows are those of dafs_hip_consistency_match, bit for bit; the others are
 * empty (zero counts, offsets and row pointers).  The relaxed store is marked as holding listed pairs only, and keeps the list,
 * until another call produces it: dafs_hip_alignment_reliabilities refuses an alignment that needs a pair outside the list
 * (DAFS_HIP_EINVAL) instead of taking the empty pairs for zero probabilities.  DAFS_HIP_EINVAL also for w_pct_a = 0, an empty list, an id that does not ascend or is not a pair of the
 * context, and a missing or partial un-relaxed store. */
int dafs_hip_consistency_match_pairs(dafs_hip_ctx* ctx, float w_pct_a, uint64_t npairs, const uint64_t* pair_ids);

/* ------------------------------------------------------------------------------------------
 * L1: decoder plugins on dense row-major matrices (host buffers).
 * dafs_hip_nussinov_decode replaces SparseNussinov::decode(w,p,q,ss) (src/nussinov.cpp:207-298);
 * with q == NULL it is the final-decode overload decode(p,ss,str) (:300-392, score p-th, w unused;
 * brackets: dafs_hip_make_brackets).  ss[i] = partner index or DAFS_HIP_NONE.
 * dafs_hip_nw_envelope replaces SparseNeedlemanWunsch::initialize (src/needleman_wunsch.cpp:198-253):
 * env[2*i], env[2*i+1] = first/last column of row i, i = 0..L1.
 * dafs_hip_nw_decode replaces SparseNeedlemanWunsch::decode (:255-422), q may be NULL;
 * al[i] = aligned column or DAFS_HIP_NONE.
 * ---------------------------------------------------------------------------------------- */
int dafs_hip_nussinov_decode(dafs_hip_ctx* ctx, float th, float w, uint32_t L, const float* p, const float* q,
                             uint32_t* ss, float* score);
int dafs_hip_nw_envelope(dafs_hip_ctx* ctx, float th, uint32_t L1, uint32_t L2, const float* p, uint32_t* env);
int dafs_hip_nw_decode(dafs_hip_ctx* ctx, float th, uint32_t L1, uint32_t L2, const float* p, const float* q,
                       const uint32_t* env, uint32_t* al, float* score);
/* The dense decoder classes of the reference (Nussinov, src/nussinov.cpp:32-204: every pair scores, bifurcation over
 * every split; NeedlemanWunsch, src/needleman_wunsch.cpp:28-196: no envelope).  DAFS instantiates the sparse ones
 * (src/dafs.cpp:1692,1759); these complete the plugin set.  q may be NULL (the final-decode overloads). */
int dafs_hip_nussinov_decode_dense(dafs_hip_ctx* ctx, float th, float w, uint32_t L, const float* p, const float* q,
                                   uint32_t* ss, float* score);
int dafs_hip_nw_decode_dense(dafs_hip_ctx* ctx, float th, uint32_t L1, uint32_t L2, const float* p, const float* q,
                             uint32_t* al, float* score);
/* make_brackets (src/nussinov.cpp:401-413): str needs L+1 bytes. Host-only helper. */
void dafs_hip_make_brackets(uint32_t L, const uint32_t* ss, char* str);
/* The same for a structure of several levels: the pair at column i prints with the bracket kind of
 * level[i], "()", "[]", "{}", "<>" for levels 0..3 (the reference's table, src/fold.cpp:57-58).  A pair whose level is
 * outside 0..3 or whose partner is outside the structure prints as unpaired.  level == NULL: every pair is of level 0. */
void dafs_hip_make_brackets_levels(uint32_t L, const uint32_t* ss, const uint8_t* level, char* str);
/* Level-by-level decode of a dense host matrix (dafs_hip_consensus_structures_levels has the contract):
 * th[nlevels], 1 <= nlevels <= DAFS_HIP_MAX_LEVELS, th[k] > 0 for k >= 1 (else DAFS_HIP_EINVAL, outputs untouched).
 * ss[L] the merged structure, level[L] (may be NULL) the pair's level at both of its columns and 0xFF elsewhere,
 * score[nlevels] (may be NULL).  Level 0 is dafs_hip_nussinov_decode without q at th[0], bit for bit. */
#define DAFS_HIP_MAX_LEVELS 4u
int dafs_hip_nussinov_decode_levels(dafs_hip_ctx* ctx, uint32_t nlevels, const float* th, uint32_t L, const float* p, uint32_t* ss,
                                    uint8_t* level, float* score);
/* The same with the thresholds chosen by pseudo-expected accuracy (DESIGN.md section 27;
 * dafs_hip_consensus_structures_auto has the contract) from the candidates cand[ncand]. */
#define DAFS_HIP_MAX_CANDIDATES 16u
int dafs_hip_nussinov_decode_auto(dafs_hip_ctx* ctx, uint32_t nlevels, uint32_t ncand, const float* cand, uint32_t L, const float* p,
                                  uint32_t* ss, uint8_t* level, float* score, uint32_t* chosen, uint64_t* sum_p, uint64_t* tp,
                                  uint32_t* npairs, uint64_t* cand_tp, uint32_t* cand_pairs);

/* ------------------------------------------------------------------------------------------
 * L1: fused guide-tree node solver.
 * One call solves a batch of independent nodes: for each, average the base-pairing and matching
 * probabilities of the two child alignments (src/dafs.cpp:513-607, no alifold term), enumerate the
 * consensus base pairs, and run the whole dual-decomposition loop on the device
 * (DAFS::solve_by_dd, src/dafs.cpp:1006-1295).  Uses the context's current stores (after
 * dafs_hip_consistency when that was called).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  uint32_t n1, n2;        /* rows (sequences) of the two child alignments                     */
  uint32_t len1, len2;    /* their column counts                                              */
  const uint32_t* seq1;   /* [n1] sequence index of each row                                  */
  const uint32_t* seq2;   /* [n2]                                                             */
  const uint8_t* mask1;   /* [n1*len1] 1 = residue, 0 = gap (the reference's vector<bool>)    */
  const uint8_t* mask2;   /* [n2*len2]                                                        */
  const float* p_x;       /* optional [len1*len1]: base-pairing matrix of alignment 1 to use in   */
  const float* p_y;       /* optional [len2*len2]  place of the averaged one (--bp-update: the matrices
                             re-estimated by dafs_hip_update_basepairing, dafs.cpp:919-934); NULL = average */
} dafs_node_input;

typedef struct {
  uint32_t* x;            /* [len1] common structure of alignment 1 (may be NULL)             */
  uint32_t* y;            /* [len2] (may be NULL)                                             */
  uint32_t* z;            /* [len1] column of alignment 2 aligned to each column of 1         */
  float score;            /* value solve_by_dd returns (s_prev)                               */
  uint32_t ncbp, iterations, violated; /* dafs.cpp:1292 log line                             */
} dafs_node_output;

typedef struct {
  float w;                /* -w    default 4.0 */
  float eta0;             /* --eta default 0.5 */
  float th_a;             /* -u    default 0.01 */
  float th_s;             /* -t    default 0.2 */
  uint32_t t_max;         /* -m    default 600 */
  int force_iters;        /* bench only: ignore the violated==0 exit (never for parity runs)  */
  int skip_uncoupled_folds; /* default 0 = solve_by_dd as it is.  1: a node with no consensus base pair (ncbp == 0:
                             nothing couples its three subproblems, one pass, no multiplier ever moves) runs the
                             alignment DP only; x and y come back empty and score holds the alignment part.  For
                             callers that consume z alone, as DAFS::align_alignments does (dafs.cpp:896-912).  */
} dafs_dd_params;
void dafs_hip_dd_default_params(dafs_dd_params* p);
int dafs_hip_solve_nodes(dafs_hip_ctx* ctx, uint32_t nnodes, const dafs_node_input* in, const dafs_dd_params* prm,
                         dafs_node_output* out);

/* The same solver with the nodes resident on the device, so that the progressive phase needs no level
 * barrier: open the nodes whose children are ready, advance all open nodes by at most max_iterations
 * subgradient iterations per call (one launch), collect the finished ones, open their parents, repeat.
 * Replaces the recursion of DAFS::align (reference src/dafs.cpp:983-1004) as the driver of
 * DAFS::align_alignments / solve_by_dd.  Results are those of dafs_hip_solve_nodes, bit for bit.        */
int dafs_hip_nodes_open(dafs_hip_ctx* ctx, uint32_t nnodes, const dafs_node_input* in, const dafs_dd_params* prm, uint32_t* handles);
int dafs_hip_nodes_advance(dafs_hip_ctx* ctx, uint32_t n, const uint32_t* handles, const dafs_dd_params* prm, uint32_t max_iterations,
                           uint8_t* finished);
/* One round in a single call: the n_old open nodes advance while the n_new nodes whose children have just finished are
 * opened and started beside them on a second stream (their handles come back in new_handles).  Every node runs at most
 * max_iterations iterations and, when budget_us > 0, stops at the first iteration end past budget_us microseconds after
 * the round began, late starters included.  Results are those of the calls above, bit for bit.                          */
int dafs_hip_nodes_round(dafs_hip_ctx* ctx, uint32_t n_new, const dafs_node_input* in, uint32_t* new_handles, uint32_t n_old,
                         const uint32_t* old_handles, const dafs_dd_params* prm, uint32_t max_iterations, uint32_t budget_us,
                         uint8_t* finished_old, uint8_t* finished_new);
int dafs_hip_nodes_result(dafs_hip_ctx* ctx, uint32_t handle, dafs_node_output* out);
/* The plan nodes_open gives a node of len1 x len2 columns under the solver's environment switches (DAFS_HIP_DD_*), read as
 * it reads them: the LDS forms of its workgroup and of its split folders, the bytes each needs, the score copies it carves. */
typedef struct {
  uint32_t lds_flags, fold_fast, nw_w;  /* as in the device descriptor (dafs_amd/csrc/dd.h)                                 */
  uint32_t lds, split_lds;              /* dynamic LDS bytes of the node's workgroup; of a split launch (0 = never split)   */
  uint32_t s_x, s_y, s_xs, s_ys;        /* 1 = the node carves this score copy (sweep order x / y, by span x / y)          */
} dafs_dd_node_plan;
int dafs_hipk_dd_node_plan(uint32_t len1, uint32_t len2, dafs_dd_node_plan* out);
/* 32-bit words of dynamic LDS the solver's layout gives a node's workgroup (role 0, lds_flags) or its x / y folder
 * (role 1 / 2, the folder's form in fold_fast).                                                                        */
uint32_t dafs_hipk_dd_lds_words(uint32_t len1, uint32_t len2, uint32_t lds_flags, uint32_t fold_fast, int role);
/* The plan the CONTRAfold launch gives a batch whose longest sequence has max_len residues, under the kernel's environment
 * switches (DAFS_HIP_CF_*), read as the launch reads them.  static_lds: bytes of k_contrafold's static LDS; 0 = ask the
 * runtime, 28 KB where it does not answer, as the launch does.  DAFS_HIP_ETOOLONG where the launch refuses.               */
typedef struct {
  uint32_t threads, cell_waves;    /* workgroup size; wavefronts the cells of a span are dealt to                            */
  uint32_t use_ring;               /* 1 = the LDS ring of the 33 most recent spans of FC / FCo                               */
  uint32_t pool_floats, pool_bufs; /* term pool: floats in all (0 = none), 2 = two halves filled beside the cells, else 1    */
  uint32_t lds;                    /* dynamic LDS bytes of the launch                                                        */
  uint32_t static_lds;             /* the static size the plan was made for (static_lds, or what 0 resolved to)              */
} dafs_contrafold_plan;
int dafs_hipk_contrafold_plan(uint32_t max_len, uint32_t static_lds, dafs_contrafold_plan* out);
/* A read-only copy of one array that the set-up kernels of dafs_hip_nodes_open / dafs_hip_nodes_round wrote for a resident
 * node (tests; nothing in a run calls it).  The node's streams are drained first.  p_*: the matrices solve_by_dd starts from;
 * *_PTR / *_COL / *_K: row pointers (rows + 1 words) and entries of the lists of p_x, p_y (cells above the cut-off, j > i), p_z
 * and c_z (cells of z in a consensus base pair); *_MAP: per dense cell its entry or -1 (ZMAP: into the c_z list); ENV:
 * 2 * (len1 + 1) words; ENV4: 2 * (len1 + 130) words, written by the node's first iteration, not by the set-up; CBP_CNT: a word
 * per entry of p_x -- its consensus pairs, and from the fill on (nodes with at least one pair) their running total; CBP: 8
 * words per consensus base pair (i j k l, entry of p_x, entry of p_y, c_z entries of (i, k) and (j, l)), bytes_out / 32 pairs.
 * DAFS_HIP_EINVAL, with dst and bytes_out untouched and the context usable, for a handle that names no node holding its
 * memory (unknown, in a launch, or given back by dafs_hip_nodes_result), an unknown `what`, a capacity below the array's
 * bytes, or CBP of a node opened without its folding arrays (skip_uncoupled_folds and no consensus pair).                 */
enum {
  DAFS_PEEK_P_X = 0, DAFS_PEEK_P_Y, DAFS_PEEK_P_Z, DAFS_PEEK_X_PTR, DAFS_PEEK_X_COL, DAFS_PEEK_X_MAP, DAFS_PEEK_Y_PTR, DAFS_PEEK_Y_COL,
  DAFS_PEEK_Y_MAP, DAFS_PEEK_PZ_PTR, DAFS_PEEK_PZ_K, DAFS_PEEK_CZ_PTR, DAFS_PEEK_CZ_K, DAFS_PEEK_ZMAP, DAFS_PEEK_ENV, DAFS_PEEK_ENV4,
  DAFS_PEEK_CBP_CNT, DAFS_PEEK_CBP
};
int dafs_hip_node_peek(dafs_hip_ctx* ctx, uint32_t handle, int what, void* dst, uint64_t capacity_bytes, uint64_t* bytes_out);
int dafs_hip_nodes_close(dafs_hip_ctx* ctx);
/* Device memory of the resident nodes (diagnostics): bytes reserved from the device, bytes held by open nodes now, and
 * the largest value the latter has had.  A node's memory is returned when dafs_hip_nodes_result has copied it out. */
int dafs_hip_nodes_memory(dafs_hip_ctx* ctx, uint64_t* reserved, uint64_t* in_use, uint64_t* peak);
/* Split-mode nodes whose folding workgroups did not show up in time and that went on in the one-workgroup form since the
 * last dafs_hip_nodes_close (diagnostics: results are unaffected, the run is slower; 0 on an undisturbed device). */
int dafs_hip_nodes_demotions(dafs_hip_ctx* ctx, uint32_t* n);
/* Final common structure of an alignment (src/dafs.cpp:1857-1871 without the RNAalifold term):
 * averaged base-pairing matrix -> SparseNussinov::decode(p,ss,str) with threshold th. */
int dafs_hip_consensus_structure(dafs_hip_ctx* ctx, uint32_t n, uint32_t len, const uint32_t* seq, const uint8_t* mask,
                                 float th, uint32_t* ss, float* score, float* p_out);
/* The same for nalign alignments in one call: alignment a has n_rows[a] rows of len[a] columns; seq
 * holds the rows' sequence indices of all alignments one after another, mask their n_rows[a] * len[a] bytes, ss their len[a]
 * entries; score[nalign] may be NULL.  Alignment a's results are, bit for bit, those of dafs_hip_consensus_structure on its
 * rows in the same order.  Rows of different alignments may belong to different families, and a sequence to many alignments.
 * Everything is checked before the first launch: DAFS_HIP_EINVAL leaves ss and score untouched.  nalign = 0 does nothing.
 * The alignments run in chunks under a budget of device memory (dafs_host_structures_batch_bytes; DAFS_HIP_CS_BATCH_BYTES
 * overrides it), which does not change any result. */
int dafs_hip_consensus_structures(dafs_hip_ctx* ctx, uint32_t nalign, const uint32_t* n_rows, const uint32_t* len, const uint32_t* seq,
                                  const uint8_t* mask, float th, uint32_t* ss, float* score);
/* A consensus structure that may hold pseudoknots, decoded level by level; laid out as
 * dafs_hip_consensus_structures, with th[nlevels], level (the len[a] bytes of every alignment one after another; may be NULL)
 * and score[nalign * nlevels] (may be NULL).  Level 0 is the decode of dafs_hip_consensus_structures at th[0], bit for bit.
 * Level k >= 1 is the same decoder at th[k] on the averaged matrix with every cell set to 0 that has a column paired at a
 * lower level or that crosses no pair of some lower level; levels above an empty one are empty and score 0.  ss is the union
 * of the levels, level[i] the pair's level at both of its columns and 0xFF at unpaired ones.  Each level is one of IPknot's
 * (reference src/ipknot.cpp:145-206) given the lower ones; its stacking constraints (:209-247) and its joint optimum over
 * the levels are not part of this.  Checks and chunks as in dafs_hip_consensus_structures; also DAFS_HIP_EINVAL for nlevels
 * outside 1..DAFS_HIP_MAX_LEVELS or th[k] <= 0 at a k >= 1.  DAFS_HIP_EINVAL leaves the outputs untouched. */
int dafs_hip_consensus_structures_levels(dafs_hip_ctx* ctx, uint32_t nalign, const uint32_t* n_rows, const uint32_t* len,
                                         const uint32_t* seq, const uint8_t* mask, uint32_t nlevels, const float* th, uint32_t* ss,
                                         uint8_t* level, float* score);
/* The same decode with every level's threshold chosen from cand[ncand] by pseudo-expected accuracy, as
 * CentroidAlifold and IPknot choose theirs.  cand: 1 <= ncand <= DAFS_HIP_MAX_CANDIDATES thresholds, strictly decreasing, each
 * inside (0, 1).  Every cell counts as the integer q(p) = (uint64_t)(fminf(fmaxf(p, 0), 1) * 2^30) and every sum is a sum of
 * those in uint64, so no floating-point rounding takes part in a choice.  S is the sum of q over the cells i < j of the
 * averaged matrix; a structure has T, the sum of q over its pairs, and n, their number, and its pseudo-expected F is
 * 2 T / (n 2^30 + S).  (Ta, na) beats (Tb, nb) when Ta (nb 2^30 + S) > Tb (na 2^30 + S) in 128-bit integers.  Level k: every
 * candidate is decoded on the level's masked matrix (the decoder, its ties and its score are those of the call above) and
 * valued with the levels already kept added in; the first candidate in list order that no earlier one equals or beats is the
 * best; the level is its structure when that beats the levels already kept alone, else the level is empty, and so is every
 * higher one.  ss, level and score[nalign * nlevels] are those of dafs_hip_consensus_structures_levels at the thresholds
 * cand[chosen[0 .. m - 1]] of the m kept levels (the scores of the others are 0; m = 0: all unpaired).  Per alignment, one
 * after another, each may be NULL: chosen[nlevels] (the candidate's index, DAFS_HIP_NONE for an empty level), sum_p[1] (S),
 * tp[nlevels] and npairs[nlevels] (T and n of each kept level alone, 0 for an empty one), and the whole table
 * cand_tp / cand_pairs[nlevels * ncand] (level-major; 0 for the levels that were not decoded).  Checks and chunks as above
 * (dafs_host_structure_auto_bytes is the estimate); DAFS_HIP_EINVAL, outputs untouched, also for nlevels outside
 * 1..DAFS_HIP_MAX_LEVELS, ncand outside 1..DAFS_HIP_MAX_CANDIDATES and a list that is not as described. */
int dafs_hip_consensus_structures_auto(dafs_hip_ctx* ctx, uint32_t nalign, const uint32_t* n_rows, const uint32_t* len, const uint32_t* seq,
                                       const uint8_t* mask, uint32_t nlevels, uint32_t ncand, const float* cand, uint32_t* ss,
                                       uint8_t* level, float* score, uint32_t* chosen, uint64_t* sum_p, uint64_t* tp, uint32_t* npairs,
                                       uint64_t* cand_tp, uint32_t* cand_pairs);

/* DAFS::update_basepairing_probability (src/dafs.cpp:609-712; options --bp-update and --bp-update1), without the RNAalifold
 * term: the sequences of the alignment (rows seq / mask as in dafs_node_input) are folded again with CONTRAfold under the
 * constraint the common structure ss (ss[i] = j for the left partner, DAFS_HIP_NONE otherwise, as the decoders return it)
 * puts on each of them, and the constrained posteriors are averaged; p_out receives the len x len matrix. */
int dafs_hip_update_basepairing(dafs_hip_ctx* ctx, uint32_t n, uint32_t len, const uint32_t* seq, const uint8_t* mask,
                                const uint32_t* ss, float* p_out);

/* Reliability of an alignment (no counterpart in the reference; definitions in DESIGN.md "Alignment reliability").  Rows
 * seq / mask as in dafs_node_input: n distinct sequences of one family (else DAFS_HIP_EINVAL), each mask row placing every
 * residue of its sequence.  ss: the consensus structure over the len columns in the decoders' convention (ss[c] = right
 * partner at the left column, DAFS_HIP_NONE otherwise; every column in at most one pair), or NULL for no pairs.
 * mp_relaxed / bp_relaxed: 0 = the un-relaxed store (with -f the four-way result), 1 = the relaxed one, negative = the
 * store the progressive phase reads now; the matching store must be valid and hold every pair of the context, or every pair
 * of these rows when it is a listed one (not needed for n = 1), the base-pairing store must be valid when ss is given, and no
 * folding may be in flight.  Every sum is taken in double, rows in ascending sequence order, so
 * the order of the given rows changes no bit.  Outputs (host; any may be NULL):
 *   res_rel[sum of the rows' lengths]  rel(r, i): the rows in the given order, residues in sequence order (1.0 for n = 1)
 *   col_rel[len]                       mean of rel over the residues of each column (0 for a column of gaps)
 *   pair_rel[len], pair_rows[len]      at the left column of each pair of ss: the mean of bp[x](i, j) over the rows that
 *                                      hold both residues, and their number; 0 elsewhere
 *   expected_accuracy                  mean of rel over all residues */
int dafs_hip_alignment_reliability(dafs_hip_ctx* ctx, uint32_t n, uint32_t len, const uint32_t* seq, const uint8_t* mask,
                                   const uint32_t* ss, int mp_relaxed, int bp_relaxed, double* res_rel, double* col_rel,
                                   double* pair_rel, uint32_t* pair_rows, double* expected_accuracy);
/* The same for nalign alignments in one call, laid out as in dafs_hip_consensus_structures (n_rows, len,
 * seq, mask) and dafs_hip_structure_support (ss: the len[a] entries of every alignment one after another, or NULL for no pairs
 * anywhere).  Rows of different alignments may belong to different families and a sequence may sit in many alignments.
 * want: one byte per row, nonzero = compute its residue values; NULL = every row.  Outputs (host; any may be NULL):
 *   res_rel            the residues of all rows one after another, rows in the given order; the entries of a row that is not
 *                      wanted are left untouched
 *   col_rel, pair_rel, pair_rows   the len[a] entries of every alignment one after another
 *   expected_accuracy[nalign]
 * col_rel and expected_accuracy of an alignment with a row that is not wanted are NaN.  Every value that is computed equals, bit
 * for bit, what dafs_hip_alignment_reliability returns for that alignment's rows, which is this call with nalign = 1.
 * The matching store (needed by an alignment of more than one row) must be valid and whole, or a relaxed store of
 * dafs_hip_consistency_match_pairs whose list holds every pair (x, y) with x a wanted row and y another row of x's alignment.
 * The alignments run in chunks under a budget of device memory (dafs_host_reliability_batch_bytes; DAFS_HIP_REL_BATCH_BYTES
 * overrides it), three launches per chunk; the chunking changes no result.  DAFS_HIP_EINVAL before any launch (outputs
 * untouched, context usable): a row count or length of 0, an unknown sequence, a sequence twice in one alignment, rows of two
 * families in one alignment, a mask that does not place every residue of its sequence, a bad ss, an invalid or partial store, a
 * needed pair that a listed store does not hold, or a folding in flight. */
int dafs_hip_alignment_reliabilities(dafs_hip_ctx* ctx, uint32_t nalign, const uint32_t* n_rows, const uint32_t* len, const uint32_t* seq,
                                     const uint8_t* mask, const uint32_t* ss, const uint8_t* want, int mp_relaxed, int bp_relaxed,
                                     double* res_rel, double* col_rel, double* pair_rel, uint32_t* pair_rows, double* expected_accuracy);

/* How far every row of an alignment keeps a given structure, for nalign alignments laid out as in
 * dafs_hip_consensus_structures (n_rows, len, seq, mask), ss holding their len[a] entries one after another (the convention
 * of dafs_hip_alignment_reliability).  Per row r (sequence x), over the pairs c1 -> c2 of its alignment's ss in ascending c1,
 * with i, j the residues of r at the two columns (outputs [sum of n_rows], rows in the given order; any may be NULL):
 *   both       pairs of which the row holds both residues
 *   canonical  those of `both` whose residues CONTRAfold can pair (dafs_host_fold_complementary)
 *   half       pairs of which the row holds exactly one residue
 *   expected   the sum over the `both` pairs of bp[x](i, j) from the base-pairing store the progressive phase reads now, 0 for
 *              a pair that is not stored; each term widened to double and added in ascending c1, no contraction
 * DAFS_HIP_EINVAL before any launch (outputs untouched, context usable): a row count or length of 0, an unknown sequence, a
 * mask that does not place every residue of its sequence, a bad ss, an invalid store or a folding in flight.  The call reads
 * no matching store, so a relaxed matching store that holds listed pairs only (dafs_hip_consistency_match_pairs) is no
 * obstacle. */
int dafs_hip_structure_support(dafs_hip_ctx* ctx, uint32_t nalign, const uint32_t* n_rows, const uint32_t* len, const uint32_t* seq,
                               const uint8_t* mask, const uint32_t* ss, uint32_t* both, uint32_t* canonical, uint32_t* half,
                               double* expected);

/* Covariation statistics of an alignment (no counterpart in the reference; definitions, to the bit, in DESIGN.md section 13
 * "Covariation").  The call reads the alignment and the structure alone, none of the context's stores.
 *   code[n * len]  row-major, one byte per cell: A 0, C 1, G 2, U/T 3, everything else (gaps, N, IUPAC) 4
 *   ss             the consensus structure as in dafs_hip_alignment_reliability, or NULL
 *   shuffles, seed the null: `shuffles` alignments whose columns are each permuted on their own (counter-based generator
 *                  from `seed`); 0 = no null, every E is NaN
 * For columns c1 != c2: n_ab = rows with base a at c1 and b at c2; Gq = 2 * sum n_ab * (LNQ[n_ab] + LNQ[m] - LNQ[r_a] -
 * LNQ[s_b]) with LNQ[k] = floor(log(k) * 65536 + 0.5), an exact int64 (the G statistic in 2^-16 nats); R(c) = sum of Gq(c, .),
 * T = sum of R; S(c1, c2) = (Gq - R(c1) * R(c2) / T * (len / (len - 1))) / 65536 in double, in that order (average-product
 * correction); E(s) = number of (shuffle, c1 < c2) with a shuffled S >= s, divided by `shuffles`: the expected number of
 * column pairs that reach s by chance under a null that ignores phylogeny.  Outputs (host; any may be NULL):
 *   col_sum[len], total                 R and T
 *   best[len], best_score[len], best_e[len]   per column the partner with the largest S (the smallest such column), that S, its E
 *   pair_score[len], pair_e[len], pair_rows[len], pair_canonical[len], pair_types[len]
 *                                       at the left column of each pair of ss: S, E, m, the rows holding AU UA GC CG GU UG and
 *                                       how many of those six occur; 0 elsewhere
 *   g[len * len]                        the whole Gq matrix (small alignments, tests)
 * DAFS_HIP_EINVAL: n or len 0, a code above 4, a bad ss, n > 2^20 or n * len^2 > 2^45 (T then fits an int64); the context
 * stays usable.  With n < 2 or len < 2 everything is 0, best is DAFS_HIP_NONE, E is 0 (NaN for shuffles = 0), without a launch. */
int dafs_hip_alignment_covariation(dafs_hip_ctx* ctx, uint32_t n, uint32_t len, const uint8_t* code, const uint32_t* ss,
                                   uint32_t shuffles, uint64_t seed, int64_t* col_sum, uint32_t* best, double* best_score,
                                   double* best_e, double* pair_score, double* pair_e, uint32_t* pair_rows,
                                   uint32_t* pair_canonical, uint32_t* pair_types, int64_t* total, int64_t* g);
/* The same statistics under a chosen null ("Null by evolution along a tree").  dafs_hip_alignment_covariation
 * is this call with DAFS_COV_NULL_SHUFFLE and no tree, to the bit.
 *   null                    DAFS_COV_NULL_SHUFFLE: every column permuted on its own, which ignores phylogeny.
 *                           DAFS_COV_NULL_TREE: the rows are the leaves of a tree; Fitch parsimony places every column's
 *                           substitutions on its branches, and null alignment k evolves from the root's states with every
 *                           branch keeping its number of substitutions, on columns drawn afresh per (k, branch) by a stateless
 *                           permutation.  Gaps (code 4) stay where they are.  All of it is integer arithmetic.
 *   tree_left, tree_right   2n-1 entries each in the layout of dafs_host_build_tree (leaf r is row r; the children of join n + t
 *                           are earlier nodes; the root is 2n-2), or both NULL under DAFS_COV_NULL_TREE: average linkage
 *                           (dafs_hip_linkage_tree) of sim(r, s) = (float)((double)ident / (double)both), ident and both counted
 *                           over the columns where both rows hold a base (0.0f where there is none); that takes n <= 32768.
 * DAFS_HIP_EINVAL with a message in dafs_hip_last_error, outputs untouched and the context usable, beyond the refusals above: an
 * unknown null, a tree under DAFS_COV_NULL_SHUFFLE, only one of the two arrays, a malformed tree (the checks of
 * dafs_host_cluster_cut), and under the default tree a row without a base.  With n < 2, len < 2 or shuffles = 0 the call behaves
 * as above: no tree is built and none of the tree null's kernels is launched (a tree that is passed is still checked). */
enum { DAFS_COV_NULL_SHUFFLE = 0, DAFS_COV_NULL_TREE = 1 };
int dafs_hip_alignment_covariation_null(dafs_hip_ctx* ctx, uint32_t n, uint32_t len, const uint8_t* code, const uint32_t* ss,
                                        uint32_t shuffles, uint64_t seed, int null, const int32_t* tree_left, const int32_t* tree_right,
                                        int64_t* col_sum, uint32_t* best, double* best_score, double* best_e, double* pair_score,
                                        double* pair_e, uint32_t* pair_rows, uint32_t* pair_canonical, uint32_t* pair_types,
                                        int64_t* total, int64_t* g);
/* Null alignment k (0-based) of either null as out_code[n * len], the codes the statistics above are computed from: what a user
 * looks at to see what the null keeps, and what the tests compare byte for byte.  Arguments and refusals as above; one row comes
 * back as it is. */
int dafs_hip_covariation_null_alignment(dafs_hip_ctx* ctx, uint32_t n, uint32_t len, const uint8_t* code, int null,
                                        const int32_t* tree_left, const int32_t* tree_right, uint64_t seed, uint32_t k,
                                        uint8_t* out_code);

/* Alignment statistics: how similar the rows of an alignment are to one another (no counterpart in the reference; definitions,
 * to the bit, in DESIGN.md section 18 "Alignment statistics").  Both device calls read the alignment alone, none of the
 * context's stores, and work on a context on which no sequences were set.
 *   cell[n * len]  row-major, one byte per cell: A 0, C 1, G 2, U/T 3, any other letter 4 (a residue that matches nothing),
 *                  a gap 5 (dafs_host_ali_code)
 *   use[len]       the columns that count, or NULL: all of them.  Everything below sees used columns only.
 *   cand[n]        the rows that may be somebody's nearest, or NULL: every row
 * res(r) = cells of r with code <= 4; aligned(r, s) = columns where both have code <= 4; ident(r, s) = columns where both codes
 * are equal and <= 3; den = min(res(r), res(s)); pid = (double)ident / (double)den.  (i1, d1) is more identical than (i2, d2)
 * iff i1 * d2 > i2 * d1 in uint64.  nearest(r) = the s != r with cand[s] of the most identical (ident, den), the smallest s
 * among equals, DAFS_HIP_NONE without a candidate (nearest_ident and nearest_den are then 0).  red(r, s) <=> (double)ident >=
 * nr_threshold * (double)den, one multiplication and one comparison in double.  Outputs (host; any may be NULL):
 *   res[n]
 *   ident[n * n], aligned[n * n]        the whole matrices (n <= 32768); diagonal: the cells of r with code <= 3, and res(r)
 *   nearest[n], nearest_ident[n], nearest_den[n]
 *   red[n * ceil(n / 32)]               bit s % 32 of word s / 32 of row r = red(r, s), the diagonal and the padding 0
 *                                       (n <= 65536); with nr_threshold = 0 it is not computed and not written
 * DAFS_HIP_EINVAL before any launch (outputs untouched, context usable): n or len 0 or above 2^20, a code above 5, a row
 * without a residue in the used columns, nr_threshold outside [0, 1], a matrix beyond its limit. */
int dafs_hip_alignment_identity(dafs_hip_ctx* ctx, uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use,
                                const uint8_t* cand, double nr_threshold, uint32_t* res, uint32_t* ident, uint32_t* aligned,
                                uint32_t* nearest, uint32_t* nearest_ident, uint32_t* nearest_den, uint32_t* red);
/* Henikoff position-based weights in Easel's form, in double and in this order: k_c(a) = rows with code
 * a in column c (a = 0..4), t_c = how many a have k_c(a) > 0; v_r = the running sum over the used columns c, ascending, where r
 * has a code <= 4, of 1.0 / (double)(t_c * k_c(code)); u_r = v_r / (double)res(r); U = the running sum of u_r, r ascending;
 * weight[r] = (u_r * (double)n) / U.  n = 1: 1.0 without a launch.  Refusals as above. */
int dafs_hip_alignment_weights(dafs_hip_ctx* ctx, uint32_t n, uint32_t len, const uint8_t* cell, const uint8_t* use, double* weight);
/* The non-redundant subset (host code) from the bit matrix `red` of dafs_hip_alignment_identity.  The
 * rows are visited in the order rank[0], rank[1], ... (a permutation of 0..n-1, else DAFS_HIP_EINVAL with a message in
 * dafs_hip_last_error).  A row with forced[r] != 0 (NULL: none) is always kept; any other row is kept iff it is redundant with
 * no row kept before it.  kept[n]: 1 or 0; by[n]: the first kept row, in visiting order, that removes r, DAFS_HIP_NONE for a
 * kept row. */
int dafs_host_nr_select(uint32_t n, const uint32_t* red, const uint32_t* rank, const uint8_t* forced, uint8_t* kept, uint32_t* by);
/* What both drivers say when they refuse a combination of the alignment statistics' options */
enum {
  DAFS_ALISTAT_NO_PAIRWISE = 0, /* identity statistics asked of pairwise alignments */
  DAFS_ALISTAT_NR_NEEDS_MERGED, /* a non-redundant subset without the merged alignment */
  DAFS_ALISTAT_NR_THRESHOLD,    /* a threshold outside (0, 1] */
  DAFS_ALISTAT_TOO_MANY_ROWS    /* the summary needs the identity matrix: more than 32768 rows */
};
const char* dafs_host_alistat_refusal(int which);
/* The cell code of a character for the two calls above; 255 for a character that is neither a letter nor '-' or '.' */
uint8_t dafs_host_ali_code(char ch);
/* Average, minimum and maximum pid over the pairs r < s into summary[3]: the average a running double
 * sum with r ascending, then s ascending, divided by the number of pairs; minimum and maximum by the integer order.  n = 1:
 * three NaN.  ident is the n x n matrix, res as returned. */
int dafs_host_identity_summary(uint32_t n, const uint32_t* ident, const uint32_t* res, double* summary);
/* The --identity table: the line "# rows n columns len average A min B max C", then per row r the line "r+1 name residues
 * weight nearest+1 nearest_name pid", tab-separated, floats as %.9g, "nan" for a NaN; a row without a nearest row has "0",
 * "-" and "nan" in the last three fields. */
int dafs_host_identity_table(uint32_t n, uint32_t len, const char* const* names, const uint32_t* res, const double* weight,
                             const uint32_t* nearest, const uint32_t* nearest_ident, const uint32_t* nearest_den,
                             const double* summary, char** table);
/* The --identity-matrix table, one line per pair r < s as dafs_host_pairwise_table lays its pairs out: "r+1 s+1 names[r]
 * names[s] ident aligned den pid" */
int dafs_host_identity_matrix_table(uint32_t n, const char* const* names, const uint32_t* res, const uint32_t* ident,
                                    const uint32_t* aligned, char** table);
/* A Stockholm block with one "#=GS <name> WT <%.6f>" line per row directly after its "#=GF" lines (after "# STOCKHOLM 1.0"
 * when it has none); every other byte of `block` is kept. */
int dafs_host_stockholm_weights(const char* block, uint32_t n, const char* const* names, const double* weight, char** out);
/* The non-redundant block of a merged alignment: `block` (dafs_host_stockholm_block_merged over the n
 * rows `names`, the first nseed of them the seed's) without the row and the "#=GR" lines of every row with kept[r] = 0, and
 * with the line "#=GF CC nr <threshold as %.9g> kept K of M hits" after "# STOCKHOLM 1.0" (M = n - nseed, K of them kept).
 * Nothing else changes: columns that become all-gap stay, and so do the "#=GC" lines. */
int dafs_host_stockholm_nr(const char* block, uint32_t n, const char* const* names, const uint8_t* kept, uint32_t nseed,
                           double threshold, char** out);
/* dafs_host_seed_table_support with two more columns at the end: the Stockholm name of the seed row nearest to the sequence
 * (nearest_name[j], "-" for none) and its identity as %.9g.  Both NULL: the table of dafs_host_seed_table_support. */
int dafs_host_seed_table_nearest(uint32_t n, const char* const* headers, const uint32_t* length, const uint32_t* matched,
                                 const double* score, const int64_t* iterations, const uint32_t* both, const uint32_t* canonical,
                                 const uint32_t* half, const double* expected, const char* const* nearest_name,
                                 const double* identity, char** table);

/* Alignment comparison: how far two alignments of the same n >= 2 sequences agree (no counterpart in the reference;
 * definitions, to the integer, in DESIGN.md section 19 "Comparing two alignments").  R is the reference (len_r columns), T the
 * test (len_t columns).  The call reads the two alignments alone, none of the context's stores, and works on a context on which
 * no sequences were set.  Inputs (host):
 *   cell_r[n * len_r], cell_t[n * len_t]  cells in the codes of dafs_host_ali_code; row r of both holds the same residue codes
 *                                         in the same order
 *   use_r[len_r], use_t[len_t]            the columns that are aligned, or NULL: all of them
 *   ss_r[len_r], ss_t[len_t]              structures as dafs_host_seed_clean_structure gives them (the partner at the left
 *                                         column of a pair, DAFS_HIP_NONE elsewhere; the symmetric form, with the left column
 *                                         at the right one, is taken too), or NULL: no structure part (it needs both)
 *   pp[n * len_t]                         per cell of T the PP class 0..10 ('0'..'9', '*'), 255 for none, or NULL: no PP part
 * For residue k of row r, a = its column in R if use_r has it, else none; b = the same in T.  k_c = residues with a = c, m_d =
 * residues with b = d, cnt(c, d) = residues with a = c and b = d.  refn = k_a - 1, testn = m_b - 1, shr = cnt(a, b) - 1, each 0
 * where a key it needs is none.  Outputs (host; any may be NULL, and only the kernels that a non-NULL output needs are run): */
typedef struct {
  uint32_t* residues;                    /* [n] residues of the row */
  uint64_t *shared, *refp, *testp;       /* [n] the sums of shr, refn, testn over the row's residues */
  double *sps, *ppv;                     /* [n] (double)shared / (double)refp and / (double)testp; NaN for a denominator of 0 */
  uint64_t* total;                       /* [3] half the sums over the rows of shared, refp, testp */
  double* score;                         /* [3] SPS and PPV of the totals, TC = tc[0] / tc[1]; NaN for a denominator of 0 */
  uint32_t *k, *m;                       /* [len_r] k_c, [len_t] m_d */
  uint64_t *colref, *colshared;          /* [len_r] k_c (k_c - 1) / 2; the sum over d of cnt(c, d) (cnt(c, d) - 1) / 2 */
  uint8_t* reproduced;                   /* [len_r] 1 iff k_c >= 2 and some d has cnt(c, d) = k_c = m_d */
  uint64_t* tc;                          /* [2] reproduced columns, columns with k_c >= 2 */
  uint32_t *pair_shared, *pair_refp, *pair_testp; /* [n * n], n <= 16384: for r != s the residue pairs of the two rows with
                                            equal a and equal b, with equal a, with equal b (none is never equal); symmetric,
                                            the diagonal 0; row r sums to shared[r], refp[r], testp[r] */
  uint64_t* pp_count;                    /* [3 * 11], needs pp: per class q the residues [q], the sum of refn [11 + q] and of
                                            shr [22 + q] */
  uint64_t *tp, *nref, *ntest;           /* [n], need ss_r and ss_t (the masks play no part): the pairs of residues of the row
                                            whose R columns are partners in ss_r (nref), whose T columns are in ss_t (ntest),
                                            and those in both (tp) */
  uint64_t* ss_total;                    /* [3] the sums over the rows of tp, nref, ntest */
} dafs_compare_out;
/* DAFS_HIP_EINVAL before any launch (outputs untouched, context usable): n < 2 or above 2^20; a length of 0 or above 2^20;
 * len_r * len_t above 2^30; a pair matrix with n above 16384; a code above 5; a PP class that is neither 0..10 nor 255; a
 * structure with a partner beyond its length, a column in two pairs or a one-sided right column; a structure output with one
 * of ss_r and ss_t missing or pp_count without pp; and a row whose residue codes differ between R and T, which
 * dafs_hip_last_error() then names.  DAFS_CMP_CHUNK_COLS and DAFS_CMP_BAND_BLOCKS shrink the pair
 * pass's LDS stage and its launches for tests and change no result. */
int dafs_hip_alignment_compare(dafs_hip_ctx* ctx, uint32_t n, uint32_t len_r, uint32_t len_t, const uint8_t* cell_r,
                               const uint8_t* cell_t, const uint8_t* use_r, const uint8_t* use_t, const uint32_t* ss_r,
                               const uint32_t* ss_t, const uint8_t* pp, const dafs_compare_out* out);

/* Host text of the comparison.  What both drivers say when they refuse a combination of its options: */
enum {
  DAFS_COMPARE_NEEDS_REF = 0,   /* one of --compare and --compare-ref without the other */
  DAFS_COMPARE_NEEDS_COMPARE,   /* --compare-columns or --compare-matrix without --compare */
  DAFS_COMPARE_NO_PAIRWISE,     /* a comparison asked of pairwise alignments */
  DAFS_COMPARE_NEEDS_MERGED,    /* a comparison of --seed-each placements without the merged alignment */
  DAFS_COMPARE_TOO_MANY_ROWS    /* the pair table with more than 16384 rows */
};
const char* dafs_host_compare_refusal(int which);
/* The rows to compare: the names (the first word of each string, as a Stockholm file names a row) present in both alignments,
 * in the reference's order.  ref_row[k] and test_row[k] (room for
 * min(n_ref, n_test) entries each) are the rows of the k-th common name, *count their number.  Refused (DAFS_HIP_EINVAL, message
 * in dafs_hip_last_error): a name on two rows of either alignment, fewer than two common names. */
int dafs_host_compare_match(uint32_t n_ref, const char* const* ref_names, uint32_t n_test, const char* const* test_names,
                            uint32_t* count, uint32_t* ref_row, uint32_t* test_row);
/* The "#=GR <name> PP" lines of the first alignment of a Stockholm file, read beside dafs_host_seed_parse / _clean: per row of
 * the file, in its order, the PP characters over the columns that dafs_host_seed_clean keeps, joined by '\n'; a row without a
 * PP line is all '.'.  *has_pp = 0 when the file holds no PP line (aligned FASTA never does).  Refused: what the seed reader
 * refuses, a PP line that names no row or has another length than the rows. */
int dafs_host_seed_pp(const char* text, size_t bytes, uint32_t* n, int* has_pp, char** pp);
/* The --compare table of n compared rows (only_ref / only_test: rows of one alignment alone, which were left out).  Lines:
 *   "# rows n only_ref x only_test y columns_ref len_r columns_test len_t"
 *   "# pairs shared S ref P test Q sps A ppv B"
 *   "# columns reproduced K of M tc C"
 *   with tp: "# structure tp .. ref .. test .. sensitivity .. ppv .. f .." (the sums of tp, nref, ntest)
 *   with pp_count: per class with residues "# pp <class character> residues ref shared accuracy"
 *   per row, tab-separated: "r+1 name residues shared ref test sps ppv", then "tp nref ntest" with tp
 * Floats as %.9g, "nan" for a NaN.  The arrays are those of dafs_compare_out; tp / nref / ntest and pp_count may be NULL. */
int dafs_host_compare_table(uint32_t n, const char* const* names, uint32_t only_ref, uint32_t only_test, uint32_t len_r,
                            uint32_t len_t, const uint32_t* residues, const uint64_t* shared, const uint64_t* refp,
                            const uint64_t* testp, const uint64_t* total, const uint64_t* tc, const uint64_t* tp,
                            const uint64_t* nref, const uint64_t* ntest, const uint64_t* pp_count, char** table);
/* The --compare-columns table: per column of the reference "c+1 residues colref colshared reproduced" (residues = k_c,
 * reproduced 1 or 0), tab-separated */
int dafs_host_compare_columns_table(uint32_t len_r, const uint32_t* k, const uint64_t* colref, const uint64_t* colshared,
                                    const uint8_t* reproduced, char** table);
/* The --compare-matrix table, one line per pair r < s as dafs_host_identity_matrix_table lays its pairs out: "r+1 s+1 names[r]
 * names[s] shared ref test sps ppv" */
int dafs_host_compare_matrix_table(uint32_t n, const char* const* names, const uint32_t* pair_shared, const uint32_t* pair_refp,
                                   const uint32_t* pair_testp, char** table);

/* ---- device-resident exchange of the sparse stores (multi-GPU runs) ---------------------------------------------------
 * One process per GPU shards phase 1 of DAFS::run (src/dafs.cpp:1787-1827): the folds (src/fold.cpp:66-67), the pair jobs
 * (src/align.cpp:46-50) and the output pairs of relax_matching_probability (src/dafs.cpp:265-315) are independent.  The
 * shards travel by all-gather over RCCL; these entry points move a store to and from DEVICE buffers of the context's own
 * device in the layouts of dafs_hip_mp_fetch / dafs_hip_bp_fetch, so nothing goes through host memory.  Every pointer
 * argument is device memory except where noted.
 *   dafs_hip_mp_export_dev   pairs [first, first + count) of the store's own pair order (an un-relaxed shard computed by
 *                            dafs_hip_align_posteriors(pair_begin, pair_end) numbers its pairs from 0; the relaxed store
 *                            keeps the global row-major index): nnz[count], the pairs' relative row pointers, their entries
 *                            (col / val, capacity cap_entries), and for relaxed = 0 the similarity scores sim[count].
 *                            n_rowptr / n_entries (host) receive what was written.
 *   dafs_hip_mp_install_dev  the whole store from arrays of all N(N-1)/2 pairs in row-major order (dafs_hip_mp_install's
 *                            arguments, on the device); n_entries = entries in col / val = 2 * sum of nnz.
 *   dafs_hip_bp_export_dev   the un-relaxed base-pairing store, sequences in input order (dafs_hip_bp_fetch's layout).
 *   dafs_hip_set_bp_dev      the un-relaxed base-pairing store from nblocks = N blocks in any order: block k holds the rows
 *                            of sequence seq_of_block[k] (host array); rowptr / col / val are the blocks' arrays concatenated
 *                            in block order -- what the ranks' exports look like after the gather.
 * DAFS_HIP_EINVAL: a range beyond the store's pairs (first > npairs or count > npairs - first), sim with relaxed = 1, a relaxed
 * install without an un-relaxed store, an n_entries that is not what the counts (mp) or the blocks' last row pointers (bp) add
 * up to, nblocks != N, a sequence named twice or beyond N.  DAFS_HIP_EOVERFLOW: cap_entries below the entries of the range (of
 * the store, for bp).  A refused export writes nothing into the caller's buffers; an install refused for its n_entries or for
 * the sequences its blocks name leaves the store it was to fill invalid until a correct one (dafs_hip_mp_install_dev checks
 * the total only, dafs_hip_mp_install every pair's row pointers).  count = 0 is no error and writes nothing. */
int dafs_hip_mp_export_dev(dafs_hip_ctx* ctx, int relaxed, uint64_t first, uint64_t count, uint32_t* nnz, uint32_t* rowptr, uint32_t* col, float* val,
                           float* sim, uint64_t cap_entries, uint64_t* n_rowptr, uint64_t* n_entries);
int dafs_hip_mp_install_dev(dafs_hip_ctx* ctx, int relaxed, const uint32_t* nnz, const uint32_t* rowptr, const uint32_t* col, const float* val,
                            const float* sim, uint64_t n_entries);
int dafs_hip_bp_export_dev(dafs_hip_ctx* ctx, uint32_t* rowptr, uint32_t* col, float* val, uint64_t cap_entries, uint64_t* n_rowptr, uint64_t* n_entries);
int dafs_hip_set_bp_dev(dafs_hip_ctx* ctx, uint32_t nblocks, const uint32_t* seq_of_block, const uint32_t* rowptr, const uint32_t* col, const float* val,
                        uint64_t n_entries);

/* ---- all-against-all pairwise runs (dafs --pairwise, pipeline.pairwise) ----
 * dafs_hip_pairs_from fills dst with the npairs two-sequence families [pair_x[p], pair_y[p]] (host arrays, x < y < N) of the
 * N sequences of src: dst row 2p is sequence pair_x[p], row 2p + 1 is pair_y[p], family p holds rows 2p and 2p + 1.  src must
 * hold one family of N >= 2 sequences with its raw stores complete (dafs_hip_fold_posteriors, or _begin/_end, and
 * dafs_hip_align_posteriors of the whole pair set; no transform run on it).  dst receives the raw base-pairing rows of its
 * sequences, per family its pair's raw mp[x][y] and transpose and the similarity block [[1, s_xy], [s_xy, 1]]: the state
 * dafs_hip_set_sequences + dafs_hip_set_families + dafs_hip_fold_posteriors + dafs_hip_align_posteriors leave for that input,
 * bit for bit, by device-to-device gathers (no recomputation).  The transforms, node rounds and decoders then run on dst
 * unchanged.  src is not modified, so calls with different pair chunks may follow one another.  DAFS_HIP_EINVAL: contexts on
 * different devices (or the same context), src with more than one family, missing or partial stores, a folding in flight,
 * a pair with x >= y or y >= N. */
int dafs_hip_pairs_from(dafs_hip_ctx* dst, const dafs_hip_ctx* src, uint32_t npairs, const uint32_t* pair_x, const uint32_t* pair_y);
/* The same gather for arbitrary families (dafs --seed-each, pipeline.add_each): dst becomes nfam
 * families, family f holding the sequences member[first[f] .. first[f + 1]) of src (host arrays; first[0] = 0, no empty
 * family, members strictly ascending within a family, so that a dst pair is the src pair in the same orientation).  A sequence
 * may be a member of many families; a family of one has no pair and the similarity block [[1]].  src: one family of N
 * sequences with its base-pairing store and an un-relaxed matching store that covers a row-major prefix [0, n_tasks) of its
 * pairs (dafs_hip_align_posteriors(ctx, model, th, 0, pair_end); the whole set is the special case): every pair a family needs
 * must lie in it.  The pairs (x, y) with x < m are the ids below m N - m (m + 1) / 2.  dst's sequences, families, raw stores
 * (un-relaxed, pair p = task p) and similarity blocks are, bit for bit, those of a context built directly on the listed
 * sequences with that partition, dafs_hip_fold_posteriors and dafs_hip_align_posteriors.  src is not modified.
 * DAFS_HIP_EINVAL (dst left usable): null or equal contexts or different devices, src with more than one family, a missing
 * store, a folding in flight on either context, nfam = 0, first[0] != 0, an empty family, a member >= N or not ascending, a
 * pair that is not in src's store.  DAFS_HIP_EOVERFLOW: more than 2^31 dst sequences or pairs. */
int dafs_hip_families_from(dafs_hip_ctx* dst, const dafs_hip_ctx* src, uint32_t nfam, const uint32_t* first, const uint32_t* member);

/* ---- phase 1 of DAFS::run on one rank of a multi-GPU run (src/dafs.cpp:1787-1827) ----
 * One process per GPU; every rank has called dafs_hip_set_sequences with all N sequences.  Rank r folds the sequences
 * x = r (mod world) (independent per sequence, src/fold.cpp:66-67), computes the pair posteriors and similarity scores of
 * the r-th contiguous range of the row-major pair enumeration (dafs_hip_pair_range; independent per pair,
 * src/align.cpp:46-50) and relax_matching_probability's output pairs of the same range (src/dafs.cpp:265-315); after each of
 * the three pieces the shards are packed on the device, all-gathered by `allgather` and installed, so that on return the
 * context is in the state a single-GPU phase 1 (fold_posteriors, align_posteriors, consistency) leaves it in, bit for
 * bit, on every rank.  The base-pairing transform is replicated.  Not for the aux-file inputs or the four-way transform.
 *
 * dafs_allgather_fn: gather `bytes` bytes from every rank (send, device memory) into recv (device memory, world * bytes,
 * rank order) -- ncclAllGather's contract.  The collective may be enqueued on hip_stream (a hipStream_t of the context's
 * device); the library waits for that stream before it reads recv.  Non-zero return = failure (DAFS_HIP_ECOMM). */
typedef int (*dafs_allgather_fn)(void* user, const void* send, void* recv, size_t bytes, void* hip_stream);
void dafs_hip_pair_range(uint64_t npairs, uint32_t world, uint32_t rank, uint64_t* begin, uint64_t* end);
int dafs_hip_phase1_sharded(dafs_hip_ctx* ctx, uint32_t rank, uint32_t world, int align_model, float th_a, float w_pct_a, float w_pct_s,
                            int fold_model, float fold_th, dafs_allgather_fn allgather, void* user);

/* ---- measurement aid: device time per kernel (bench.py's "stages") ----
 * dafs_hip_stage_timing(ctx, 1) makes every kernel launch of the library record a pair of HIP events on its stream
 * (one context per process at a time); dafs_hip_stage_report waits for the device, adds the elapsed times up per kernel and
 * starts the next interval; dafs_hip_stage_timing(ctx, 0) switches it off.  `ms` of kernels that ran beside others on
 * different streams overlap: they are per-kernel durations, not a partition of the wall-clock. */
typedef struct {
  const char* kernel;   /* kernel name as in the rocprofv3 kernel trace (template arguments left out) */
  double ms;            /* sum over the launches of the interval */
  double longest_ms;    /* the longest single launch */
  uint32_t launches;
} dafs_stage_time;
int dafs_hip_stage_timing(dafs_hip_ctx* ctx, int enable);
int dafs_hip_stage_report(dafs_hip_ctx* ctx, dafs_stage_time* out, uint32_t cap, uint32_t* n);

#ifdef __cplusplus
}
#endif
#endif
