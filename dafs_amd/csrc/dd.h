// dafs_amd/csrc/dd.h -- device-side descriptors of the progressive phase (dd.hip):
// one dd_node per guide-tree node being solved, all pointers into device memory.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sparse_view.h"

namespace dafs {

struct nuss_ws {      // SparseNussinov work arrays for one problem of size L
  float* dp;          // L*L
  uint32_t* tr;       // L*L
  uint32_t* ck;       // L*L  candidate list of column j at ck[j*L ..], insertion order (k descending)
  float* cv;          // L*L
  uint32_t* cc;       // L    candidates per column
};

// One child alignment of a node and the folding of its columns.  A node has two, f[0] = x and f[1] = y, indexed like
// dd_lds::f and dd_fold_form; everything over a folding is written once and takes this.
struct dd_fold {
  uint32_t n, L;      // rows (sequences) and columns of the child alignment
  // per row the sequence index, per (row, column) the residue rank or NONE, and per (row, residue) its column
  const uint32_t *seq, *rank, *idx, *idxoff;
  float *p, *q;       // L*L each: averaged base-pairing posteriors (dafs.cpp:561-607) and Lagrange multipliers
  nuss_ws w;
  uint8_t* trb;       // L(L+1)/2: Nussinov traceback codes 0..4 (HBM copy)
  uint32_t* trk;      // L*L: bifurcation code of the cells whose traceback code is 4
  float* s;           // (L+63)*ceil(L/64)*64: pair scores w*(p-th)-q in sweep order of the folding DP; null when the
                      // folding has no register form (more than DD_WFOLD columns per lane)
  float* s_span;      // L*Lp (Lp = L rounded up to 64): the same scores stored by span, S[(j-i)*Lp + i], for the span form
                      // (nuss_wave_span); null when no launch of this node can take that form
  // sparse structure of p (> CUTOFF, upper triangle) and of the consensus base pairs
  int32_t* map;       // dense cell -> entry id or -1
  uint32_t *ptr, *col;  // row pointers and columns of the entries
  uint8_t* cflag;     // per entry: part of a consensus base pair (c_x / c_y, dafs.cpp:1038-1039)
  int32_t* tc;        // per entry violation counter
  uint32_t* ss;       // result: per column its partner or NONE
};

struct dd_node {
  dd_fold f[2];
  // averaged matching posteriors of the alignment z of the two (dafs.cpp:513-559) and its Lagrange multipliers: f[0].L x f[1].L
  float *p_z, *q_z;
  float* nw_edge;     // 2*(L1+2): the last column of a panel of the alignment DP, for the next panel (nw_wave_reg)
  uint8_t* tr_z;      // panels*(L1+1)*512: traceback codes of the alignment DP when they are not packed in LDS -- a 64-bit slot per (panel, row, lane)
  uint32_t nw_w;      // columns per lane of the alignment DP (dd_nw_cols; DAFS_HIP_DD_WIDE=1 makes it 1): second alignments beyond
                      // 64*nw_w - 1 columns run as panels of 64*nw_w columns; also the layout of pz_s / qz_s (nw_idx)
  float *pz_s, *qz_s;       // panels*(L1+63)*nw_w*64 each: p_z, q_z in sweep order of the alignment DP, panel by panel
  uint32_t lds_flags;       // LDS plan of the node's own workgroup: kLds* below (dd_node_lds lays it out)
  uint32_t* env;      // 2*(L1+1)
  uint32_t* env4;     // 2*(L1+130): the same envelope for the register-resident alignment DP -- {max(first,1), second} of row r at
                      // index r + 64, the empty range {1, 0} for the 64 rows before row 1 and the 65 behind row L1 (no clamping, no selects)
  // sparse structure of p_z (> CUTOFF) and of the cells of z in a consensus base pair (c_z)
  int32_t* zmap;                  // dense cell -> entry id (cz lists) or -1
  uint32_t *pz_ptr, *pz_k, *cz_ptr, *cz_k;
  uint8_t* cz_flag;
  uint32_t* cbp_cnt;              // per entry of f[0]
  uint32_t* cbp;                  // 8 per consensus base pair: i j k l, entry of f[0], entry of f[1], zid1 zid2
  uint32_t ncbp_cap;
  int32_t* tz;                    // per cz entry violation counter
  float* sw;                      // ncbp: positive s_w, compacted in cbp order
  // results (the foldings: f[r].ss)
  uint32_t* z;
  float* score;                   // [1]
  uint32_t* info;                 // [16]: ncbp, iterations (next iteration while paused), violated, status, slow-x, slow-y,
                                  //       started, paused; [8..13] optional phase ticks
  float* fstate;                  // [4]: c, eta, previous dual value of a paused node
  // split mode: the two folding DPs of this node run on workgroups of their own (blockIdx.y = 1, 2) next to
  // the leader (blockIdx.y = 0, alignment DP + constraints + updates); sync[0] go / exit, [1] x done, [2] y done,
  // [3] [4] the folding scores.  fold_fast: the form of each folder, kFold* below (dd_fold_form / dd_fold_k read it).
  uint32_t* sync;
  uint32_t split, fold_fast;
};
// k_dd_solve keeps the node in LDS beside its dynamic regions: kDdLdsBudget assumes this static part
static_assert(sizeof(dd_node) <= 568, "dd_node must not grow");

struct dd_params {
  float w, eta0, th_a, th_s;
  uint32_t t_max;
  int force_iters;
  int stamps;  // accumulate per-phase timing into info[8..13] (tuning aid)
  int skip_xy; // dafs_dd_params::skip_uncoupled_folds
  int span_one_wave;       // DAFS_HIP_DD_SPAN_MW=0 (tests, tuning): the folders keep the span form on one wavefront
  int debug_lose_folders;  // DAFS_HIP_DD_LOSE_FOLDERS=1 (tests): the leader of a split node treats its folders as lost at once
  uint32_t slice;  // at most this many iterations per launch (0 = run to the end); a node that is cut short is
                   // marked paused and continues from where it stopped at the next launch
  // A second bound on a launch, in time: a node also pauses at the first iteration end past `budget` ticks (100 MHz,
  // wall_clock64) after the reference tick -- its workgroup's own start, or, when t_ref is given, the tick the round's
  // first launch left there (t_ref_write: this launch is the one that leaves it), so that launches started at different
  // moments of a round stop together (dafs_hip_nodes_round).  0 = no time bound.
  unsigned long long budget;
  unsigned long long* t_ref;
  int t_ref_write;
};

int dd_avg_launch(const dd_node* d_nodes, uint32_t nnodes, uint32_t max_len, mp_store_dev mp, bp_store_dev bp, int one_row, int coop, hipStream_t st);
int dd_lists_launch(const dd_node* d_nodes, uint32_t nnodes, uint32_t max_len1, dd_params prm, uint32_t* d_ncbp, hipStream_t st);  // d_ncbp[b]: consensus pairs of node b
int dd_cbp_fill_launch(const dd_node* d_nodes, uint32_t nnodes, uint32_t max_len1, dd_params prm, hipStream_t st);
#define DD_WREG 8     // widest lane (columns) of the register-resident alignment DP, and of the folding DP with its codes in LDS
#define DD_WFOLD 16   // widest lane of the register-resident folding DP (codes in HBM beyond DD_WREG)
#define DD_WNW 16     // widest lane of the register-resident alignment DP with its codes packed in LDS (second alignments up to 1023 columns)
#define DD_WNWG 32    // widest lane of the same DP with its codes in HBM, one 64-bit slot per row and lane (up to 2047 columns)
// columns per lane of the alignment DP, which is also the layout of its sweep-order inputs (nw_skew): beyond DD_WNW the
// register form exists for multiples of four only
static inline __host__ __device__ uint32_t dd_nw_cols(uint32_t L2) {
  const uint32_t W = (L2 + 64) / 64;
  return W > DD_WNWG ? DD_WNWG : (W > DD_WNW ? (W + 3) & ~3u : W);
}
static inline __host__ __device__ uint32_t dd_nw_panels(uint32_t L2, uint32_t W) { return (L2 + 64 * W) / (64 * W); }  // columns 0 .. L2
#define DD_CAP 4  // candidates per column kept in LDS by the fast folding DP
// LDS words of the in-flight rows of a fast folding DP: one row of L values per active lane (the lanes own
// ceil(L/64) columns each, so ceil(L / that) of them are at work).  The previous-row buffers and candidate counters of
// the HBM-table form borrow the same words when that form has to run (the ring is idle then), hence the floor.
// Columns per lane of the folding wave DPs.  Up to 512 columns all 64 lanes are used; from there to 768 only 48, so
// that the rows in flight (one per lane at work, L values each) still fit LDS and the register form can run with up
// to DD_WFOLD columns per lane; wider alignments use 64 lanes again and the HBM-table form.
static inline __host__ __device__ uint32_t dd_fold_cols(uint32_t L) { return (L > 512 && L <= 768) ? (L + 47) / 48 : (L + 63) / 64; }
static inline __host__ __device__ uint32_t dd_ring_rows(uint32_t L) { const uint32_t W = dd_fold_cols(L); return W ? (L + W - 1) / W : 0; }
static inline __host__ __device__ uint32_t dd_slow_words(uint32_t L) { return 2 * dd_fold_cols(L) * 64 + L; }
static inline __host__ __device__ uint32_t dd_ring_words(uint32_t L) {
  const uint32_t a = dd_ring_rows(L) * L, b = dd_slow_words(L);
  return a > b ? a : b;
}
// Span form of a folding DP (dd.hip, nuss_wave_span): packed codes, the whole dp triangle, DD_CAP candidate values and
// row offsets for each of L + 1 columns (16-byte slots), DD_CAP split rows per column.  Each part starts on 16 bytes.
#define DD_SPAN_LMAX 256  // four row slots per lane
static inline __host__ __device__ uint32_t dd_span_nib_words(uint32_t L) { return (uint32_t)((((size_t)L * (L + 1) / 2 + 7) / 8 + 3) & ~(size_t)3); }
static inline __host__ __device__ uint32_t dd_span_tri_words(uint32_t L) { return (uint32_t)(((size_t)L * (L + 1) / 2 + 3) & ~(size_t)3); }
// workgroup form of the folding DP beyond the register forms (nuss_wg_span): three rolling rows of dp values, the candidate
// counters, and the first K candidates (key, value) of every column
static inline __host__ __device__ uint32_t dd_wg_words(uint32_t L, uint32_t K) { return (4 + 2 * K) * ((L + 3) & ~3u); }
static inline __host__ __device__ uint32_t dd_span_words(uint32_t L) { return dd_span_nib_words(L) + dd_span_tri_words(L) + 2 * DD_CAP * (L + 1) + DD_CAP * L; }
// packed traceback table of the alignment DP: two bits per cell, rows padded to whole 32-bit words (16 cells), so that the
// bit position of a lane's cells within their word is the same in every row
static inline __host__ __device__ uint32_t dd_nwtab_row_words(uint32_t L2) { return (L2 + 1 + 15) / 16; }
static inline __host__ __device__ uint32_t dd_nwtab_words(uint32_t L1, uint32_t L2) { return (L1 + 1) * dd_nwtab_row_words(L2); }
static const size_t kDdLdsBudget = 156 * 1024;  // dynamic LDS of k_dd_solve (the CU has 160 KB; ~2.2 KB is static)

// The forms of a node's folding and alignment DPs (the host's plan_node chooses them).  dd_node::lds_flags, what the
// node's workgroup keeps in LDS: the packed alignment codes; the register forms of x and y side by side; one region for both
// (x, then y), with the codes in HBM too; the span form of both side by side.
constexpr uint32_t kLdsNwTab = 1u, kLdsFastX = 2u, kLdsFastY = 4u, kLdsShared = 8u, kLdsSharedHbm = 16u, kLdsSpanXY = 64u;
// dd_node::fold_fast, the form of each folder r (0 = x, 1 = y) of a split node, at bit r of: the register form, the same
// with its codes in HBM, the span form, the workgroup form nuss_wg_span (no register form); and that form's K
// (candidates per column in LDS) at bits 8 + 4r ..
constexpr uint32_t kFoldReg = 1u, kFoldRegHbm = 4u, kFoldSpan = 16u, kFoldWg = 64u, kFoldKShift = 8, kFoldKMask = 15u;
static inline __host__ __device__ uint32_t dd_fold_form(uint32_t fold_fast, uint32_t r) { return (fold_fast >> r) & (kFoldReg | kFoldRegHbm | kFoldSpan | kFoldWg); }
static inline __host__ __device__ uint32_t dd_fold_k(uint32_t fold_fast, uint32_t r) { return (fold_fast >> (kFoldKShift + 4 * r)) & kFoldKMask; }
static inline __host__ __device__ uint32_t dd_fold_bits(uint32_t r, uint32_t form, uint32_t K) { return (form << r) | (K << (kFoldKShift + 4 * r)); }

// The dynamic LDS of k_dd_solve (dd_node_lds) and of a split node's folder (dd_folder_lds): word offsets of each region from
// the base, which is first rounded up to 16 bytes when align16 (16-byte candidate slots; `end` counts the three words this
// may take).  The host sizes its plans by `end`, the kernels carve by the offsets (dd_lds_at).
constexpr uint32_t kDdNoLds = 0xFFFFFFFFu;  // region absent
struct dd_fold_lds {  // a folding DP: packed codes, rows in flight, split rows (span form: candidate heads), span triangle,
                      // candidate values and row offsets, traceback stack, workgroup-form rows
  uint32_t trb = kDdNoLds, ring = kDdNoLds, lck = kDdNoLds, tri = kDdNoLds, cv = kDdNoLds, ck = kDdNoLds, stk = kDdNoLds, wg = kDdNoLds;
};
struct dd_lds { dd_fold_lds f[2]; uint32_t trz = kDdNoLds, end = 0; bool align16 = false; };  // f: x, y (a folder: f[0]); trz: alignment codes
static inline __host__ __device__ uint32_t dd_code_words(uint32_t L) { return (uint32_t)(((size_t)L * (L + 1) / 2 + 7) / 8); }
static inline __host__ __device__ void dd_span_lds(dd_fold_lds& f, uint32_t& w, uint32_t L) {
  f.trb = w; w += dd_span_nib_words(L); f.tri = w; w += dd_span_tri_words(L);
  f.cv = f.stk = w; w += DD_CAP * (L + 1); f.ck = w; w += DD_CAP * (L + 1); f.lck = w; w += DD_CAP * L;  // stack: dead values
}
static inline __host__ __device__ void dd_reg_lds(dd_fold_lds& f, uint32_t& w, uint32_t codes, uint32_t ring, uint32_t lck) {
  if (codes) { f.trb = w; w += codes; }
  f.ring = f.stk = w; w += ring; f.lck = w; w += lck;  // stack: the ring, idle by then
}
static inline __host__ __device__ dd_lds dd_node_lds(uint32_t L1, uint32_t L2, uint32_t flags) {
  dd_lds m; uint32_t w = 0;
  m.align16 = (flags & kLdsSpanXY) != 0;
  if (m.align16) { dd_span_lds(m.f[0], w, L1); dd_span_lds(m.f[1], w, L2); }
  if (flags & kLdsNwTab) { m.trz = w; w += dd_nwtab_words(L1, L2); }
  if (flags & kLdsFastX) dd_reg_lds(m.f[0], w, dd_code_words(L1), dd_ring_words(L1), DD_CAP * L1);
  if (flags & kLdsFastY) dd_reg_lds(m.f[1], w, dd_code_words(L2), dd_ring_words(L2), DD_CAP * L2);
  const uint32_t c1 = dd_code_words(L1), c2 = dd_code_words(L2), r1 = dd_ring_words(L1), r2 = dd_ring_words(L2);
  if (flags & kLdsShared) { dd_reg_lds(m.f[0], w, (flags & kLdsSharedHbm) ? 0 : (c1 > c2 ? c1 : c2), r1 > r2 ? r1 : r2, DD_CAP * (L1 > L2 ? L1 : L2)); m.f[1] = m.f[0]; }
  m.end = w + (m.align16 ? 4 : 0); return m;
}
static inline __host__ __device__ dd_lds dd_folder_lds(uint32_t L, uint32_t form, uint32_t K) {
  dd_lds m; uint32_t w = 0;
  m.align16 = (form & (kFoldSpan | kFoldWg)) != 0;
  if (form & kFoldSpan) dd_span_lds(m.f[0], w, L);
  else if (form & (kFoldReg | kFoldRegHbm)) dd_reg_lds(m.f[0], w, (form & kFoldReg) ? dd_code_words(L) : 0, dd_ring_words(L), DD_CAP * L);
  else if (form & kFoldWg) { m.f[0].wg = w; w += dd_wg_words(L, K); }
  m.end = w + (m.align16 ? 4 : 0); return m;
}
static inline __device__ uint32_t* dd_lds_at(unsigned char* s, const dd_lds& m, uint32_t off) {
  uint32_t* b = (uint32_t*)(m.align16 ? (((uintptr_t)s + 15) & ~(uintptr_t)15) : (uintptr_t)s);
  return off == kDdNoLds ? nullptr : b + off;
}
int dd_pack_launch(const dd_node* d_nodes, uint32_t nnodes, const uint32_t* d_off, uint32_t* d_out, hipStream_t st);
int dd_solve_launch(const dd_node* d_nodes, uint32_t nnodes, dd_params prm, size_t lds_bytes, bool split, uint32_t* d_paused, hipStream_t st);
// standalone decoders on dense device matrices (one workgroup each)
int nussinov_launch(uint32_t L, const float* p, const float* q, float w, float th, nuss_ws ws, uint32_t* ss, float* score, hipStream_t st);
// One alignment of a batched decode (k_nussinov_batch, one workgroup each): the standalone decoder's arguments without q.
// form: the candidates per column that nuss_wg_span keeps in LDS (4 / 2 / 0), or 0xFFFFFFFF for the span-ordered form on
// global tables -- per alignment what nussinov_launch chooses for its width, so both give the same table and structure.
struct cs_desc {
  uint32_t L, form;
  const float* p;  // L*L
  nuss_ws ws;
  uint32_t* ss;    // L
  float* score;    // [1]
};
uint32_t nussinov_form(uint32_t L, size_t* lds_bytes);  // the form of an alignment of L columns and its dynamic LDS
// descs[0..n): alignments of one size class -- `threads` per workgroup, lds_bytes >= every member's
int nussinov_batch_launch(const cs_desc* d_descs, uint32_t n, float th, uint32_t threads, size_t lds_bytes, hipStream_t st);
// One alignment of a level-by-level decode (levels.hip): what k_levels_merge and k_levels_mask read.
// key[c] after level k's merge: kLvPaired where column c is in a pair of level k, else the left column of the innermost
// level-k pair that strictly encloses c, or 0xFFFFFFFF.  Two columns free at level k are the ends of a cell that crosses a
// level-k pair exactly when their keys differ.
constexpr uint32_t kLvPaired = 0xFFFFFFFEu;
struct lv_desc {
  uint32_t L, flag_stride;
  float* p;             // L*L: masked in place, level after level
  const uint32_t* lss;  // L: the structure the newest level's decode wrote
  uint32_t* key;        // L
  uint32_t* ss;         // L: the merged structure
  uint8_t* level;       // L: the pair's level at both of its columns, 0xFF elsewhere
  uint32_t* flag;       // flag[k * flag_stride]: 1 when level k has a pair
};
// act[0..n): indices into descs of the alignments that take part.  merge: level k's lss into ss / level (k = 0 initialises
// them), the flag, and with want_key the keys for level k + 1's mask.  mask: zeroes every cell (i, j), i < j, of p that has
// an end paired at the newest level or crosses none of its pairs; max_len >= every member's L.
int levels_merge_launch(const lv_desc* d_descs, const uint32_t* d_act, uint32_t n, uint32_t k, int want_key, hipStream_t st);
int levels_mask_launch(const lv_desc* d_descs, const uint32_t* d_act, uint32_t n, uint32_t max_len, hipStream_t st);
// One alignment of a decode whose thresholds are chosen by pseudo-expected accuracy (pea.hip): what
// k_pea_total and k_pea_pick read and write.  Level k's C candidates decode into css (C arrays of L + 1) and cscore; the
// pick leaves the chosen one in the level's own array lss and its score in score[k], for k_levels_merge to go on from.
struct pea_desc {
  uint32_t L, pad_;
  const float* p;        // L*L: the matrix the level's candidates were decoded from
  const uint32_t* css;   // C*(L+1)
  const float* cscore;   // [C]
  uint32_t* lss;         // L
  float* score;          // [K]
  uint64_t* sum;         // [1]: S, zero before k_pea_total
  uint64_t* base;        // [2]: T and n over the levels kept so far, zero before level 0
  uint64_t* tp;          // [K]
  uint64_t* ctp;         // [K*C]
  uint32_t* chosen;      // [K]
  uint32_t* np;          // [K]
  uint32_t* cnp;         // [K*C]
};
// act[0..n): indices into descs, as above.  total: adds the q of every cell i < j of p to *sum; max_len >= every member's
// L.  pick: level k's choice among ncand candidates.
int pea_total_launch(const pea_desc* d_descs, const uint32_t* d_act, uint32_t n, uint32_t max_len, hipStream_t st);
int pea_pick_launch(const pea_desc* d_descs, const uint32_t* d_act, uint32_t n, uint32_t k, uint32_t ncand, hipStream_t st);
int nussinov_dense_launch(uint32_t L, const float* p, const float* q, float w, float th, float* dp, uint32_t* tr, uint32_t* stack, uint32_t* ss,
                          float* score, hipStream_t st);
int nw_launch(uint32_t L1, uint32_t L2, const float* p, const float* q, float th, uint32_t* env, int compute_env,
              float* dp, uint8_t* tr, uint32_t* al, float* score, hipStream_t st);

}  // namespace dafs
