// dafs_amd/csrc/stage.h -- per-kernel device timings for bench.py's "stages" object (dafs_hip_stage_timing /
// dafs_hip_stage_report).  When a context has switched the recorder on, every launcher brackets its kernel with a pair
// of HIP events on the stream it launches on; the report adds up the elapsed times per kernel.  Off (the default) the
// scopes cost one pointer test.  One recorder per process at a time: measurement aid, not part of the data path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>

namespace dafs {

enum stage_id {
  ST_CONTRAFOLD = 0, ST_CF_POSTERIOR, ST_BP_COMPACT, ST_PAIRHMM3, ST_PAIRHMM5, ST_MP_SIM, ST_MP_INTERLEAVE, ST_PCT_ROWS, ST_PCT_EMIT,
  ST_PCT_BP_ROWS, ST_PCT_BP_EMIT, ST_FOURWAY_ROWS, ST_NODE_AVG, ST_NODE_LISTS, ST_NODE_CBP_FILL, ST_DD_SOLVE, ST_NODE_PACK,
  ST_NUSSINOV_SINGLE, ST_NW_SINGLE, ST_REL_POS, ST_REL_RESIDUE, ST_REL_COLUMN, ST_COV_PACK, ST_COV_SHUFFLE, ST_COV_SUMS, ST_COV_TOTAL,
  ST_COV_BEST, ST_COV_ARG, ST_COV_NULL, ST_COV_SS, ST_NUSSINOV_BATCH, ST_SS_SUPPORT,
  ST_ALI_PACK, ST_ALI_MATRIX, ST_ALI_NEAREST, ST_ALI_RED, ST_ALI_NEAREST_COUNTS, ST_ALI_TRANSPOSE, ST_ALI_COUNT, ST_ALI_COLUMNS, ST_ALI_ROW_WEIGHTS,
  ST_CMP_MAP, ST_CMP_COUNT_COLS, ST_CMP_COUNT, ST_CMP_RESIDUE, ST_CMP_COLUMNS, ST_CMP_SS, ST_CMP_PAIRS, ST_CMP_PAIRS_OCC,
  ST_LINKAGE_INIT, ST_LINKAGE_JOINS, ST_COV_FITCH, ST_COV_DRAW, ST_COV_EVOLVE,
  ST_NJ_INIT, ST_NJ_ROWSUM, ST_NJ_PICK, ST_NJ_UPDATE, ST_BOOT_PACK, ST_BOOT_DIST, ST_NJ_BATCH,
  ST_STRUCT_SIM, ST_STRUCT_W, ST_LEVELS_MASK, ST_LEVELS_MERGE, ST_BP_COMPACT_LEVELS, ST_PEA_TOTAL, ST_PEA_PICK,
  ST_TRANSFER_SIDES, ST_TRANSFER, ST_COUNT
};
static const char* const kStageNames[ST_COUNT] = {
  "k_contrafold", "k_contrafold_posterior", "k_bp_compact", "k_pairhmm3", "k_pairhmm5", "k_mp_sim", "k_mp_interleave", "k_pct_rows", "k_pct_emit",
  "k_pct_bp_rows", "k_pct_bp_emit", "k_fourway_rows", "k_node_avg", "k_node_lists", "k_node_cbp_fill", "k_dd_solve", "k_node_pack",
  "k_nussinov_single", "k_nw_single", "k_rel_pos", "k_rel_residue", "k_rel_column", "k_cov_pack", "k_cov_shuffle", "k_cov_pairs<sums>",
  "k_cov_total", "k_cov_pairs<best>", "k_cov_pairs<arg>", "k_cov_pairs<null>", "k_cov_ss", "k_nussinov_batch", "k_ss_support",
  "k_ali_pack", "k_ali_pairs<matrix>", "k_ali_pairs<nearest>", "k_ali_pairs<red>", "k_ali_nearest_counts", "k_ali_transpose", "k_ali_count", "k_ali_columns",
  "k_ali_row_weights",
  "k_cmp_map", "k_cmp_count_cols", "k_cmp_count", "k_cmp_residue", "k_cmp_columns", "k_cmp_ss", "k_cmp_pairs<shared>", "k_cmp_pairs<occupancy>",
  "k_linkage_init", "k_linkage_joins", "k_cov_fitch", "k_cov_draw", "k_cov_evolve",
  "k_nj_init", "k_nj_rowsum", "k_nj_pick", "k_nj_update", "k_boot_pack", "k_boot_dist", "k_nj_batch",
  "k_struct_sim", "k_struct_w", "k_levels_mask", "k_levels_merge", "k_bp_compact_levels", "k_pea_total", "k_pea_pick",
  "k_transfer_sides", "k_transfer"};

struct stage_recorder {
  struct rec { int id; hipEvent_t a, b; };
  std::vector<rec> recs;
  std::vector<hipEvent_t> pool;  // events of earlier reports, reused
  hipEvent_t take() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  void clear() { for (rec& r : recs) { pool.push_back(r.a); pool.push_back(r.b); } recs.clear(); }
  void release() { clear(); for (hipEvent_t e : pool) if (e) (void)hipEventDestroy(e); pool.clear(); }
};

stage_recorder*& stage_current();  // capi.cpp: the recorder that is switched on, or null

struct stage_scope {
  stage_recorder* r;
  hipStream_t st;
  hipEvent_t b = nullptr;
  bool go = true;  // STAGE_LAUNCH: the bracketed statement runs once
  stage_scope(int id, hipStream_t s) : r(stage_current()), st(s) {
    if (!r) return;
    hipEvent_t a = r->take();
    b = r->take();
    if (!a || !b) { r = nullptr; return; }
    (void)hipEventRecord(a, st);
    r->recs.push_back({id, a, b});
  }
  ~stage_scope() { if (r) (void)hipEventRecord(b, st); }
};

}  // namespace dafs

// brackets the next statement (a kernel launch on stream st) with the recorder's events
#define STAGE_LAUNCH(id, st) for (dafs::stage_scope stage_s_(id, st); stage_s_.go; stage_s_.go = false)
