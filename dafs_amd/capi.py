"""ctypes binding of include/dafs_hip.h (the same entry points a cgo/JNI/C++ shim would bind)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DAFS_HIP_LIB") or os.path.join(_HERE, "libdafs_hip.so")  # DAFS_HIP_LIB: tuning builds

NONE = 0xFFFFFFFF
ALIGN_PROBCONS, ALIGN_CONTRALIGN = 0, 1
E_OVERFLOW = -5


class DafsHipError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise DafsHipError(
            "libdafs_hip.so is not built (%s). Run `python -m dafs_amd.build`; there is no CPU fallback." % LIB_PATH)
    return C.CDLL(LIB_PATH)


lib = _load()

u32p = C.POINTER(C.c_uint32)
f32p = C.POINTER(C.c_float)


class PairTask(C.Structure):
    _fields_ = [("off1", C.c_uint32), ("len1", C.c_uint32), ("off2", C.c_uint32), ("len2", C.c_uint32)]


class PairhmmPlan(C.Structure):
    _fields_ = [("group", C.c_uint32), ("width", C.c_uint32), ("nwaves", C.c_uint32), ("slab_steps", C.c_uint32),
                ("scratch_bytes", C.c_uint64)]


class DdNodePlan(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("lds_flags", "fold_fast", "nw_w", "lds", "split_lds", "s_x", "s_y", "s_xs", "s_ys")]


class ContrafoldPlan(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("threads", "cell_waves", "use_ring", "pool_floats", "pool_bufs", "lds", "static_lds")]


class Pairhmm3Model(C.Structure):
    _fields_ = [("init", C.c_float * 3), ("trans", (C.c_float * 3) * 3), ("match", (C.c_float * 8) * 7),
                ("ins", C.c_float * 8)]


class Pairhmm3Args(C.Structure):
    _fields_ = [("codes", C.c_void_p), ("tasks", C.c_void_p), ("ntasks", C.c_uint32), ("th", C.c_float),
                ("scratch", C.c_void_p), ("queue", C.c_void_p), ("rp_off", C.c_void_p), ("rowptr_pool", C.c_void_p),
                ("ent_col", C.c_void_p), ("ent_val", C.c_void_p), ("pool_top", C.c_void_p), ("pool_cap", C.c_uint64),
                ("pair_off", C.c_void_p), ("pair_nnz", C.c_void_p), ("sim", C.c_void_p), ("status", C.c_void_p),
                ("model", Pairhmm3Model)]


class Pairhmm5Model(C.Structure):
    _fields_ = [("match", (C.c_float * 5) * 5), ("insert", C.c_float * 5), ("single", C.c_float * 5),
                ("pair", (C.c_float * 5) * 5)]


class Pairhmm5Args(C.Structure):
    _fields_ = Pairhmm3Args._fields_[:-1] + [("model", Pairhmm5Model)]


def _sig(name, restype, argtypes):
    f = getattr(lib, name)
    f.restype = restype
    f.argtypes = argtypes
    return f


_strerror = _sig("dafs_hip_strerror", C.c_char_p, [C.c_int])
_last_error = _sig("dafs_hip_last_error", C.c_char_p, [])
_create = _sig("dafs_hip_create", C.c_int, [C.c_int, C.POINTER(C.c_void_p)])
_destroy = _sig("dafs_hip_destroy", None, [C.c_void_p])
_set_sequences = _sig("dafs_hip_set_sequences", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_char_p), u32p])
_set_families = _sig("dafs_hip_set_families", C.c_int, [C.c_void_p, C.c_uint32, u32p])
_align_posteriors = _sig("dafs_hip_align_posteriors", C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_uint64])
_align_result_size = _sig("dafs_hip_align_result_size", C.c_int,
                          [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
_align_fetch = _sig("dafs_hip_align_fetch", C.c_int, [C.c_void_p] + [C.c_void_p] * 7)
_mp_result_size = _sig("dafs_hip_mp_result_size", C.c_int,
                      [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
_mp_fetch = _sig("dafs_hip_mp_fetch", C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 6)
_get_sim = _sig("dafs_hip_get_sim", C.c_int, [C.c_void_p, C.c_void_p])
_similarity = _sig("dafs_hip_similarity", C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.POINTER(C.c_uint64)])
_similarity_ranges = _sig("dafs_host_similarity_ranges", C.c_int, [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)])
_structure_scores = _sig("dafs_hip_structure_scores", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
_similarity_scored = _sig("dafs_hip_similarity_scored", C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_uint64, C.c_int, C.c_float, C.POINTER(C.c_uint64)])
_get_pair_scores = _sig("dafs_hip_get_pair_scores", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p])
structure_score = _sig("dafs_host_structure_score", C.c_float, [C.c_uint64, C.c_uint64, C.c_uint64])
mix_score = _sig("dafs_host_mix_score", C.c_float, [C.c_float, C.c_float, C.c_float])
SCORES = ("sequence", "structure", "mix")  # --cluster-score; the index is the library's DAFS_SCORE_* code
_set_bp = _sig("dafs_hip_set_bp", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
_bp_result_size = _sig("dafs_hip_bp_result_size", C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
_bp_fetch = _sig("dafs_hip_bp_fetch", C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p])
_fold_posteriors = _sig("dafs_hip_fold_posteriors", C.c_int, [C.c_void_p, C.c_int, C.c_float])
_fold_posterior_dense = _sig("dafs_hip_fold_posterior_dense", C.c_int,
                             [C.c_void_p, C.c_char_p, C.c_uint32, C.c_char_p, C.c_void_p, C.POINTER(C.c_float)])
_consistency = _sig("dafs_hip_consistency", C.c_int, [C.c_void_p, C.c_float, C.c_float])
_consistency_match = _sig("dafs_hip_consistency_match", C.c_int, [C.c_void_p, C.c_float])
_consistency_bp = _sig("dafs_hip_consistency_bp", C.c_int, [C.c_void_p, C.c_float])
_fourway_consistency = _sig("dafs_hip_fourway_consistency", C.c_int, [C.c_void_p, C.c_float])
_fold_begin = _sig("dafs_hip_fold_posteriors_begin", C.c_int, [C.c_void_p, C.c_int, C.c_float])
_fold_end = _sig("dafs_hip_fold_posteriors_end", C.c_int, [C.c_void_p])
_fold_constrained_begin = _sig("dafs_hip_fold_posteriors_constrained_begin", C.c_int, [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_char_p)])
_fold_constrained = _sig("dafs_hip_fold_posteriors_constrained", C.c_int, [C.c_void_p, C.c_int, C.c_float, C.POINTER(C.c_char_p)])
_fold_levels_begin = _sig("dafs_hip_fold_posteriors_levels_begin", C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_uint32, C.POINTER(C.c_char_p)])
_fold_levels = _sig("dafs_hip_fold_posteriors_levels", C.c_int, [C.c_void_p, C.c_int, C.c_float, C.c_uint32, C.POINTER(C.c_char_p)])
_structure_support = _sig("dafs_hip_structure_support", C.c_int, [C.c_void_p, C.c_uint32] + [C.c_void_p] * 9)
_pairs_from = _sig("dafs_hip_pairs_from", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, u32p, u32p])
_families_from = _sig("dafs_hip_families_from", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, u32p, u32p])
_consistency_match_pairs = _sig("dafs_hip_consistency_match_pairs", C.c_int, [C.c_void_p, C.c_float, C.c_uint64, C.c_void_p])


class NodeInput(C.Structure):
    _fields_ = [("n1", C.c_uint32), ("n2", C.c_uint32), ("len1", C.c_uint32), ("len2", C.c_uint32),
                ("seq1", C.c_void_p), ("seq2", C.c_void_p), ("mask1", C.c_void_p), ("mask2", C.c_void_p),
                ("p_x", C.c_void_p), ("p_y", C.c_void_p)]


def _node_inputs(nodes):
    """The NodeInput array of nodes (s1, m1, s2, m2) or (s1, m1, s2, m2, p_x, p_y) (one entry at least: an empty list
    passes a valid pointer), and per node the arrays it points into, (s1, s2, m1, m2, p_x, p_y), which must outlive the C
    call."""
    ins = (NodeInput * max(len(nodes), 1))()
    keep = []
    for b, node in enumerate(nodes):  # p_x, p_y: supplied base-pairing matrices
        s1, m1, s2, m2 = node[:4]
        s1 = np.ascontiguousarray(s1, np.uint32); s2 = np.ascontiguousarray(s2, np.uint32)
        m1 = np.ascontiguousarray(m1, np.uint8); m2 = np.ascontiguousarray(m2, np.uint8)
        px = np.ascontiguousarray(node[4], np.float32) if len(node) > 4 and node[4] is not None else None
        py = np.ascontiguousarray(node[5], np.float32) if len(node) > 5 and node[5] is not None else None
        keep.append((s1, s2, m1, m2, px, py))
        ins[b].n1, ins[b].n2, ins[b].len1, ins[b].len2 = m1.shape[0], m2.shape[0], m1.shape[1], m2.shape[1]
        ins[b].seq1, ins[b].seq2, ins[b].mask1, ins[b].mask2 = s1.ctypes.data, s2.ctypes.data, m1.ctypes.data, m2.ctypes.data
        ins[b].p_x = px.ctypes.data if px is not None else None
        ins[b].p_y = py.ctypes.data if py is not None else None
    return ins, keep


class NodeOutput(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("z", C.c_void_p), ("score", C.c_float),
                ("ncbp", C.c_uint32), ("iterations", C.c_uint32), ("violated", C.c_uint32)]


class DDParams(C.Structure):
    _fields_ = [("w", C.c_float), ("eta0", C.c_float), ("th_a", C.c_float), ("th_s", C.c_float),
                ("t_max", C.c_uint32), ("force_iters", C.c_int), ("skip_uncoupled_folds", C.c_int)]


_nussinov_decode = _sig("dafs_hip_nussinov_decode", C.c_int,
                        [C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)])
_nw_envelope = _sig("dafs_hip_nw_envelope", C.c_int, [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])
_nw_decode = _sig("dafs_hip_nw_decode", C.c_int,
                  [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)])
_nussinov_decode_dense = _sig("dafs_hip_nussinov_decode_dense", C.c_int,
                              [C.c_void_p, C.c_float, C.c_float, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)])
_nw_decode_dense = _sig("dafs_hip_nw_decode_dense", C.c_int,
                        [C.c_void_p, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float)])
_make_brackets = _sig("dafs_hip_make_brackets", None, [C.c_uint32, C.c_void_p, C.c_char_p])
_make_brackets_levels = _sig("dafs_hip_make_brackets_levels", None, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p])
_nussinov_decode_levels = _sig("dafs_hip_nussinov_decode_levels", C.c_int,
                               [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
MAX_LEVELS = 4
MAX_CANDIDATES = 16
_nussinov_decode_auto = _sig("dafs_hip_nussinov_decode_auto", C.c_int,
                             [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32] + [C.c_void_p] * 10)
_dd_default_params = _sig("dafs_hip_dd_default_params", None, [C.POINTER(DDParams)])
_solve_nodes = _sig("dafs_hip_solve_nodes", C.c_int,
                    [C.c_void_p, C.c_uint32, C.POINTER(NodeInput), C.POINTER(DDParams), C.POINTER(NodeOutput)])
_build_tree = _sig("dafs_host_build_tree", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
_cluster_cut = _sig("dafs_host_cluster_cut", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_uint32, C.c_void_p, u32p])
CLUSTER_THRESHOLD, CLUSTER_COUNT = 0, 1  # the modes of dafs_host_cluster_cut
_cluster_table = _sig("dafs_host_cluster_table", C.c_int, [C.c_uint32, C.POINTER(C.c_char_p)] + [C.c_void_p] * 6 + [C.POINTER(C.c_void_p)])
_linkage_tree = _sig("dafs_hip_linkage_tree", C.c_int, [C.c_void_p, C.c_int, C.c_uint32] + [C.c_void_p] * 4)
linkage_workspace = _sig("dafs_hipk_linkage_workspace", C.c_size_t, [C.c_uint32])
linkage_launch = _sig("dafs_hipk_linkage", C.c_int, [C.c_int, C.c_uint32] + [C.c_void_p] * 6)
LINKAGES = ("guide", "single", "complete", "average")  # --cluster-linkage; the index is the library's DAFS_LINKAGE_* code
_nj_tree = _sig("dafs_hip_nj_tree", C.c_int, [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4)
nj_workspace = _sig("dafs_hipk_nj_workspace", C.c_size_t, [C.c_uint32])
nj_launch = _sig("dafs_hipk_nj", C.c_int, [C.c_uint32] + [C.c_void_p] * 6)
_nj_distances = _sig("dafs_host_nj_distances", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])
NJ_MODELS = ("p", "jc")  # --phylogeny-model; the index is the library's DAFS_NJ_* code
_nj_trees = _sig("dafs_hip_nj_trees", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_void_p] * 4)
nj_batch_workspace = _sig("dafs_hipk_nj_batch_workspace", C.c_size_t, [C.c_uint32, C.c_uint32])
nj_batch_launch = _sig("dafs_hipk_nj_batch", C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 6)
_alignment_bootstrap = _sig("dafs_hip_alignment_bootstrap", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int,
                                                                     C.c_uint32, C.c_uint64] + [C.c_void_p] * 5)
_bootstrap_alignment = _sig("dafs_hip_bootstrap_alignment", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                                                     C.c_uint32, C.c_void_p])
bootstrap_fixups = _sig("dafs_hip_bootstrap_fixups", C.c_uint64, [])
_tree_support = _sig("dafs_host_tree_support", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])
BOOTSTRAP_MAX = 65536
_alignment_bootstrap_transfer = _sig("dafs_hip_alignment_bootstrap_transfer", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                                                       C.c_int, C.c_uint32, C.c_uint64] + [C.c_void_p] * 6)
_tree_transfer = _sig("dafs_hip_tree_transfer", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 4)
tree_transfer_workspace = _sig("dafs_hipk_tree_transfer_workspace", C.c_size_t, [C.c_uint32, C.c_uint32])
tree_transfer_launch = _sig("dafs_hipk_tree_transfer", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 8)
_transfer_runs = _sig("dafs_host_transfer_runs", C.c_int, [C.c_uint32] + [C.c_void_p] * 5)
_split_depth = _sig("dafs_host_split_depth", C.c_int, [C.c_uint32] + [C.c_void_p] * 3)
_transfer_percent = _sig("dafs_host_transfer_percent", C.c_int32, [C.c_int64, C.c_uint32, C.c_uint32])
NJ_MAX_ROWS = 16384
COV_TREES = ("average", "nj")  # --cov-tree
_merge_added = _sig("dafs_host_merge_added", C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 5)
# host text (dafs_amd/csrc/host_text.cpp): returned text is a char* the caller frees with dafs_host_free
_strs = C.POINTER(C.c_char_p)
_text = C.POINTER(C.c_void_p)
_host_free = _sig("dafs_host_free", None, [C.c_void_p])
_pp_char = _sig("dafs_host_pp_char", C.c_char, [C.c_double])
_stockholm_names = _sig("dafs_host_stockholm_names", C.c_int, [C.c_uint32, _strs, _text])
_stockholm_block = _sig("dafs_host_stockholm_block", C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, _strs, _strs, C.POINTER(C.c_void_p), C.c_void_p,
                                                                C.c_char_p, C.c_void_p, C.c_char_p, _text])
_stockholm_block_rows = _sig("dafs_host_stockholm_block_rows", C.c_int, [C.c_char_p, C.c_uint32, C.c_uint32, _strs, _strs, C.POINTER(C.c_void_p),
                                                                          C.c_void_p, C.c_char_p, C.c_void_p, C.c_char_p, _strs, _text])
_stockholm_block_merged = _sig("dafs_host_stockholm_block_merged", C.c_int, [C.c_uint32, C.c_uint32, _strs, _strs, C.POINTER(C.c_void_p), C.c_char_p,
                                                                              C.c_void_p, C.c_void_p, _text])
_merged_refusal = _sig("dafs_host_merged_refusal", C.c_char_p, [])
_cov_code = _sig("dafs_host_cov_code", C.c_uint8, [C.c_char])
_cov_ss_cons = _sig("dafs_host_cov_ss_cons", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_double, _text])
_covariation_table = _sig("dafs_host_covariation_table", C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 10 + [_text])
_pairwise_table = _sig("dafs_host_pairwise_table", C.c_int, [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, _strs] + [C.c_void_p] * 3 + [_text])
_seed_table = _sig("dafs_host_seed_table", C.c_int, [C.c_uint32, _strs] + [C.c_void_p] * 4 + [_text])
_seed_table_support = _sig("dafs_host_seed_table_support", C.c_int, [C.c_uint32, _strs] + [C.c_void_p] * 8 + [_text])
_seed_parse_structure = _sig("dafs_host_seed_parse_structure", C.c_int, [C.c_char_p, C.c_size_t, u32p, C.POINTER(C.c_int), _text, _text, _text])
_seed_clean_structure = _sig("dafs_host_seed_clean_structure", C.c_int, [C.c_uint32, _strs, _strs, C.c_char_p, C.c_void_p, u32p, _text])
_fold_complementary = _sig("dafs_host_fold_complementary", C.c_int, [C.c_char, C.c_char])
_row_constraint = _sig("dafs_host_row_constraint", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_char_p, C.c_char_p])
_seed_clean_structure_levels = _sig("dafs_host_seed_clean_structure_levels", C.c_int,
                                    [C.c_uint32, _strs, _strs, C.c_char_p, C.c_void_p, C.c_void_p, u32p, _text])
_row_constraint_levels = _sig("dafs_host_row_constraint_levels", C.c_int,
                              [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p])
_seed_each_bytes = _sig("dafs_host_seed_each_bytes", C.c_uint64, [C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32])
_seed_parse = _sig("dafs_host_seed_parse", C.c_int, [C.c_char_p, C.c_size_t, u32p, _text, _text])
_seed_clean = _sig("dafs_host_seed_clean", C.c_int, [C.c_uint32, _strs, _strs, _text])
_family_bytes = _sig("dafs_host_family_bytes", C.c_uint64, [C.c_uint32, C.c_void_p])
_node_bytes = _sig("dafs_host_node_bytes", C.c_uint64, [C.c_uint32, C.c_uint32])
_batch_bytes = _sig("dafs_host_batch_bytes", C.c_uint64, [])
_structure_bytes = _sig("dafs_host_structure_bytes", C.c_uint64, [C.c_uint32, C.c_uint32])
_structures_batch_bytes = _sig("dafs_host_structures_batch_bytes", C.c_uint64, [])
_reliability_bytes = _sig("dafs_host_reliability_bytes", C.c_uint64, [C.c_uint32, C.c_uint32])
_reliability_batch_bytes = _sig("dafs_host_reliability_batch_bytes", C.c_uint64, [])
_pack_greedy = _sig("dafs_host_pack_greedy", C.c_int, [C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p])
_set_mp = _sig("dafs_hip_set_mp", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
_nodes_open = _sig("dafs_hip_nodes_open", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(NodeInput), C.POINTER(DDParams), C.c_void_p])
_nodes_advance = _sig("dafs_hip_nodes_advance", C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(DDParams), C.c_uint32, C.c_void_p])
_nodes_round = _sig("dafs_hip_nodes_round", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(NodeInput), C.c_void_p, C.c_uint32, C.c_void_p,
                                                      C.POINTER(DDParams), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p])
_nodes_result = _sig("dafs_hip_nodes_result", C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(NodeOutput)])
_nodes_close = _sig("dafs_hip_nodes_close", C.c_int, [C.c_void_p])
_node_peek = _sig("dafs_hip_node_peek", C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)])
# the arrays of dafs_hip_node_peek (DAFS_PEEK_* of dafs_hip.h, in their order) and their element types
NODE_PEEK = ("p_x", "p_y", "p_z", "x_ptr", "x_col", "x_map", "y_ptr", "y_col", "y_map", "pz_ptr", "pz_k", "cz_ptr", "cz_k", "zmap", "env", "env4",
             "cbp_cnt", "cbp")
_NODE_PEEK_TYPE = {"p_x": np.float32, "p_y": np.float32, "p_z": np.float32, "x_map": np.int32, "y_map": np.int32, "zmap": np.int32}
_nodes_memory = _sig("dafs_hip_nodes_memory", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)])
_nodes_demotions = _sig("dafs_hip_nodes_demotions", C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)])
_update_basepairing = _sig("dafs_hip_update_basepairing", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])
_consensus_structure = _sig("dafs_hip_consensus_structure", C.c_int,
                            [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                             C.POINTER(C.c_float), C.c_void_p])
_structure_levels_bytes = _sig("dafs_host_structure_levels_bytes", C.c_uint64, [C.c_uint32, C.c_uint32])
_consensus_structures_levels = _sig("dafs_hip_consensus_structures_levels", C.c_int,
                                    [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p])
_structure_auto_bytes = _sig("dafs_host_structure_auto_bytes", C.c_uint64, [C.c_uint32, C.c_uint32, C.c_uint32])
_consensus_structures_auto = _sig("dafs_hip_consensus_structures_auto", C.c_int,
                                  [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
                                  + [C.c_void_p] * 10)
_consensus_structures = _sig("dafs_hip_consensus_structures", C.c_int,
                             [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p])
_alignment_reliability = _sig("dafs_hip_alignment_reliability", C.c_int,
                              [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5)
_alignment_reliabilities = _sig("dafs_hip_alignment_reliabilities", C.c_int,
                                [C.c_void_p, C.c_uint32] + [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_void_p] * 5)
_alignment_covariation = _sig("dafs_hip_alignment_covariation", C.c_int,
                              [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64] + [C.c_void_p] * 11)
_alignment_covariation_null = _sig("dafs_hip_alignment_covariation_null", C.c_int,
                                   [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p,
                                    C.c_void_p] + [C.c_void_p] * 11)
_covariation_null_alignment = _sig("dafs_hip_covariation_null_alignment", C.c_int,
                                   [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                    C.c_void_p])
COV_NULLS = ("shuffle", "tree")  # --cov-null; the index is the library's DAFS_COV_NULL_* code
_alignment_identity = _sig("dafs_hip_alignment_identity", C.c_int,
                           [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double] + [C.c_void_p] * 7)
_alignment_weights = _sig("dafs_hip_alignment_weights", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])


class CompareOut(C.Structure):
    """dafs_compare_out"""
    _fields_ = [(k, C.c_void_p) for k in ("residues", "shared", "refp", "testp", "sps", "ppv", "total", "score", "k", "m", "colref", "colshared",
                                         "reproduced", "tc", "pair_shared", "pair_refp", "pair_testp", "pp_count", "tp", "nref", "ntest", "ss_total")]


_alignment_compare = _sig("dafs_hip_alignment_compare", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 7 + [C.POINTER(CompareOut)])
_compare_refusal = _sig("dafs_host_compare_refusal", C.c_char_p, [C.c_int])
CMP_NEEDS_REF, CMP_NEEDS_COMPARE, CMP_NO_PAIRWISE, CMP_NEEDS_MERGED, CMP_TOO_MANY_ROWS = range(5)  # dafs_host_compare_refusal
_compare_match = _sig("dafs_host_compare_match", C.c_int, [C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32, C.POINTER(C.c_char_p)] + [C.c_void_p] * 3)
_seed_pp = _sig("dafs_host_seed_pp", C.c_int, [C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_void_p)])
_compare_table = _sig("dafs_host_compare_table", C.c_int, [C.c_uint32, C.POINTER(C.c_char_p)] + [C.c_uint32] * 4 + [C.c_void_p] * 10 + [C.POINTER(C.c_void_p)])
_compare_columns_table = _sig("dafs_host_compare_columns_table", C.c_int, [C.c_uint32] + [C.c_void_p] * 4 + [C.POINTER(C.c_void_p)])
_compare_matrix_table = _sig("dafs_host_compare_matrix_table", C.c_int, [C.c_uint32, C.POINTER(C.c_char_p)] + [C.c_void_p] * 3 + [C.POINTER(C.c_void_p)])
_nr_select = _sig("dafs_host_nr_select", C.c_int, [C.c_uint32] + [C.c_void_p] * 5)
_ali_code = _sig("dafs_host_ali_code", C.c_uint8, [C.c_char])
_identity_summary = _sig("dafs_host_identity_summary", C.c_int, [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p])
_identity_table = _sig("dafs_host_identity_table", C.c_int, [C.c_uint32, C.c_uint32, _strs] + [C.c_void_p] * 6 + [_text])
_identity_matrix_table = _sig("dafs_host_identity_matrix_table", C.c_int, [C.c_uint32, _strs] + [C.c_void_p] * 3 + [_text])
_stockholm_weights = _sig("dafs_host_stockholm_weights", C.c_int, [C.c_char_p, C.c_uint32, _strs, C.c_void_p, _text])
_stockholm_nr = _sig("dafs_host_stockholm_nr", C.c_int, [C.c_char_p, C.c_uint32, _strs, C.c_void_p, C.c_uint32, C.c_double, _text])
_alistat_refusal = _sig("dafs_host_alistat_refusal", C.c_char_p, [C.c_int])
NO_PAIRWISE, NR_NEEDS_MERGED, NR_THRESHOLD, TOO_MANY_ROWS = range(4)  # dafs_host_alistat_refusal
_newick = _sig("dafs_host_newick", C.c_int, [C.c_uint32, _strs, C.c_void_p, C.c_void_p, C.c_void_p, _text])
_newick_support = _sig("dafs_host_newick_support", C.c_int, [C.c_uint32, _strs] + [C.c_void_p] * 4 + [C.c_uint32, _text])
_support_table = _sig("dafs_host_support_table", C.c_int, [C.c_uint32, _strs] + [C.c_void_p] * 3 + [C.c_uint32, C.c_uint64, C.c_int, _text])
_phylogeny_refusal = _sig("dafs_host_phylogeny_refusal", C.c_char_p, [C.c_int])
(PHY_NO_PAIRWISE, PHY_NO_SEED_EACH, PHY_TOO_MANY_ROWS, PHY_MODEL_NEEDS_TREE, PHY_UNKNOWN_MODEL, PHY_COV_TREE_NEEDS_NULL,
 PHY_UNKNOWN_COV_TREE) = range(7)  # dafs_host_phylogeny_refusal
_bootstrap_refusal = _sig("dafs_host_bootstrap_refusal", C.c_char_p, [C.c_int])
_newick_transfer = _sig("dafs_host_newick_transfer", C.c_int, [C.c_uint32, _strs] + [C.c_void_p] * 4 + [C.c_uint32, _text])
_transfer_table = _sig("dafs_host_transfer_table", C.c_int, [C.c_uint32, _strs] + [C.c_void_p] * 4 + [C.c_uint32, C.c_uint64, C.c_int, _text])
_transfer_refusal = _sig("dafs_host_transfer_refusal", C.c_char_p, [C.c_int])
TRANSFER_NEEDS_REPLICATES = 0  # dafs_host_transfer_refusal
BOOT_NEEDS_TREE, BOOT_COUNT, BOOT_NEEDS_REPLICATES, BOOT_NO_COLUMN = range(4)  # dafs_host_bootstrap_refusal
_seed_table_nearest = _sig("dafs_host_seed_table_nearest", C.c_int, [C.c_uint32, _strs] + [C.c_void_p] * 8 + [_strs, C.c_void_p, _text])
# dafs_allgather_fn(user, send, recv, bytes, hip_stream): the caller's collective of a sharded phase 1
_allgather_fn = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_phase1_sharded = _sig("dafs_hip_phase1_sharded", C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_float,
                                                           C.c_int, C.c_float, _allgather_fn, C.c_void_p])


class StageTime(C.Structure):
    _fields_ = [("kernel", C.c_char_p), ("ms", C.c_double), ("longest_ms", C.c_double), ("launches", C.c_uint32)]


_stage_timing = _sig("dafs_hip_stage_timing", C.c_int, [C.c_void_p, C.c_int])
_stage_report = _sig("dafs_hip_stage_report", C.c_int, [C.c_void_p, C.POINTER(StageTime), C.c_uint32, C.POINTER(C.c_uint32)])
pairhmm_plan = _sig("dafs_hipk_pairhmm_plan", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PairhmmPlan)])
pairhmm3_launch = _sig("dafs_hipk_pairhmm3_launch", C.c_int, [C.POINTER(Pairhmm3Args), C.POINTER(PairhmmPlan), C.c_void_p])
pairhmm3_default_model = _sig("dafs_hip_pairhmm3_default_model", None, [C.POINTER(Pairhmm3Model)])
pairhmm5_plan = _sig("dafs_hipk_pairhmm5_plan", C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(PairhmmPlan)])
pairhmm5_launch = _sig("dafs_hipk_pairhmm5_launch", C.c_int, [C.POINTER(Pairhmm5Args), C.POINTER(PairhmmPlan), C.c_void_p])
pairhmm5_default_model = _sig("dafs_hip_pairhmm5_default_model", None, [C.POINTER(Pairhmm5Model)])
residue_code = _sig("dafs_hip_residue_code", C.c_uint8, [C.c_char])
dd_node_plan = _sig("dafs_hipk_dd_node_plan", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(DdNodePlan)])
dd_lds_words = _sig("dafs_hipk_dd_lds_words", C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int])
contrafold_plan = _sig("dafs_hipk_contrafold_plan", C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(ContrafoldPlan)])


def check(rc):
    if rc != 0:
        raise DafsHipError("%s (code %d; hip: %s)" % (_strerror(rc).decode(), rc, _last_error().decode()))


def _allgather_callback(allgather, failures):
    """allgather(send_ptr, recv_ptr, nbytes) as a dafs_allgather_fn.  No exception may cross the library's frames: one that
    allgather raises is appended to `failures` and the callback returns 1, which the library reports as DAFS_HIP_ECOMM."""
    def cb(user, send, recv, nbytes, stream):
        try:
            allgather(send, recv, nbytes)
        except BaseException as e:  # noqa: BLE001
            failures.append(e)
            return 1
        return 0
    return _allgather_fn(cb)


def encode(seq):
    """residue bytes -> class codes (uint8 numpy array)"""
    b = seq.encode() if isinstance(seq, str) else bytes(seq)
    table = np.array([residue_code(bytes([i])) for i in range(256)], dtype=np.uint8)
    return table[np.frombuffer(b, dtype=np.uint8)]


_COV_CODE = np.array([_cov_code(bytes([i])) for i in range(256)], np.uint8)


def encode_alignment(rows):
    """Alignment text (equally long rows) -> the uint8 [n, len] codes of Context.alignment_covariation: A 0, C 1, G 2, U / T 3
    in either case, everything else (gaps, N, IUPAC codes) 4."""
    rows = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in rows]
    if not rows or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("encode_alignment: at least one row, all of one length")
    return _COV_CODE[np.frombuffer(b"".join(rows), np.uint8)].reshape(len(rows), len(rows[0]))


_ALI_CODE = np.array([_ali_code(bytes([i])) for i in range(256)], np.uint8)


def encode_cells(rows):
    """Alignment text (equally long rows) -> the uint8 [n, len] cells of Context.alignment_identity / alignment_weights
    (DESIGN.md section 18): A 0, C 1, G 2, U / T 3 in either case, any other letter 4, '-' and '.' 5; anything else is refused."""
    rows = [r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in rows]
    if not rows or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("encode_cells: at least one row, all of one length")
    cell = _ALI_CODE[np.frombuffer(b"".join(rows), np.uint8)].reshape(len(rows), len(rows[0]))
    if (cell == 255).any():
        r, c = np.argwhere(cell == 255)[0]
        raise ValueError("encode_cells: row %d, column %d holds neither a letter nor a gap" % (r + 1, c + 1))
    return cell


def _cells(rows, who):
    """text rows or a 2-D integer array of cell codes -> uint8 [n, len]"""
    if isinstance(rows, np.ndarray):
        if rows.ndim != 2 or rows.dtype.kind not in "iu":
            raise ValueError("%s: rows are text rows or a 2-D integer array of cells" % who)
        if rows.size and (rows.min() < 0 or rows.max() > 255):
            raise ValueError("%s: cells must fit a byte (the library refuses a code above 5)" % who)
        return np.ascontiguousarray(rows, np.uint8)
    return encode_cells(rows)


def _byte_mask(mask, size, who, what):
    if mask is None:
        return None
    mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    if mask.shape != (size,):
        raise ValueError("%s: %s" % (who, what))
    return mask


def alistat_refusal(which):
    """what both drivers say when they refuse a combination of the alignment statistics' options (dafs_host_alistat_refusal)"""
    return _alistat_refusal(which).decode()


class Identity:
    """Result of Context.alignment_identity: .res, .nearest (NONE without a candidate), .nearest_ident, .nearest_den,
    .pid_nearest (NaN without a candidate); with matrix, .ident and .aligned ([n, n]); with nr, .red ([n, ceil(n / 32)] bits)."""

    def bit(self, r, s):
        """red(r, s)"""
        return bool((int(self.red[r, s // 32]) >> (s % 32)) & 1)


def nr_select(red, rank, forced=None):
    """dafs_host_nr_select: the non-redundant subset from the bit matrix red ([n, ceil(n / 32)] uint32),
    visiting the rows in the order rank (a permutation, else ValueError); forced rows are always kept.  Returns (kept as bool
    [n], by as uint32 [n]: the first kept row that removes a dropped one, NONE for a kept row)."""
    red = np.ascontiguousarray(red, np.uint32)
    n = red.shape[0] if red.ndim == 2 else 0
    if n == 0 or red.shape[1] != (n + 31) // 32:
        raise ValueError("nr_select: red is a [n, ceil(n / 32)] bit matrix")
    rank = np.ascontiguousarray(rank, np.uint32).reshape(-1)
    if len(rank) != n:
        raise ValueError("nr_select: the visiting order is not a permutation of the rows")
    forced = _byte_mask(forced, n, "nr_select", "forced needs one entry per row")
    kept = np.zeros(n, np.uint8)
    by = np.zeros(n, np.uint32)
    rc = _nr_select(n, red.ctypes.data, rank.ctypes.data, None if forced is None else forced.ctypes.data, kept.ctypes.data, by.ctypes.data)
    if rc == -1:
        raise ValueError(_last_error().decode("latin-1"))
    check(rc)
    return kept.astype(bool), by


def identity_summary(ident, res):
    """dafs_host_identity_summary: (average, minimum, maximum) pid over the pairs r < s; three NaN for one row"""
    ident = np.ascontiguousarray(ident, np.uint32)
    res = np.ascontiguousarray(res, np.uint32)
    n = len(res)
    if ident.shape != (n, n):
        raise ValueError("identity_summary: ident is the [n, n] matrix of the rows of res")
    out = np.zeros(3, np.float64)
    check(_identity_summary(n, ident.ctypes.data, res.ctypes.data, out.ctypes.data))
    return tuple(float(x) for x in out)


PP_CLASSES = "0123456789*"  # the characters of a "#=GR PP" line, by class


def encode_pp(rows):
    """The characters of "#=GR PP" lines (equally long rows, or None for a row without one) -> the uint8 [n, len] classes of
    Context.alignment_compare: '0'..'9' 0..9, '*' 10, anything else (the '.' of a gap) 255."""
    table = np.full(256, 255, np.uint8)
    for q, ch in enumerate(PP_CLASSES):
        table[ord(ch)] = q
    length = max((len(r) for r in rows if r is not None), default=0)
    rows = [b"." * length if r is None else r.encode("latin-1") if isinstance(r, str) else bytes(r) for r in rows]
    if not rows or any(len(r) != length for r in rows):
        raise ValueError("encode_pp: at least one row, all of one length")
    return table[np.frombuffer(b"".join(rows), np.uint8)].reshape(len(rows), length)


def compare_refusal(which):
    """what both drivers say when they refuse a combination of the comparison's options (dafs_host_compare_refusal)"""
    return _compare_refusal(which).decode()


def compare_match(ref_names, test_names):
    """dafs_host_compare_match: the rows to compare, as (ref_row, test_row) index arrays over the names in both alignments in
    the reference's order; ValueError for a name on two rows of either, or fewer than two common names"""
    ref_names, test_names = list(ref_names), list(test_names)
    room = max(min(len(ref_names), len(test_names)), 1)
    count = C.c_uint32()
    ref_row, test_row = np.zeros(room, np.uint32), np.zeros(room, np.uint32)
    rc = _compare_match(len(ref_names), c_strings(ref_names), len(test_names), c_strings(test_names), C.byref(count), ref_row.ctypes.data,
                        test_row.ctypes.data)
    if rc == -1:
        raise ValueError(_last_error().decode("latin-1"))
    check(rc)
    return ref_row[:count.value].copy(), test_row[:count.value].copy()


class Comparison:
    """Result of Context.alignment_compare, R the reference and T the test alignment.
    Per row: .residues, .shared, .refp, .testp (uint64), .row_sps, .row_ppv.  Totals: .total_shared, .total_refp, .total_testp,
    .sps, .ppv.  Per column: .k [len_r], .m [len_t], .colref, .colshared, .reproduced [len_r]; .tc_reproduced, .tc_columns, .tc.
    With matrix: .pair_shared, .pair_refp, .pair_testp ([n, n] uint32).  With pp: .pp_residues, .pp_ref, .pp_shared (uint64 [11])
    and .pp_accuracy (NaN for a class without pairs).  With both structures: .tp, .nref, .ntest per row, .total_tp, .total_nref,
    .total_ntest, .sensitivity, .ss_ppv, .f."""


class PairPosteriors:
    """Result of Context.align_posteriors: per pair (in shard order) the sparse matching
    probabilities mp[x][y] (CSR) and mp[y][x] (CSR of the transpose), and sim[x][y]."""

    def __init__(self, pair_x, pair_y, sim, nnz, rowptr, col, val, lens):
        self.pair_x, self.pair_y, self.sim, self.nnz = pair_x, pair_y, sim, nnz
        self._rowptr, self._col, self._val, self._lens = rowptr, col, val, lens
        l1 = lens[pair_x].astype(np.int64) + 1
        l2 = lens[pair_y].astype(np.int64) + 1
        self._rp_off = np.concatenate([[0], np.cumsum(l1 + l2)])[:-1]
        self._ent_off = np.concatenate([[0], np.cumsum(2 * nnz.astype(np.int64))])[:-1]

    def __len__(self):
        return len(self.pair_x)

    def csr(self, p, transposed=False):
        """(rowptr, col, val) of mp[x][y] (or mp[y][x]) for pair number p"""
        l1 = int(self._lens[self.pair_x[p]]) + 1
        l2 = int(self._lens[self.pair_y[p]]) + 1
        r0, e0, n = int(self._rp_off[p]), int(self._ent_off[p]), int(self.nnz[p])
        if not transposed:
            return self._rowptr[r0:r0 + l1], self._col[e0:e0 + n], self._val[e0:e0 + n]
        return self._rowptr[r0 + l1:r0 + l1 + l2], self._col[e0 + n:e0 + 2 * n], self._val[e0 + n:e0 + 2 * n]


class AutoThresholds:
    """Thresholds chosen by pseudo-expected accuracy: every level takes the candidate 1 / (1 + gamma)
    whose structure has the best F against the matrix it was decoded from, and a level is kept only if it raises F.
    gammas: 1 to MAX_CANDIDATES weights, strictly increasing and positive (the command line's -G); levels: at most this
    many levels, 1 to MAX_LEVELS."""

    def __init__(self, gammas=(1, 2, 4, 8, 16, 32), levels=1):
        self.gammas = tuple(float(g) for g in gammas)
        self.levels = int(levels)
        if not 1 <= self.levels <= MAX_LEVELS:
            raise ValueError("AutoThresholds: 1 to %d levels" % MAX_LEVELS)
        if not 1 <= len(self.gammas) <= MAX_CANDIDATES:
            raise ValueError("AutoThresholds: 1 to %d candidates" % MAX_CANDIDATES)
        if not all(g > 0 and np.isfinite(g) for g in self.gammas) or any(b <= a for a, b in zip(self.gammas, self.gammas[1:])):
            raise ValueError("AutoThresholds: the weights are positive and strictly increasing")
        self.candidates = np.array([np.float32(1.0 / (1.0 + g)) for g in self.gammas], np.float32)  # as -G is converted

    def __repr__(self):
        return "AutoThresholds(gammas=%r, levels=%d)" % (self.gammas, self.levels)


class AutoChoice:
    """What an automatic choice kept for one alignment: .chosen [levels] (the candidate's index, NONE for an empty level),
    .thresholds and .gammas (of the kept levels), .sum_p (S), .tp and .npairs [levels] (T and n of each kept level alone),
    .cand_tp and .cand_pairs [levels, candidates] (every decode's T and n; 0 for the levels that were not decoded), and .f, the
    pseudo-expected F of the whole structure, 2 sum(tp) / (sum(npairs) 2^30 + sum_p), a float for display only."""

    def __init__(self, auto, chosen, sum_p, tp, npairs, cand_tp, cand_pairs):
        self.chosen, self.sum_p, self.tp, self.npairs = chosen, int(sum_p), tp, npairs
        self.cand_tp, self.cand_pairs = cand_tp, cand_pairs
        kept = [int(c) for c in chosen if c != NONE]
        self.thresholds = auto.candidates[kept]
        self.gammas = tuple(auto.gammas[c] for c in kept)
        self.f = pseudo_f(sum(int(t) for t in tp), sum(int(n) for n in npairs), self.sum_p)


class _AutoArrays:
    """the arrays dafs_hip_consensus_structures_auto fills beside ss, level and score, for n alignments"""

    def __init__(self, n, K, ncand):
        self.chosen = np.zeros((n, K), np.uint32)
        self.sum_p = np.zeros(n, np.uint64)
        self.tp = np.zeros((n, K), np.uint64)
        self.npairs = np.zeros((n, K), np.uint32)
        self.cand_tp = np.zeros((n, K, ncand), np.uint64)
        self.cand_pairs = np.zeros((n, K, ncand), np.uint32)

    def pointers(self):
        return [x.ctypes.data for x in (self.chosen, self.sum_p, self.tp, self.npairs, self.cand_tp, self.cand_pairs)]

    def choice(self, auto, a):
        return AutoChoice(auto, self.chosen[a], self.sum_p[a], self.tp[a], self.npairs[a], self.cand_tp[a], self.cand_pairs[a])


def pseudo_f(tp, npairs, sum_p):
    """2 T / (n 2^30 + S) as a float, 0.0 when the denominator is 0 (display only: the library compares in integers)"""
    den = int(npairs) * 2 ** 30 + int(sum_p)
    return 2 * int(tp) / den if den else 0.0


class Context:
    """Owns one dafs_hip_ctx (device workspace on one GPU)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        check(_create(device, C.byref(self._h)))
        self._lens = None
        self._first = np.array([0, 0], np.uint32)
        self._node_lens = {}  # handle -> (len1, len2) of the nodes opened since nodes_close (node_peek shapes its arrays by them)
        self.device_index = device

    def close(self):
        if self._h:
            _destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_sequences(self, seqs):
        bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
        arr = (C.c_char_p * len(bs))(*bs)
        lens = np.array([len(b) for b in bs], dtype=np.uint32)
        check(_set_sequences(self._h, len(bs), arr, lens.ctypes.data_as(u32p)))
        self._lens = lens
        self._first = np.array([0, len(bs)], np.uint32)

    def set_families(self, first):
        """Family partition of the sequences (dafs_hip_set_families): family f is sequences first[f] .. first[f+1]-1, with
        first[0] = 0 and first[-1] = the number of sequences.  Invalidates the stores."""
        first = np.ascontiguousarray(first, np.uint32)
        if len(first) < 2:
            raise ValueError("set_families: first needs nfam + 1 >= 2 entries")
        check(_set_families(self._h, len(first) - 1, first.ctypes.data_as(u32p)))
        self._first = first

    def align_posteriors(self, model=ALIGN_PROBCONS, th=0.01, pair_begin=0, pair_end=0, fetch=True):
        check(_align_posteriors(self._h, model, th, pair_begin, pair_end))
        if not fetch:
            return None
        npairs, nnz, nrp = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(_align_result_size(self._h, C.byref(npairs), C.byref(nnz), C.byref(nrp)))
        n = npairs.value
        px = np.zeros(n, np.uint32); py = np.zeros(n, np.uint32)
        sim = np.zeros(n, np.float32); cnt = np.zeros(n, np.uint32)
        rowptr = np.zeros(nrp.value, np.uint32)
        col = np.zeros(2 * nnz.value, np.uint32); val = np.zeros(2 * nnz.value, np.float32)
        check(_align_fetch(self._h, px.ctypes.data, py.ctypes.data, sim.ctypes.data, cnt.ctypes.data,
                           rowptr.ctypes.data, col.ctypes.data, val.ctypes.data))
        return PairPosteriors(px, py, sim, cnt, rowptr, col, val, self._lens)

    def mp(self, relaxed):
        """the matching-probability store (0: model output, 1: after consistency) as PairPosteriors"""
        npairs, nnz, nrp = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(_mp_result_size(self._h, relaxed, C.byref(npairs), C.byref(nnz), C.byref(nrp)))
        n = npairs.value
        px = np.zeros(n, np.uint32); py = np.zeros(n, np.uint32); cnt = np.zeros(n, np.uint32)
        rowptr = np.zeros(nrp.value, np.uint32)
        col = np.zeros(2 * nnz.value, np.uint32); val = np.zeros(2 * nnz.value, np.float32)
        check(_mp_fetch(self._h, relaxed, px.ctypes.data, py.ctypes.data, cnt.ctypes.data,
                        rowptr.ctypes.data, col.ctypes.data, val.ctypes.data))
        return PairPosteriors(px, py, None, cnt, rowptr, col, val, self._lens)

    def sim(self):
        """the N x N similarity matrix of a one-family context (sim_blocks() for several families)"""
        if len(self._first) != 2:
            raise ValueError("Context.sim: the context holds %d families; use sim_blocks()" % (len(self._first) - 1))
        return self.sim_blocks()[0]

    def sim_blocks(self):
        """per family its n x n similarity block (unit diagonal)"""
        sizes = np.diff(self._first.astype(np.int64))
        flat = np.zeros(int((sizes * sizes).sum()), np.float32)
        check(_get_sim(self._h, flat.ctypes.data))
        out, o = [], 0
        for n in sizes:
            out.append(flat[o:o + n * n].reshape(n, n).copy())
            o += n * n
        return out

    def similarity(self, model=ALIGN_PROBCONS, th=0.01, max_bytes=None, score="sequence", structure_weight=0.5):
        """dafs_hip_similarity: the N x N similarity matrix of a one-family context of any size, the pairs computed in ranges
        under max_bytes of estimated device memory (None: the library's budget; similarity_ranges gives the ranges).  Returns
        (sim, n_ranges); sim is what sim() returns after a full-pair-set align_posteriors, bit for bit.  The matching stores
        are invalid afterwards, whatever the number of ranges.

        score "structure" or "mix" (dafs_hip_similarity_scored): the matrix returned, and left for
        sim() and linkage_tree(), is the structural pair score or its mix with the sequence score at structure_weight (read
        with "mix" only).  They need the base-pairing store (fold_posteriors or set_bp after set_sequences), which stays
        valid; pair_scores() then gives the sequence and the structure matrix.  "sequence" is the call above."""
        score_check(score, structure_weight if score == "mix" else None)
        n_ranges = C.c_uint64()
        budget = 0 if max_bytes is None else int(max_bytes)
        if score == "sequence":
            check(_similarity(self._h, model, th, budget, C.byref(n_ranges)))
        else:
            check(_similarity_scored(self._h, model, th, budget, SCORES.index(score), float(structure_weight), C.byref(n_ranges)))
        return self.sim(), n_ranges.value

    def structure_scores(self):
        """dafs_hip_structure_scores: (T, terms, W) as uint64 arrays, T and terms per pair of the
        un-relaxed matching store valid now (in the pair order of align_posteriors' result), W per sequence from the
        un-relaxed base-pairing store.  Stores installed with set_mp / set_bp count like computed ones."""
        npairs = C.c_uint64()
        if _align_result_size(self._h, C.byref(npairs), None, None) != 0:
            npairs.value = 0  # no matching store: the call below refuses with its own message
        T = np.zeros(npairs.value, np.uint64); terms = np.zeros(npairs.value, np.uint64); W = np.zeros(len(self._lens), np.uint64)
        check(_structure_scores(self._h, T.ctypes.data, terms.ctypes.data, W.ctypes.data))
        return T, terms, W

    def pair_scores(self):
        """dafs_hip_get_pair_scores: (seq, struct), the raw sequence matrix and the structure matrix of the last
        similarity() with score "structure" or "mix" (N x N float32 each, unit diagonals)"""
        n = len(self._lens)
        seq = np.zeros((n, n), np.float32); st = np.zeros((n, n), np.float32)
        check(_get_pair_scores(self._h, seq.ctypes.data, st.ctypes.data))
        return seq, st

    def linkage_tree(self, rule, sim=None):
        """dafs_hip_linkage_tree: the "single", "complete" or "average" linkage tree of the n x n
        matrix sim (only the entries x < y are read, all of them finite), joined on the device; sim None: of the context's
        own similarity block (a one-family context after similarity() or a full-pair-set align_posteriors), read on the
        device and left untouched.  Returns (score, left, right) in build_tree's layout and types.  ValueError before any
        device work for an unknown rule, "guide" (that is build_tree), a matrix that is not square and a non-finite entry
        above its diagonal."""
        code, sim = linkage_check(rule, sim)
        n = int(len(self._lens)) if sim is None and self._lens is not None else (0 if sim is None else sim.shape[0])
        if n == 0:
            raise ValueError("linkage_tree: the context holds no sequences and no matrix was given")
        score = np.zeros(2 * n - 1, np.float32); left = np.zeros(2 * n - 1, np.int32); right = np.zeros(2 * n - 1, np.int32)
        rc = _linkage_tree(self._h, code, n, None if sim is None else sim.ctypes.data, score.ctypes.data, left.ctypes.data, right.ctypes.data)
        if rc == -1:
            raise ValueError(_last_error().decode("latin-1"))
        check(rc)
        return score, left.astype(np.int64), right.astype(np.int64)

    def nj_tree(self, dist):
        """dafs_hip_nj_tree: the neighbour-joining tree of the n x n matrix dist (float64; only the
        entries x < y are read, all of them finite), joined on the device.  Returns (left, right, length): int64 children in
        build_tree's layout and the float64 length of the branch above each node (0.0 at the root; negative lengths are kept).
        ValueError for a matrix that is not square, more than NJ_MAX_ROWS rows, a non-finite entry above the diagonal and an
        overflow during the joins."""
        dist = np.ascontiguousarray(dist, np.float64)
        if dist.ndim != 2 or dist.shape[0] != dist.shape[1] or dist.shape[0] == 0:
            raise ValueError("nj_tree: the distance matrix must be n x n with n >= 1")
        n = dist.shape[0]
        if n > NJ_MAX_ROWS:
            raise ValueError(phylogeny_refusal(PHY_TOO_MANY_ROWS))
        left = np.zeros(2 * n - 1, np.int32); right = np.zeros(2 * n - 1, np.int32); length = np.zeros(2 * n - 1, np.float64)
        rc = _nj_tree(self._h, n, dist.ctypes.data, left.ctypes.data, right.ctypes.data, length.ctypes.data)
        if rc == -1:
            raise ValueError(_last_error().decode("latin-1"))
        check(rc)
        return left.astype(np.int64), right.astype(np.int64), length

    def alignment_tree(self, cell, use=None, model="jc"):
        """The neighbour-joining tree of an alignment's rows: the identity counts of
        alignment_identity(cell, use, matrix=True), nj_distances under `model` ("jc" or "p"), nj_tree.  cell: the text rows or
        their cells (encode_cells); use: the columns that count (None: all).  Returns (left, right, length)."""
        if model not in NJ_MODELS:
            raise ValueError(phylogeny_refusal(PHY_UNKNOWN_MODEL))
        cell = _cells(cell, "alignment_tree")
        if cell.shape[0] > NJ_MAX_ROWS:
            raise ValueError(phylogeny_refusal(PHY_TOO_MANY_ROWS))
        idt = self.alignment_identity(cell, use=use, matrix=True, nearest=False)
        return self.nj_tree(nj_distances(idt.ident, idt.aligned, model))

    def nj_trees(self, dists):
        """dafs_hip_nj_trees: the neighbour-joining trees of `count` n x n matrices (float64
        [count, n, n]; of each only the entries x < y are read), all matrices in one launch up to 2 048 rows.  Returns (left,
        right, length) as [count, 2n-1] arrays, each row what nj_tree gives the matrix.  ValueError for what nj_tree refuses,
        with the matrix named."""
        dists = np.ascontiguousarray(dists, np.float64)
        if dists.ndim != 3 or dists.shape[1] != dists.shape[2] or dists.shape[0] == 0 or dists.shape[1] == 0:
            raise ValueError("nj_trees: the distance matrices are [count, n, n] with count >= 1 and n >= 1")
        count, n = dists.shape[:2]
        if n > NJ_MAX_ROWS:
            raise ValueError(phylogeny_refusal(PHY_TOO_MANY_ROWS))
        left = np.zeros((count, 2 * n - 1), np.int32); right = np.zeros((count, 2 * n - 1), np.int32)
        length = np.zeros((count, 2 * n - 1), np.float64)
        rc = _nj_trees(self._h, n, count, dists.ctypes.data, left.ctypes.data, right.ctypes.data, length.ctypes.data)
        if rc == -1:
            raise ValueError(_last_error().decode("latin-1"))
        check(rc)
        return left.astype(np.int64), right.astype(np.int64), length

    def alignment_bootstrap(self, cell, use=None, model="jc", B=100, seed=12345, tree=None, trees=False, transfer=False):
        """Bootstrap support of a tree of an alignment's rows (dafs_hip_alignment_bootstrap): B replicate
        alignments drawn from the used columns with replacement, their distances under `model` and their neighbour-joining
        trees, all on the device.  tree: (left, right) or (left, right, length) of the main tree; None: alignment_tree(cell,
        use, model).  Returns support (int64 [2n-1]: the number of replicate trees holding the node's split, -1 for the root
        and trivial splits); with trees=True (support, rep_left, rep_right), the replicate trees as [B, 2n-1].  transfer=True
        (dafs_hip_alignment_bootstrap_transfer) appends the transfer sums (int64 [2n-1]: per split the
        sum over the replicates of its transfer index, -1 where support is -1) to what is returned: (support, transfer) or
        (support, rep_left, rep_right, transfer)."""
        if model not in NJ_MODELS:
            raise ValueError(phylogeny_refusal(PHY_UNKNOWN_MODEL))
        cell = _cells(cell, "alignment_bootstrap")
        n, L = cell.shape
        if n > NJ_MAX_ROWS:
            raise ValueError(phylogeny_refusal(PHY_TOO_MANY_ROWS))
        if not 1 <= int(B) <= BOOTSTRAP_MAX:
            raise ValueError(bootstrap_refusal(BOOT_COUNT))
        use = _byte_mask(use, L, "alignment_bootstrap", "use needs one entry per column")
        if tree is None:
            tree = self.alignment_tree(cell, use=use, model=model)
        left = np.ascontiguousarray(tree[0], np.int32).reshape(-1)
        right = np.ascontiguousarray(tree[1], np.int32).reshape(-1)
        if n == 0 or len(left) != 2 * n - 1 or len(right) != 2 * n - 1:
            raise ValueError("alignment_bootstrap: a tree of n rows has 2n - 1 nodes")
        support = np.zeros(2 * n - 1, np.int32)
        rep = [np.zeros((int(B), 2 * n - 1), np.int32) for _ in range(2)] if trees else [None, None]
        sums = np.zeros(2 * n - 1, np.int64) if transfer else None
        args = (self._h, n, L, cell.ctypes.data, None if use is None else use.ctypes.data, NJ_MODELS.index(model), int(B),
                int(seed) & 0xFFFFFFFFFFFFFFFF, left.ctypes.data, right.ctypes.data, support.ctypes.data,
                None if rep[0] is None else rep[0].ctypes.data, None if rep[1] is None else rep[1].ctypes.data)
        rc = _alignment_bootstrap_transfer(*args, sums.ctypes.data) if transfer else _alignment_bootstrap(*args)
        if rc == -1:
            raise ValueError(_last_error().decode("latin-1"))
        check(rc)
        support = support.astype(np.int64)
        out = (support, rep[0].astype(np.int64), rep[1].astype(np.int64)) if trees else (support,)
        if transfer:
            return out + (sums,)
        return out if trees else support

    def tree_transfer(self, tree, rep_left, rep_right, each=False):
        """Transfer bootstrap of a tree against replicate trees (dafs_hip_tree_transfer).  tree: (left,
        right[, length]) of the main tree; rep_left, rep_right: [B, 2n-1].  Returns transfer (int64 [2n-1]: per split the sum
        over the replicates of the transfer index, the fewest leaves that have to move for the replicate to hold the split;
        -1 for the root and trivial splits); with each=True (transfer, phi), phi int64 [B, 2n-1] the index per replicate."""
        left = np.ascontiguousarray(tree[0], np.int32).reshape(-1)
        right = np.ascontiguousarray(tree[1], np.int32).reshape(-1)
        rep_left = np.ascontiguousarray(rep_left, np.int32)
        rep_right = np.ascontiguousarray(rep_right, np.int32)
        T = len(left)
        if T % 2 != 1 or len(right) != T or rep_left.ndim != 2 or rep_left.shape[1] != T or rep_right.shape != rep_left.shape:
            raise ValueError("tree_transfer: a tree of n leaves has 2n - 1 nodes and the replicates are [B, 2n - 1]")
        B = rep_left.shape[0]
        sums = np.zeros(T, np.int64)
        phi = np.zeros((B, T), np.int32) if each else None
        rc = _tree_transfer(self._h, (T + 1) // 2, left.ctypes.data, right.ctypes.data, B, rep_left.ctypes.data, rep_right.ctypes.data,
                            sums.ctypes.data, None if phi is None else phi.ctypes.data)
        if rc == -1:
            raise ValueError(_last_error().decode("latin-1"))
        check(rc)
        return (sums, phi.astype(np.int64)) if each else sums

    def bootstrap_alignment(self, cell, k, use=None, seed=12345):
        """Replicate k (0-based) behind alignment_bootstrap(cell, use, seed=seed) as cells (uint8 [n, U], U the number of used
        columns; dafs_hip_bootstrap_alignment)."""
        cell = _cells(cell, "bootstrap_alignment")
        n, L = cell.shape
        use = _byte_mask(use, L, "bootstrap_alignment", "use needs one entry per column")
        U = L if use is None else int(use.sum())
        out = np.zeros((n, max(U, 1)), np.uint8)
        rc = _bootstrap_alignment(self._h, n, L, cell.ctypes.data, None if use is None else use.ctypes.data, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                  int(k), out.ctypes.data)
        if rc == -1:
            raise ValueError(_last_error().decode("latin-1"))
        check(rc)
        return out[:, :U]

    def set_bp(self, rows):
        """rows: per sequence (rowptr[len+1], col, val)"""
        rp = np.concatenate([np.asarray(r[0], np.uint32) for r in rows])
        col = np.concatenate([np.asarray(r[1], np.uint32) for r in rows]) if rows else np.zeros(0, np.uint32)
        val = np.concatenate([np.asarray(r[2], np.float32) for r in rows]) if rows else np.zeros(0, np.float32)
        rp = np.ascontiguousarray(rp); col = np.ascontiguousarray(col); val = np.ascontiguousarray(val)
        check(_set_bp(self._h, rp.ctypes.data, col.ctypes.data if len(col) else None, val.ctypes.data if len(val) else None))

    def bp(self, relaxed):
        """per sequence (rowptr, col, val)"""
        nnz, nrp = C.c_uint64(), C.c_uint64()
        check(_bp_result_size(self._h, relaxed, C.byref(nnz), C.byref(nrp)))
        rp = np.zeros(nrp.value, np.uint32); col = np.zeros(nnz.value, np.uint32); val = np.zeros(nnz.value, np.float32)
        check(_bp_fetch(self._h, relaxed, rp.ctypes.data, col.ctypes.data, val.ctypes.data))
        out, r0, e0 = [], 0, 0
        for L in self._lens:
            r = rp[r0:r0 + int(L) + 1]
            n = int(r[-1])
            out.append((r, col[e0:e0 + n], val[e0:e0 + n]))
            r0 += int(L) + 1
            e0 += n
        return out

    def _constraints(self, constraints):
        """per sequence a constraint string or None, or a sequence of up to MAX_LEVELS of them (one per level), as the char*
        array of the library: (array, None) for one string per sequence, (array[n * K], K) when an entry holds several"""
        cons = list(constraints)
        if self._lens is None or len(cons) != len(self._lens):
            raise ValueError("fold constraints: one entry (a string or None) per sequence of the context")
        plain = all(x is None or isinstance(x, (str, bytes, bytearray)) for x in cons)
        per = [[x] if x is None or isinstance(x, (str, bytes, bytearray)) else list(x) for x in cons]
        K = max([len(x) for x in per] + [1])
        bs = [None if x is None else (x.encode("latin-1") if isinstance(x, str) else bytes(x)) for row in per for x in row + [None] * (K - len(row))]
        if any(b is not None and b"\0" in b for b in bs):
            raise ValueError("fold constraints: a string holds a NUL byte")
        return (C.c_char_p * len(bs))(*bs), None if plain else K

    def fold_posteriors(self, th=0.01, model=0, constraints=None):
        """CONTRAfold base-pairing posteriors of every sequence -> the un-relaxed bp store.  constraints: per sequence None
        or "" (folded free) or len characters of "?.()" (dafs_hip_fold_posteriors_constrained); a refused string raises
        DafsHipError with the sequence index in its text.  An entry may also be a sequence of up to four such strings, one
        per level (dafs_hip_fold_posteriors_levels): the sequence is folded once per string that is
        neither None nor empty (once, free, when none is), and a cell's value is the maximum over its folds."""
        if constraints is None:
            check(_fold_posteriors(self._h, model, th))
            return
        arr, K = self._constraints(constraints)
        check(_fold_constrained(self._h, model, th, arr) if K is None else _fold_levels(self._h, model, th, K, arr))

    def fold_begin(self, th=0.01, model=0, constraints=None):
        """enqueue the folding kernels on their own stream; fold_end() waits and fills the bp store.  constraints: as in
        fold_posteriors"""
        if constraints is None:
            check(_fold_begin(self._h, model, th))
            return
        arr, K = self._constraints(constraints)
        check(_fold_constrained_begin(self._h, model, th, arr) if K is None else _fold_levels_begin(self._h, model, th, K, arr))

    def fold_end(self):
        check(_fold_end(self._h))

    def fold_posterior_dense(self, seq, constraint=None):
        b = seq.encode() if isinstance(seq, str) else bytes(seq)
        L = len(b)
        post = np.zeros((L + 1) * (L + 2) // 2, np.float32)
        logz = C.c_float()
        check(_fold_posterior_dense(self._h, b, L, None if constraint is None else constraint.encode(), post.ctypes.data, C.byref(logz)))
        return post, np.float32(logz.value)

    def consistency(self, w_pct_a=0.25, w_pct_s=0.25):
        check(_consistency(self._h, w_pct_a, w_pct_s))

    def fourway_consistency(self, w_pct_f):
        """DAFS::relax_fourway_consistency (-f): replaces the un-relaxed matching store and recomputes the similarity scores"""
        check(_fourway_consistency(self._h, w_pct_f))

    def consistency_match(self, w_pct_a=0.25):
        check(_consistency_match(self._h, w_pct_a))

    def consistency_bp(self, w_pct_s=0.25):
        check(_consistency_bp(self._h, w_pct_s))

    def pairs_from(self, src, pair_x, pair_y):
        """dafs_hip_pairs_from: this context becomes the P two-sequence families [pair_x[p], pair_y[p]] of src's sequences
        (rows 2p and 2p + 1), with the raw stores and similarity blocks those inputs give, gathered from src on the device.
        src: a one-family context after fold_posteriors and a full-pair-set align_posteriors, left unchanged."""
        px = np.ascontiguousarray(pair_x, np.uint32)
        py = np.ascontiguousarray(pair_y, np.uint32)
        if px.ndim != 1 or px.shape != py.shape:
            raise ValueError("pairs_from: pair_x and pair_y need one entry per pair")
        check(_pairs_from(self._h, src._h, len(px), px.ctypes.data_as(u32p), py.ctypes.data_as(u32p)))
        lens = np.empty(2 * len(px), np.uint32)
        lens[0::2], lens[1::2] = src._lens[px], src._lens[py]
        self._lens = lens
        self._first = np.arange(0, 2 * len(px) + 1, 2, dtype=np.uint32)

    def families_from(self, src, families):
        """dafs_hip_families_from: this context becomes the families `families` (per family the strictly ascending indices
        of its members among src's sequences; a sequence may be in many), with the raw stores and similarity blocks those
        inputs give, gathered from src on the device.  src: a one-family context after fold_posteriors and an
        align_posteriors over a prefix of its pairs that holds every pair the families need, left unchanged."""
        fams = [np.ascontiguousarray(f, np.uint32).reshape(-1) for f in families]
        first = np.zeros(len(fams) + 1, np.uint32)
        first[1:] = np.cumsum([len(f) for f in fams])
        member = np.ascontiguousarray(np.concatenate(fams) if fams else np.zeros(0, np.uint32), np.uint32)
        if len(member) == 0:
            member = np.zeros(1, np.uint32)  # a valid pointer: the library refuses the empty family itself
        check(_families_from(self._h, src._h, len(fams), first.ctypes.data_as(u32p), member.ctypes.data_as(u32p)))
        self._lens = src._lens[member[:int(first[-1])]]
        self._first = first

    def consistency_match_pairs(self, w_pct_a, pair_ids):
        """dafs_hip_consistency_match_pairs: the matching transform for the strictly ascending pair ids `pair_ids` of the
        context only; the other pairs of the relaxed store stay empty, and alignment_reliabilities refuses an alignment that
        needs one."""
        ids = np.ascontiguousarray(pair_ids, np.uint64).reshape(-1)
        check(_consistency_match_pairs(self._h, w_pct_a, len(ids), ids.ctypes.data if len(ids) else None))

    def phase1_sharded(self, rank, world, align_model, th_a, w_pct_a, w_pct_s, fold_th, allgather, fold_model=0):
        """dafs_hip_phase1_sharded: phase 1 on rank `rank` of `world` (every rank has set all the sequences, two at least);
        afterwards every rank's context holds the complete stores.  allgather(send_ptr, recv_ptr, nbytes) is the collective:
        nbytes of device memory from every rank into recv (world * nbytes, rank order), landed when it returns.  An exception
        it raises ends the call with a DafsHipError (DAFS_HIP_ECOMM) chained to it."""
        failures = []
        fn = _allgather_callback(allgather, failures)  # referenced until the library returns
        rc = _phase1_sharded(self._h, rank, world, align_model, th_a, w_pct_a, w_pct_s, fold_model, fold_th, fn, None)
        if rc and failures:
            raise DafsHipError("%s (code %d): %r" % (_strerror(rc).decode(), rc, failures[0])) from failures[0]
        check(rc)

    # --- decoder plugins ---
    def nussinov(self, p, q, th, w=0.0):
        p = np.ascontiguousarray(p, np.float32)
        L = p.shape[0]
        qq = None if q is None else np.ascontiguousarray(q, np.float32)
        ss = np.zeros(L, np.uint32)
        score = C.c_float()
        check(_nussinov_decode(self._h, th, w, L, p.ctypes.data, None if qq is None else qq.ctypes.data,
                               ss.ctypes.data, C.byref(score)))
        return np.float32(score.value), ss

    def nussinov_levels(self, p, ths):
        """dafs_hip_nussinov_decode_levels: the level-by-level decode of the dense matrix p at the thresholds ths (one per
        level, at most MAX_LEVELS); returns (scores[len(ths)], ss, level)"""
        p = np.ascontiguousarray(p, np.float32)
        th = np.ascontiguousarray(ths, np.float32).reshape(-1)
        L = p.shape[0]
        ss = np.zeros(L, np.uint32)
        level = np.zeros(L, np.uint8)
        score = np.zeros(max(len(th), 1), np.float32)
        check(_nussinov_decode_levels(self._h, len(th), th.ctypes.data, L, p.ctypes.data, ss.ctypes.data, level.ctypes.data, score.ctypes.data))
        return score[:len(th)], ss, level

    def nussinov_auto(self, p, auto):
        """dafs_hip_nussinov_decode_auto: the level-by-level decode of the dense matrix p with every level's threshold chosen
        from auto's candidates (an AutoThresholds); returns (scores[auto.levels], ss, level, AutoChoice)"""
        p = np.ascontiguousarray(p, np.float32)
        L, K, cand = p.shape[0], auto.levels, auto.candidates
        ss = np.zeros(L, np.uint32)
        level = np.zeros(L, np.uint8)
        score = np.zeros(K, np.float32)
        o = _AutoArrays(1, K, len(cand))
        check(_nussinov_decode_auto(self._h, K, len(cand), cand.ctypes.data, L, p.ctypes.data, ss.ctypes.data, level.ctypes.data,
                                    score.ctypes.data, *o.pointers()))
        return score, ss, level, o.choice(auto, 0)

    def nussinov_dense(self, p, q, th, w=0.0):
        """the dense Nussinov class (q None: the final-decode overload); returns (score, ss)"""
        p = np.ascontiguousarray(p, np.float32)
        q = None if q is None else np.ascontiguousarray(q, np.float32)
        ss = np.zeros(p.shape[0], np.uint32)
        s = C.c_float()
        check(_nussinov_decode_dense(self._h, th, w, p.shape[0], p.ctypes.data, None if q is None else q.ctypes.data, ss.ctypes.data, C.byref(s)))
        return np.float32(s.value), ss

    def nw_dense(self, p, q, th):
        p = np.ascontiguousarray(p, np.float32)
        q = None if q is None else np.ascontiguousarray(q, np.float32)
        al = np.zeros(p.shape[0], np.uint32)
        s = C.c_float()
        check(_nw_decode_dense(self._h, th, p.shape[0], p.shape[1], p.ctypes.data, None if q is None else q.ctypes.data, al.ctypes.data, C.byref(s)))
        return np.float32(s.value), al

    def nw_envelope(self, p, th):
        p = np.ascontiguousarray(p, np.float32)
        env = np.zeros(2 * (p.shape[0] + 1), np.uint32)
        check(_nw_envelope(self._h, th, p.shape[0], p.shape[1], p.ctypes.data, env.ctypes.data))
        return env

    def nw(self, p, q, th, env=None):
        p = np.ascontiguousarray(p, np.float32)
        if env is None:
            env = self.nw_envelope(p, th)
        qq = None if q is None else np.ascontiguousarray(q, np.float32)
        al = np.zeros(p.shape[0], np.uint32)
        score = C.c_float()
        check(_nw_decode(self._h, th, p.shape[0], p.shape[1], p.ctypes.data, None if qq is None else qq.ctypes.data,
                         env.ctypes.data, al.ctypes.data, C.byref(score)))
        return np.float32(score.value), al

    # --- fused node solver ---
    def solve_nodes(self, nodes, prm=None):
        """nodes: list of (seq1, mask1, seq2, mask2) with seq* uint32 arrays and mask* uint8 [n, len], or
        (seq1, mask1, seq2, mask2, p_x, p_y) with supplied base-pairing matrices.
        Returns list of dicts x, y, z, score, ncbp, iterations, violated."""
        if prm is None:
            prm = dd_params()
        n = len(nodes)
        ins, keep = _node_inputs(nodes)
        outs = (NodeOutput * n)()
        xyz = []
        for b, k in enumerate(keep):
            x = np.zeros(k[2].shape[1], np.uint32); y = np.zeros(k[3].shape[1], np.uint32); z = np.zeros(k[2].shape[1], np.uint32)
            xyz.append((x, y, z))
            outs[b].x, outs[b].y, outs[b].z = x.ctypes.data, y.ctypes.data, z.ctypes.data
        check(_solve_nodes(self._h, n, ins, C.byref(prm), outs))
        return [dict(x=x, y=y, z=z, score=np.float32(outs[b].score), ncbp=outs[b].ncbp, iterations=outs[b].iterations,
                     violated=outs[b].violated) for b, (x, y, z) in enumerate(xyz)]

    def set_mp(self, nnz, rowptr, col, val):
        """Supplied matching probabilities (--align-aux, or the shards of several GPUs after their all-gather): per
        pair x<y in row-major order nnz[p], then len[x]+1 relative row pointers, then the (col, val) entries."""
        nnz = np.ascontiguousarray(nnz, np.uint32); rowptr = np.ascontiguousarray(rowptr, np.uint32)
        col = np.ascontiguousarray(col, np.uint32); val = np.ascontiguousarray(val, np.float32)
        check(_set_mp(self._h, nnz.ctypes.data, rowptr.ctypes.data, col.ctypes.data, val.ctypes.data))

    # --- resident nodes (no level barrier) ---
    def nodes_open(self, nodes, prm):
        """nodes as in solve_nodes; returns their handles and their (len1, len2)"""
        n = len(nodes)
        ins, keep = _node_inputs(nodes)
        handles = np.zeros(n, np.uint32)
        check(_nodes_open(self._h, n, ins, C.byref(prm), handles.ctypes.data))
        lens = [(k[2].shape[1], k[3].shape[1]) for k in keep]
        self._node_lens.update(zip((int(h) for h in handles), lens))
        return [int(h) for h in handles], lens

    def nodes_advance(self, handles, prm, max_iterations):
        """one launch: at most max_iterations more iterations for every listed node; returns the finished flags"""
        h = np.ascontiguousarray(handles, np.uint32)
        fin = np.zeros(len(h), np.uint8)
        check(_nodes_advance(self._h, len(h), h.ctypes.data, C.byref(prm), max_iterations, fin.ctypes.data))
        return fin.astype(bool)

    def nodes_round(self, new_nodes, old_handles, prm, max_iterations, budget_us=0):
        """one round: the open nodes (old_handles) advance while new_nodes (as in solve_nodes) are opened and started beside
        them; at most max_iterations iterations each and, with budget_us, a common stop budget_us microseconds after the
        round began.  Returns (handles of the new nodes, their (len1, len2), finished flags of the old, of the new)."""
        n = len(new_nodes)
        ins, keep = _node_inputs(new_nodes)
        nh = np.zeros(max(n, 1), np.uint32)
        h = np.ascontiguousarray(old_handles, np.uint32)
        fo = np.zeros(max(len(h), 1), np.uint8); fn = np.zeros(max(n, 1), np.uint8)
        check(_nodes_round(self._h, n, ins, nh.ctypes.data, len(h), h.ctypes.data if len(h) else None, C.byref(prm), max_iterations,
                           budget_us, fo.ctypes.data, fn.ctypes.data))
        lens = [(k[2].shape[1], k[3].shape[1]) for k in keep]
        self._node_lens.update(zip((int(x) for x in nh[:n]), lens))
        return ([int(x) for x in nh[:n]], lens, fo[:len(h)].astype(bool), fn[:n].astype(bool))

    def nodes_result(self, handle, len1, len2):
        out = NodeOutput()
        x = np.zeros(len1, np.uint32); y = np.zeros(len2, np.uint32); z = np.zeros(len1, np.uint32)
        out.x, out.y, out.z = x.ctypes.data, y.ctypes.data, z.ctypes.data
        check(_nodes_result(self._h, handle, C.byref(out)))
        return dict(x=x, y=y, z=z, score=np.float32(out.score), ncbp=out.ncbp, iterations=out.iterations, violated=out.violated)

    def node_peek(self, handle, what):
        """dafs_hip_node_peek: a copy of array `what` (a name of NODE_PEEK) of the open node `handle`, as the set-up kernels left
        it -- flat, but the matrices and dense maps in their shape and cbp as [pairs, 8]"""
        if what not in NODE_PEEK:
            raise DafsHipError("node_peek: unknown array %r" % (what,))
        len1, len2 = self._node_lens.get(handle, (0, 0))  # an unknown handle: the library refuses it
        cells = {"p_x": (len1, len1), "p_y": (len2, len2), "p_z": (len1, len2), "x_map": (len1, len1), "y_map": (len2, len2), "zmap": (len1, len2)}
        words = max(len1, len2) ** 2 + 2 * (max(len1, len2) + 130)  # no array of a node is longer, cbp apart
        if what == "cbp":  # as many pairs as the node's own counts say
            n = self.node_peek(handle, "cbp_cnt")
            words = 8 * (int(n[-1]) if len(n) else 0) + 8
        buf = np.zeros(words, _NODE_PEEK_TYPE.get(what, np.uint32))
        got = C.c_uint64()
        check(_node_peek(self._h, handle, NODE_PEEK.index(what), buf.ctypes.data, buf.nbytes, C.byref(got)))
        out = buf[:got.value // 4].copy()
        return out.reshape(cells[what]) if what in cells else out.reshape(-1, 8) if what == "cbp" else out

    def nodes_close(self):
        check(_nodes_close(self._h))
        self._node_lens.clear()

    def nodes_memory(self):
        """(reserved, in_use, peak) bytes of the resident nodes' device memory"""
        r, u, p = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(_nodes_memory(self._h, C.byref(r), C.byref(u), C.byref(p)))
        return r.value, u.value, p.value

    def stage_timing(self, enable=True):
        """per-kernel device timings on / off (dafs_hip_stage_timing: HIP events around every launch of the library)"""
        check(_stage_timing(self._h, 1 if enable else 0))

    def stage_report(self):
        """{kernel: (ms summed over its launches, longest launch ms, launches)} since the last report"""
        buf = (StageTime * 64)()
        n = C.c_uint32()
        check(_stage_report(self._h, buf, 64, C.byref(n)))
        return {buf[k].kernel.decode(): (buf[k].ms, buf[k].longest_ms, buf[k].launches) for k in range(min(n.value, 64))}

    def nodes_demotions(self):
        """split-mode nodes that lost their folding workgroups and went on in the one-workgroup form (since nodes_close)"""
        n = C.c_uint32()
        check(_nodes_demotions(self._h, C.byref(n)))
        return n.value

    def update_basepairing(self, seq, mask, ss):
        """DAFS::update_basepairing_probability (--bp-update): the L x L matrix re-estimated under the structure ss"""
        seq = np.ascontiguousarray(seq, np.uint32); mask = np.ascontiguousarray(mask, np.uint8)
        ss = np.ascontiguousarray(ss, np.uint32)
        n, L = mask.shape
        p = np.zeros((L, L), np.float32)
        check(_update_basepairing(self._h, n, L, seq.ctypes.data, mask.ctypes.data, ss.ctypes.data, p.ctypes.data))
        return p

    def consensus_structure(self, seq, mask, th, want_p=False):
        seq = np.ascontiguousarray(seq, np.uint32); mask = np.ascontiguousarray(mask, np.uint8)
        n, L = mask.shape
        ss = np.zeros(L, np.uint32)
        score = C.c_float()
        p = np.zeros((L, L), np.float32) if want_p else None
        check(_consensus_structure(self._h, n, L, seq.ctypes.data, mask.ctypes.data, th, ss.ctypes.data, C.byref(score),
                                   None if p is None else p.ctypes.data))
        return np.float32(score.value), ss, p

    def consensus_structures(self, alignments, th):
        """dafs_hip_consensus_structures: the common structures of many alignments in one call.  alignments: a list of
        (seq, mask) as consensus_structure takes them; returns a list of (score, ss), each what consensus_structure gives.
        th a sequence of thresholds: dafs_hip_consensus_structures_levels, one level per threshold; returns a list of
        (scores[len(th)], ss, level).
        th an AutoThresholds: dafs_hip_consensus_structures_auto, every level's threshold chosen from its candidates; returns a
        list of (scores[th.levels], ss, level, AutoChoice)."""
        als = [(np.ascontiguousarray(s, np.uint32).reshape(-1), np.ascontiguousarray(m, np.uint8)) for s, m in alignments]
        if any(m.ndim != 2 or m.shape[0] != len(s) for s, m in als):
            raise ValueError("consensus_structures: every alignment is (seq[n], mask[n, len])")
        if isinstance(th, AutoThresholds):
            return self._consensus_structures_auto(als, th)
        if np.ndim(th) != 0:
            return self._consensus_structures_levels(als, np.ascontiguousarray(th, np.float32).reshape(-1))
        if not als:
            check(_consensus_structures(self._h, 0, None, None, None, None, th, None, None))
            return []
        n_rows = np.array([m.shape[0] for _, m in als], np.uint32)
        lens = np.array([m.shape[1] for _, m in als], np.uint32)
        seq = np.ascontiguousarray(np.concatenate([s for s, _ in als]), np.uint32)
        mask = np.ascontiguousarray(np.concatenate([m.reshape(-1) for _, m in als]), np.uint8)
        ss = np.zeros(max(int(lens.sum()), 1), np.uint32)
        score = np.zeros(len(als), np.float32)
        check(_consensus_structures(self._h, len(als), n_rows.ctypes.data, lens.ctypes.data, seq.ctypes.data, mask.ctypes.data, th,
                                    ss.ctypes.data, score.ctypes.data))
        cuts = np.cumsum(lens)[:-1]
        return [(sc, x) for sc, x in zip(score, np.split(ss[:int(lens.sum())], cuts))]

    def _consensus_structures_levels(self, als, th):
        K = len(th)
        if not als:
            check(_consensus_structures_levels(self._h, 0, None, None, None, None, K, th.ctypes.data, None, None, None))
            return []
        n_rows = np.array([m.shape[0] for _, m in als], np.uint32)
        lens = np.array([m.shape[1] for _, m in als], np.uint32)
        seq = np.ascontiguousarray(np.concatenate([s for s, _ in als]), np.uint32)
        mask = np.ascontiguousarray(np.concatenate([m.reshape(-1) for _, m in als]), np.uint8)
        total = int(lens.sum())
        ss = np.zeros(max(total, 1), np.uint32)
        level = np.zeros(max(total, 1), np.uint8)
        score = np.zeros(max(len(als) * K, 1), np.float32)
        check(_consensus_structures_levels(self._h, len(als), n_rows.ctypes.data, lens.ctypes.data, seq.ctypes.data, mask.ctypes.data, K,
                                           th.ctypes.data, ss.ctypes.data, level.ctypes.data, score.ctypes.data))
        cuts = np.cumsum(lens)[:-1]
        return [(score[a * K:(a + 1) * K], x, lv) for a, (x, lv) in enumerate(zip(np.split(ss[:total], cuts), np.split(level[:total], cuts)))]

    def _consensus_structures_auto(self, als, auto):
        K, cand = auto.levels, auto.candidates
        if not als:
            check(_consensus_structures_auto(self._h, 0, None, None, None, None, K, len(cand), cand.ctypes.data, *[None] * 9))
            return []
        n_rows = np.array([m.shape[0] for _, m in als], np.uint32)
        lens = np.array([m.shape[1] for _, m in als], np.uint32)
        seq = np.ascontiguousarray(np.concatenate([s for s, _ in als]), np.uint32)
        mask = np.ascontiguousarray(np.concatenate([m.reshape(-1) for _, m in als]), np.uint8)
        total = int(lens.sum())
        ss = np.zeros(max(total, 1), np.uint32)
        level = np.zeros(max(total, 1), np.uint8)
        score = np.zeros(len(als) * K, np.float32)
        o = _AutoArrays(len(als), K, len(cand))
        check(_consensus_structures_auto(self._h, len(als), n_rows.ctypes.data, lens.ctypes.data, seq.ctypes.data, mask.ctypes.data, K,
                                         len(cand), cand.ctypes.data, ss.ctypes.data, level.ctypes.data, score.ctypes.data, *o.pointers()))
        cuts = np.cumsum(lens)[:-1]
        return [(score[a * K:(a + 1) * K], x, lv, o.choice(auto, a))
                for a, (x, lv) in enumerate(zip(np.split(ss[:total], cuts), np.split(level[:total], cuts)))]

    def structure_support(self, alignments, structures):
        """dafs_hip_structure_support: how far every row of each alignment keeps the structure given for it.  alignments: a
        list of (seq, mask) as consensus_structures takes them; structures: per alignment its ss (left column -> right
        column, NONE otherwise).  Returns per alignment a dict of arrays with one entry per row, in the given row order: both,
        canonical, half (uint32) and expected (float64), read from the base-pairing store the progressive phase reads."""
        als = [(np.ascontiguousarray(s, np.uint32).reshape(-1), np.ascontiguousarray(m, np.uint8)) for s, m in alignments]
        sss = [np.ascontiguousarray(x, np.uint32).reshape(-1) for x in structures]
        if any(m.ndim != 2 or m.shape[0] != len(s) for s, m in als):
            raise ValueError("structure_support: every alignment is (seq[n], mask[n, len])")
        if len(sss) != len(als) or any(len(x) != m.shape[1] for x, (_, m) in zip(sss, als)):
            raise ValueError("structure_support: one structure per alignment, one entry per column")
        if not als:
            return []
        n_rows = np.array([m.shape[0] for _, m in als], np.uint32)
        lens = np.array([m.shape[1] for _, m in als], np.uint32)
        seq = np.ascontiguousarray(np.concatenate([s for s, _ in als]), np.uint32)
        mask = np.ascontiguousarray(np.concatenate([m.reshape(-1) for _, m in als] + [np.zeros(1, np.uint8)]), np.uint8)
        ss = np.ascontiguousarray(np.concatenate(sss + [np.zeros(1, np.uint32)]), np.uint32)
        R = max(int(n_rows.sum()), 1)
        out = dict(both=np.zeros(R, np.uint32), canonical=np.zeros(R, np.uint32), half=np.zeros(R, np.uint32), expected=np.zeros(R, np.float64))
        check(_structure_support(self._h, len(als), n_rows.ctypes.data, lens.ctypes.data, seq.ctypes.data, mask.ctypes.data, ss.ctypes.data,
                                 *[out[k].ctypes.data for k in ("both", "canonical", "half", "expected")]))
        cuts = np.cumsum(n_rows)[:-1]
        per = {k: np.split(v[:int(n_rows.sum())], cuts) for k, v in out.items()}
        return [{k: per[k][a] for k in per} for a in range(len(als))]

    def alignment_reliability(self, seq, mask, ss=None, mp_relaxed=None, bp_relaxed=None):
        """Reliability of the alignment (seq, mask) from the context's stores (dafs_hip_alignment_reliability).  ss: the
        consensus structure (left column -> right column, NONE otherwise) or None.  mp_relaxed / bp_relaxed: 0, 1, or None
        for the store the progressive phase reads.  Returns a dict of numpy arrays: residue (float64, the rows' residues
        one row after another in the given order), col (per column), pair and pair_rows (at the left column of each pair),
        and expected_accuracy (a float)."""
        seq = np.ascontiguousarray(seq, np.uint32); mask = np.ascontiguousarray(mask, np.uint8)
        n, L = mask.shape
        ss = None if ss is None else np.ascontiguousarray(ss, np.uint32)
        if ss is not None and ss.shape != (L,):
            raise ValueError("alignment_reliability: ss needs one entry per column")
        res = np.zeros(int(mask.astype(bool).sum()), np.float64)
        col = np.zeros(L, np.float64); pair = np.zeros(L, np.float64); rows = np.zeros(L, np.uint32)
        ea = C.c_double()
        check(_alignment_reliability(self._h, n, L, seq.ctypes.data, mask.ctypes.data, None if ss is None else ss.ctypes.data,
                                     -1 if mp_relaxed is None else int(mp_relaxed), -1 if bp_relaxed is None else int(bp_relaxed),
                                     res.ctypes.data, col.ctypes.data, pair.ctypes.data, rows.ctypes.data, C.byref(ea)))
        return dict(residue=res, col=col, pair=pair, pair_rows=rows, expected_accuracy=ea.value)

    def alignment_reliabilities(self, alns, sss=None, want=None, mp_relaxed=None, bp_relaxed=None, residue=None):
        """dafs_hip_alignment_reliabilities: the reliability of many alignments in one call.  alns: a list of (seq, mask) as
        consensus_structures takes them; sss: per alignment its ss or None (no pairs), or None for no pairs anywhere; want:
        per alignment a bool per row (None: every row of it), or None for every row; mp_relaxed / bp_relaxed as in
        alignment_reliability.  Returns per alignment the dict alignment_reliability returns for it, bit for bit; the residue
        values of a row that is not wanted keep what `residue` held (a writable C-contiguous float64 array over all residues,
        written in place and refused otherwise; default zeros), and col and expected_accuracy of an alignment with such a row
        are NaN."""
        als = [(np.ascontiguousarray(s, np.uint32).reshape(-1), np.ascontiguousarray(m, np.uint8)) for s, m in alns]
        if any(m.ndim != 2 or m.shape[0] != len(s) for s, m in als):
            raise ValueError("alignment_reliabilities: every alignment is (seq[n], mask[n, len])")
        if sss is not None and (len(sss) != len(als) or any(x is not None and np.shape(x) != (m.shape[1],) for x, (_, m) in zip(sss, als))):
            raise ValueError("alignment_reliabilities: one structure per alignment, one entry per column")
        if want is not None and (len(want) != len(als) or any(x is not None and np.shape(x) != (len(s),) for x, (s, _) in zip(want, als))):
            raise ValueError("alignment_reliabilities: one want entry per row")
        if not als:
            return []
        n_rows = np.array([m.shape[0] for _, m in als], np.uint32)
        lens = np.array([m.shape[1] for _, m in als], np.uint32)
        seq = np.ascontiguousarray(np.concatenate([s for s, _ in als]), np.uint32)
        mask = np.ascontiguousarray(np.concatenate([m.reshape(-1) for _, m in als]), np.uint8)
        ss = None
        if sss is not None and any(x is not None for x in sss):
            ss = np.ascontiguousarray(np.concatenate([np.full(m.shape[1], 0xFFFFFFFF, np.uint32) if x is None else np.asarray(x, np.uint32)
                                                      for x, (_, m) in zip(sss, als)]), np.uint32)
        w8 = None
        if want is not None and any(x is not None for x in want):
            w8 = np.ascontiguousarray(np.concatenate([np.ones(len(s), np.uint8) if x is None else np.asarray(x, bool).astype(np.uint8)
                                                      for x, (s, _) in zip(want, als)]), np.uint8)
        nres = [m.astype(bool).sum(1) for _, m in als]  # per alignment, per row
        total, L = int(sum(int(x.sum()) for x in nres)), int(lens.sum())
        res = np.zeros(max(total, 1), np.float64) if residue is None else residue
        if residue is not None and not (isinstance(res, np.ndarray) and res.dtype == np.float64 and res.flags.c_contiguous and res.flags.writeable
                                        and res.shape == (total,)):  # written in place: no copy may stand in for it
            raise ValueError("alignment_reliabilities: residue is a writable C-contiguous float64 array with one entry per residue of every row")
        col = np.zeros(max(L, 1), np.float64); pair = np.zeros(max(L, 1), np.float64); rows = np.zeros(max(L, 1), np.uint32)
        ea = np.zeros(len(als), np.float64)
        check(_alignment_reliabilities(self._h, len(als), n_rows.ctypes.data, lens.ctypes.data, seq.ctypes.data, mask.ctypes.data,
                                       None if ss is None else ss.ctypes.data, None if w8 is None else w8.ctypes.data,
                                       -1 if mp_relaxed is None else int(mp_relaxed), -1 if bp_relaxed is None else int(bp_relaxed),
                                       res.ctypes.data, col.ctypes.data, pair.ctypes.data, rows.ctypes.data, ea.ctypes.data))
        rcut = np.cumsum([int(x.sum()) for x in nres])[:-1]
        ccut = np.cumsum(lens)[:-1]
        per = [np.split(v[:n], cut) for v, n, cut in ((res, total, rcut), (col, L, ccut), (pair, L, ccut), (rows, L, ccut))]
        return [dict(residue=per[0][a], col=per[1][a], pair=per[2][a], pair_rows=per[3][a], expected_accuracy=float(ea[a]))
                for a in range(len(als))]


    def alignment_covariation(self, rows, ss=None, shuffles=100, seed=1, matrix=False, null="shuffle", tree=None):
        """Covariation statistics of an alignment (dafs_hip_alignment_covariation_null).  rows: the text
        rows, or their codes (uint8 [n, len], encode_alignment).  ss: the consensus structure or None.  shuffles, seed: how
        many null alignments stand behind the E-values (0: no null, every E is NaN) and their seed.  null: one of COV_NULLS,
        "shuffle" (every column permuted on its own; it ignores phylogeny) or "tree" (the substitutions of every branch of a
        tree over the rows, moved to other columns); tree: with "tree", a (left, right) pair in build_tree's layout, None for
        average linkage on the rows' identities.  Returns a dict of numpy arrays per column: col_sum (int64), best,
        best_score, best_e, and at the left column of each pair of ss pair_score, pair_e, pair_rows, pair_canonical,
        pair_types; total (int); with matrix, g (int64 [len, len])."""
        code = _cov_codes(rows, "alignment_covariation")
        n, L = code.shape
        which, left, right = _cov_null(null, tree, n, "alignment_covariation")
        ss = None if ss is None else np.ascontiguousarray(ss, np.uint32)
        if ss is not None and ss.shape != (L,):
            raise ValueError("alignment_covariation: ss needs one entry per column")
        out = dict(col_sum=np.zeros(L, np.int64), best=np.zeros(L, np.uint32), best_score=np.zeros(L, np.float64),
                   best_e=np.zeros(L, np.float64), pair_score=np.zeros(L, np.float64), pair_e=np.zeros(L, np.float64),
                   pair_rows=np.zeros(L, np.uint32), pair_canonical=np.zeros(L, np.uint32), pair_types=np.zeros(L, np.uint32))
        total = C.c_int64()
        g = np.zeros((L, L), np.int64) if matrix else None
        check(_alignment_covariation_null(self._h, n, L, code.ctypes.data, None if ss is None else ss.ctypes.data, int(shuffles), int(seed),
                                          which, None if left is None else left.ctypes.data, None if right is None else right.ctypes.data,
                                          *[out[k].ctypes.data for k in ("col_sum", "best", "best_score", "best_e", "pair_score", "pair_e",
                                                                          "pair_rows", "pair_canonical", "pair_types")],
                                          C.byref(total), None if g is None else g.ctypes.data))
        out["total"] = total.value
        if matrix:
            out["g"] = g
        return out

    def covariation_null_alignment(self, rows, k, null="shuffle", tree=None, seed=1):
        """Null alignment k (0-based) behind the E-values of alignment_covariation(rows, seed=seed, null=null, tree=tree), as
        codes (uint8 [n, len]; dafs_hip_covariation_null_alignment)."""
        code = _cov_codes(rows, "covariation_null_alignment")
        n, L = code.shape
        which, left, right = _cov_null(null, tree, n, "covariation_null_alignment")
        out = np.zeros((n, L), np.uint8)
        check(_covariation_null_alignment(self._h, n, L, code.ctypes.data, which, None if left is None else left.ctypes.data,
                                          None if right is None else right.ctypes.data, int(seed), int(k), out.ctypes.data))
        return out


    def alignment_identity(self, rows, use=None, cand=None, nr=None, matrix=False, nearest=True):
        """How identical the rows of an alignment are (dafs_hip_alignment_identity).  rows: the text
        rows, or their cells (uint8 [n, len], encode_cells).  use: the columns that count (None: all); cand: the rows that may
        be somebody's nearest (None: all); nr: the threshold of the redundancy bit matrix (None: none); matrix: the whole
        ident and aligned matrices too; nearest=False: no nearest rows (their pass is not run; the three arrays and
        pid_nearest are absent).  Returns an Identity."""
        cell = _cells(rows, "alignment_identity")
        n, L = cell.shape
        use = _byte_mask(use, L, "alignment_identity", "use needs one entry per column")
        cand = _byte_mask(cand, n, "alignment_identity", "cand needs one entry per row")
        if nr is not None and not (0.0 < float(nr) <= 1.0):
            raise ValueError(alistat_refusal(NR_THRESHOLD))
        out = Identity()
        out.res = np.zeros(n, np.uint32)
        near = [np.zeros(n, np.uint32) for _ in range(3)] if nearest else [None] * 3
        ident = np.zeros((n, n), np.uint32) if matrix else None
        aligned = np.zeros((n, n), np.uint32) if matrix else None
        red = np.zeros((n, (n + 31) // 32), np.uint32) if nr is not None else None
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        check(_alignment_identity(self._h, n, L, cell.ctypes.data, ptr(use), ptr(cand), 0.0 if nr is None else float(nr), ptr(out.res),
                                  ptr(ident), ptr(aligned), ptr(near[0]), ptr(near[1]), ptr(near[2]), ptr(red)))
        if nearest:
            out.nearest, out.nearest_ident, out.nearest_den = near
            with np.errstate(invalid="ignore", divide="ignore"):
                out.pid_nearest = np.where(out.nearest == NONE, np.nan, out.nearest_ident.astype(np.float64) / out.nearest_den.astype(np.float64))
        if matrix:
            out.ident, out.aligned = ident, aligned
        if nr is not None:
            out.red = red
        return out

    def alignment_weights(self, rows, use=None):
        """Position-based sequence weights of an alignment's rows (dafs_hip_alignment_weights): float64 [n]"""
        cell = _cells(rows, "alignment_weights")
        n, L = cell.shape
        use = _byte_mask(use, L, "alignment_weights", "use needs one entry per column")
        weight = np.zeros(n, np.float64)
        check(_alignment_weights(self._h, n, L, cell.ctypes.data, None if use is None else use.ctypes.data, weight.ctypes.data))
        return weight

    def alignment_compare(self, ref_rows, test_rows, use_ref=None, use_test=None, ss_ref=None, ss_test=None, pp=None, matrix=False):
        """How far two alignments of the same sequences agree (dafs_hip_alignment_compare).  ref_rows,
        test_rows: the text rows, or their cells (uint8 [n, len], encode_cells), row r of both holding the same residues.
        use_ref, use_test: the aligned columns (None: all).  ss_ref, ss_test: partner arrays (NONE for unpaired), both or
        neither.  pp: the PP classes of the test's cells (uint8 [n, len_test], encode_pp).  matrix: the three pair matrices
        too.  Returns a Comparison."""
        cr = _cells(ref_rows, "alignment_compare")
        ct = _cells(test_rows, "alignment_compare")
        if cr.shape[0] != ct.shape[0]:
            raise ValueError("alignment_compare: both alignments need the same rows")
        n, lr = cr.shape
        lt = ct.shape[1]
        use_ref = _byte_mask(use_ref, lr, "alignment_compare", "use_ref needs one entry per column of the reference")
        use_test = _byte_mask(use_test, lt, "alignment_compare", "use_test needs one entry per column of the test")
        if (ss_ref is None) != (ss_test is None):
            raise ValueError("alignment_compare: the structure part needs ss_ref and ss_test")
        if ss_ref is not None:
            ss_ref = np.ascontiguousarray(ss_ref, np.uint32)
            ss_test = np.ascontiguousarray(ss_test, np.uint32)
            if ss_ref.shape != (lr,) or ss_test.shape != (lt,):
                raise ValueError("alignment_compare: a structure needs one entry per column")
        if pp is not None:
            pp = np.ascontiguousarray(pp, np.uint8)
            if pp.shape != (n, lt):
                raise ValueError("alignment_compare: pp needs one entry per cell of the test")
        u64 = lambda *shape: np.zeros(shape, np.uint64)  # noqa: E731
        arr = dict(residues=np.zeros(n, np.uint32), shared=u64(n), refp=u64(n), testp=u64(n), sps=np.zeros(n), ppv=np.zeros(n), total=u64(3),
                   score=np.zeros(3), k=np.zeros(lr, np.uint32), m=np.zeros(lt, np.uint32), colref=u64(lr), colshared=u64(lr),
                   reproduced=np.zeros(lr, np.uint8), tc=u64(2))
        if matrix:
            arr.update(pair_shared=np.zeros((n, n), np.uint32), pair_refp=np.zeros((n, n), np.uint32), pair_testp=np.zeros((n, n), np.uint32))
        if pp is not None:
            arr.update(pp_count=u64(3, 11))
        if ss_ref is not None:
            arr.update(tp=u64(n), nref=u64(n), ntest=u64(n), ss_total=u64(3))
        o = CompareOut(**{k: v.ctypes.data for k, v in arr.items()})
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        check(_alignment_compare(self._h, n, lr, lt, cr.ctypes.data, ct.ctypes.data, ptr(use_ref), ptr(use_test), ptr(ss_ref), ptr(ss_test),
                                 ptr(pp), C.byref(o)))
        out = Comparison()
        for key in ("residues", "shared", "refp", "testp", "k", "m", "colref", "colshared"):
            setattr(out, key, arr[key])
        out.row_sps, out.row_ppv = arr["sps"], arr["ppv"]
        out.reproduced = arr["reproduced"].astype(bool)
        out.total_shared, out.total_refp, out.total_testp = (int(x) for x in arr["total"])
        out.sps, out.ppv, out.tc = (float(x) for x in arr["score"])
        out.tc_reproduced, out.tc_columns = (int(x) for x in arr["tc"])
        if matrix:
            out.pair_shared, out.pair_refp, out.pair_testp = arr["pair_shared"], arr["pair_refp"], arr["pair_testp"]
        if pp is not None:
            out.pp_residues, out.pp_ref, out.pp_shared = arr["pp_count"]
            with np.errstate(invalid="ignore", divide="ignore"):
                out.pp_accuracy = np.where(out.pp_ref == 0, np.nan, out.pp_shared.astype(np.float64) / out.pp_ref.astype(np.float64))
        if ss_ref is not None:
            out.tp, out.nref, out.ntest = arr["tp"], arr["nref"], arr["ntest"]
            tp, nref, ntest = (int(x) for x in arr["ss_total"])
            out.total_tp, out.total_nref, out.total_ntest = tp, nref, ntest
            nan = float("nan")
            out.sensitivity = float(tp) / float(nref) if nref else nan
            out.ss_ppv = float(tp) / float(ntest) if ntest else nan
            out.f = float(2 * tp) / float(nref + ntest) if nref + ntest else nan
        return out


def fold_complementary(a, b):
    """True when CONTRAfold can pair the two residues: AU, GC, GU in either order and case; T is not U in its alphabet"""
    return bool(_fold_complementary(a.encode("latin-1"), b.encode("latin-1")))


def row_constraint(mask_row, ss, residues):
    """dafs_host_row_constraint: the folding constraint the structure ss (left column -> right column, NONE otherwise) puts on
    the row whose residues `residues` lie at the non-zero columns of mask_row: '?' everywhere, '(' and ')' at the residues of a
    pair the row holds both ends of when they are complementary and at least 4 apart."""
    m = np.ascontiguousarray(mask_row, np.uint8).reshape(-1)
    ss = np.ascontiguousarray(ss, np.uint32).reshape(-1)
    if ss.shape != m.shape:
        raise ValueError("row_constraint: one structure entry per column")
    b = residues.encode("latin-1") if isinstance(residues, str) else bytes(residues)
    if b"\0" in b:
        raise ValueError("row_constraint: the residues hold a NUL byte")
    buf = C.create_string_buffer(int(m.astype(bool).sum()) + 1)
    check(_row_constraint(len(m), m.ctypes.data if len(m) else None, ss.ctypes.data if len(m) else None, b, buf))
    return buf.value.decode("latin-1")


def row_constraint_levels(mask_row, ss, level, nlevels, residues):
    """dafs_host_row_constraint_levels: one constraint per level of a structure with levels (level: per
    column the pair's level, 0xFF at unpaired columns).  Returns a list of nlevels strings: string k forces the pairs of level
    k as row_constraint does and puts '.' at both residues of a pair of another level that the row holds both ends of; a
    string k >= 1 that forces nothing is "" (the row is not folded for that level)."""
    m = np.ascontiguousarray(mask_row, np.uint8).reshape(-1)
    ss = np.ascontiguousarray(ss, np.uint32).reshape(-1)
    level = np.ascontiguousarray(level, np.uint8).reshape(-1)
    if ss.shape != m.shape or level.shape != m.shape:
        raise ValueError("row_constraint_levels: one structure entry and one level per column")
    b = residues.encode("latin-1") if isinstance(residues, str) else bytes(residues)
    if b"\0" in b:
        raise ValueError("row_constraint_levels: the residues hold a NUL byte")
    nlevels = int(nlevels)
    if not 1 <= nlevels <= MAX_LEVELS:
        raise ValueError("row_constraint_levels: 1 to %d levels" % MAX_LEVELS)
    stride = int(m.astype(bool).sum()) + 1
    buf = C.create_string_buffer(stride * nlevels)
    check(_row_constraint_levels(len(m), m.ctypes.data if len(m) else None, ss.ctypes.data if len(m) else None,
                                 level.ctypes.data if len(m) else None, nlevels, b, buf))
    return [C.string_at(C.addressof(buf) + k * stride).decode("latin-1") for k in range(nlevels)]


def build_tree(sim):
    """DAFS::build_tree (host code in the library): (score, left, right) with -1 for leaves"""
    sim = np.ascontiguousarray(sim, np.float32)
    n = sim.shape[0]
    score = np.zeros(2 * n - 1, np.float32); left = np.zeros(2 * n - 1, np.int32); right = np.zeros(2 * n - 1, np.int32)
    check(_build_tree(n, sim.ctypes.data, score.ctypes.data, left.ctypes.data, right.ctypes.data))
    return score, left.astype(np.int64), right.astype(np.int64)


def _cov_codes(rows, who):
    """text rows, or a 2-D integer array of codes (any integer type, checked) -> uint8 [n, len]"""
    if isinstance(rows, np.ndarray) and rows.ndim == 2 and rows.dtype.kind in "iu":
        if rows.size and (rows.min() < 0 or rows.max() > 255):
            raise ValueError("%s: codes must fit a byte (the library refuses a code above 4)" % who)
        return np.ascontiguousarray(rows, np.uint8)
    if isinstance(rows, np.ndarray):
        raise ValueError("%s: rows are text rows or a 2-D integer array of codes" % who)
    return encode_alignment(rows)


def _cov_null(null, tree, n, who):
    """(the library's code of the null, left, right as int32 arrays or None).  What cannot be handed over is a ValueError
    here; everything else (a tree under "shuffle", a malformed tree) is the library's to refuse."""
    if null not in COV_NULLS:
        raise ValueError("%s: unknown null %r (one of %s)" % (who, null, ", ".join(COV_NULLS)))
    if tree is None:
        return COV_NULLS.index(null), None, None
    if len(tree) != 2:
        raise ValueError("%s: tree is a (left, right) pair" % who)
    left, right = (None if a is None else np.ascontiguousarray(a, np.int32) for a in tree)
    for a in (left, right):
        if a is not None and a.shape != (2 * n - 1,):
            raise ValueError("%s: a tree of n rows has 2n - 1 nodes" % who)
    return COV_NULLS.index(null), left, right


def linkage_check(rule, sim=None):
    """The checks of Context.linkage_tree that need no device: (the library's code of `rule`, sim as a contiguous float32 matrix
    or None).  ValueError for an unknown rule, for "guide" (the guide tree is build_tree), for a matrix that is not square or
    is empty, and for a non-finite entry above its diagonal."""
    if rule not in LINKAGES:
        raise ValueError("linkage: unknown rule %r (one of %s)" % (rule, ", ".join(LINKAGES)))
    if rule == "guide":
        raise ValueError("linkage: \"guide\" is the guide tree's own rule: use build_tree")
    if sim is None:
        return LINKAGES.index(rule), None
    sim = np.ascontiguousarray(sim, np.float32)
    if sim.ndim != 2 or sim.shape[0] != sim.shape[1] or sim.shape[0] == 0:
        raise ValueError("linkage: the similarity matrix must be n x n with n >= 1")
    if not np.isfinite(sim[np.triu_indices(sim.shape[0], 1)]).all():
        raise ValueError("linkage: an entry above the diagonal is not finite")
    return LINKAGES.index(rule), sim


def score_check(score, structure_weight=None, who="similarity"):
    """ValueError for an unknown score, a weight outside [0, 1] and a weight given with a score other than "mix"
    (structure_weight None: not given)"""
    if score not in SCORES:
        raise ValueError("%s: unknown score %r (one of %s)" % (who, score, ", ".join(SCORES)))
    if structure_weight is None:
        return
    if score != "mix":
        raise ValueError("%s: structure_weight is the weight of score=\"mix\"; it was given with score=%r" % (who, score))
    try:
        w = float(structure_weight)
    except (TypeError, ValueError):
        w = float("nan")
    if not 0.0 <= w <= 1.0:
        raise ValueError("%s: structure_weight must lie in 0 .. 1" % who)


def similarity_ranges(lens, max_bytes=None):
    """dafs_host_similarity_ranges (host code in the library): the ranges [begin, end) of the row-major pair enumeration that
    Context.similarity walks for sequences of these lengths under max_bytes (None: the library's budget), as a list"""
    lens = np.ascontiguousarray([int(x) for x in lens], np.uint32)
    budget = 0 if max_bytes is None else int(max_bytes)
    if budget < 0 or (max_bytes is not None and budget == 0):
        raise ValueError("similarity_ranges: max_bytes must be positive (None: the library's budget)")
    count = C.c_uint64()
    check(_similarity_ranges(len(lens), lens.ctypes.data, budget, None, 0, C.byref(count)))
    end = np.zeros(max(count.value, 1), np.uint64)
    check(_similarity_ranges(len(lens), lens.ctypes.data, budget, end.ctypes.data, count.value, C.byref(count)))
    ends = [int(e) for e in end[:count.value]]
    return list(zip([0] + ends[:-1], ends))


def _tree_arrays(tree, who):
    """(score, left, right) of build_tree as the library's arrays; n from their length"""
    score, left, right = tree
    score = np.ascontiguousarray(score, np.float32).reshape(-1)
    left = np.ascontiguousarray(left, np.int32).reshape(-1)
    right = np.ascontiguousarray(right, np.int32).reshape(-1)
    if len(score) % 2 != 1 or len(left) != len(score) or len(right) != len(score):
        raise ValueError("%s: a tree of n leaves is three arrays of 2 n - 1 entries" % who)
    return score, left, right, (len(score) + 1) // 2


def cluster_cut(tree, threshold=None, count=None):
    """dafs_host_cluster_cut (host code in the library): the cut of the guide tree `tree` = (score, left,
    right) of build_tree into clusters.  threshold: a join is kept when its score is >= threshold and every join below it is
    kept; count: exactly that many clusters, the joins made last undone.  Exactly one of the two.  Returns (labels as uint32
    [n], the number of clusters); the clusters are numbered by their smallest member.  ValueError for what the library
    refuses."""
    if (threshold is None) == (count is None):
        raise ValueError("cluster_cut: exactly one of threshold and count")
    score, left, right, n = _tree_arrays(tree, "cluster_cut")
    if count is not None and not 0 <= int(count) <= 0xFFFFFFFF:
        raise ValueError("cluster cut: the number of clusters must be 1 .. the number of sequences")
    labels = np.zeros(n, np.uint32)
    k = C.c_uint32()
    rc = _cluster_cut(n, score.ctypes.data, left.ctypes.data, right.ctypes.data, CLUSTER_THRESHOLD if count is None else CLUSTER_COUNT,
                      0.0 if threshold is None else float(threshold), 0 if count is None else int(count), labels.ctypes.data, C.byref(k))
    if rc == -1:
        raise ValueError(_last_error().decode("latin-1"))
    check(rc)
    return labels, k.value


def cluster_table(headers, lengths, labels, tree, sim):
    """dafs_host_cluster_table: the text of `dafs --cluster-table` -- per sequence "i name length cluster size join nearest_in
    sim_in nearest_out sim_out" (1-based indices, floats as %.9g, "0" and "nan" where there is none)"""
    headers = list(headers)
    score, left, right, n = _tree_arrays(tree, "cluster_table")
    lengths = np.ascontiguousarray(lengths, np.uint32).reshape(-1)
    labels = np.ascontiguousarray(labels, np.uint32).reshape(-1)
    sim = np.ascontiguousarray(sim, np.float32)
    if len(headers) != n or len(lengths) != n or len(labels) != n or sim.shape != (n, n):
        raise ValueError("cluster_table: one header, length and label per leaf of the tree and an n x n similarity matrix")
    return host_text(_cluster_table, n, c_strings(headers), lengths.ctypes.data, labels.ctypes.data, score.ctypes.data, left.ctypes.data,
                     right.ctypes.data, sim.ctypes.data)


def phylogeny_refusal(which):
    """what both drivers say when they refuse a combination of the phylogeny options (dafs_host_phylogeny_refusal)"""
    return _phylogeny_refusal(which).decode()


def bootstrap_refusal(which):
    """what both drivers say when they refuse a combination of the bootstrap options (dafs_host_bootstrap_refusal)"""
    return _bootstrap_refusal(which).decode()


def transfer_refusal(which):
    """what both drivers say when they refuse the transfer option (dafs_host_transfer_refusal)"""
    return _transfer_refusal(which).decode()


def split_depth(left, right):
    """dafs_host_split_depth: per node of the tree the depth of its split, the size of the smaller side, as int64 [2n-1]; -1
    for the root and for a split with fewer than two leaves on a side"""
    left = np.ascontiguousarray(left, np.int32).reshape(-1)
    right = np.ascontiguousarray(right, np.int32).reshape(-1)
    T = len(left)
    if T % 2 != 1 or len(right) != T:
        raise ValueError("split_depth: a tree of n leaves has 2n - 1 nodes")
    depth = np.zeros(T, np.int32)
    rc = _split_depth((T + 1) // 2, left.ctypes.data, right.ctypes.data, depth.ctypes.data)
    if rc == -1:
        raise ValueError(_last_error().decode("latin-1"))
    check(rc)
    return depth.astype(np.int64)


def transfer_percent(transfer, depth, B):
    """dafs_host_transfer_percent: the transfer bootstrap expectation of a split in percent, (200 (M - transfer) + M) / (2 M)
    with M = B (depth - 1) in integer division (halves round up).  ValueError for depth < 2, B = 0 or a sum outside 0 .. M."""
    if not (0 <= int(transfer) < 2 ** 63 and 0 <= int(depth) < 2 ** 31 and 0 <= int(B) < 2 ** 32):
        raise ValueError("transfer_percent: a transfer sum, a depth and a number of replicates that are not negative")
    p = _transfer_percent(int(transfer), int(depth), int(B))
    if p < 0:
        raise ValueError("transfer_percent: depth >= 2, B >= 1 and a transfer sum in 0 .. B (depth - 1)")
    return p


def transfer_table(names, left, right, support, transfer, replicates, seed=12345, model="jc"):
    """dafs_host_transfer_table: the text of `dafs --phylogeny-support` under --phylogeny-transfer -- "# rows n replicates B
    seed S model M measure transfer", then per non-trivial split "node support B percent size leaves depth transfer tbe",
    tab-separated"""
    if model not in NJ_MODELS:
        raise ValueError(phylogeny_refusal(PHY_UNKNOWN_MODEL))
    names = list(names)
    n = len(names)
    left = np.ascontiguousarray(left, np.int32).reshape(-1)
    right = np.ascontiguousarray(right, np.int32).reshape(-1)
    support = np.ascontiguousarray(support, np.int32).reshape(-1)
    transfer = np.ascontiguousarray(transfer, np.int64).reshape(-1)
    if n == 0 or any(len(a) != 2 * n - 1 for a in (left, right, support, transfer)):
        raise ValueError("transfer_table: a tree of n names has 2n - 1 nodes")
    return host_text(_transfer_table, n, c_strings(names), left.ctypes.data, right.ctypes.data, support.ctypes.data, transfer.ctypes.data,
                     int(replicates), int(seed) & 0xFFFFFFFFFFFFFFFF, NJ_MODELS.index(model))


def nj_distances(ident, aligned, model="jc"):
    """dafs_host_nj_distances: the float64 [n, n] distances of an alignment's rows from the integer
    matrices of Context.alignment_identity(matrix=True), under the model "jc" (Jukes-Cantor, quantised to 2^-20 and capped at
    3.0) or "p" (the share of differing columns).  A letter outside ACGU counts as a difference."""
    if model not in NJ_MODELS:
        raise ValueError(phylogeny_refusal(PHY_UNKNOWN_MODEL))
    ident = np.ascontiguousarray(ident, np.uint32)
    aligned = np.ascontiguousarray(aligned, np.uint32)
    if ident.ndim != 2 or ident.shape[0] != ident.shape[1] or ident.shape[0] == 0 or aligned.shape != ident.shape:
        raise ValueError("nj_distances: ident and aligned are n x n matrices with n >= 1")
    n = ident.shape[0]
    dist = np.zeros((n, n), np.float64)
    rc = _nj_distances(n, ident.ctypes.data, aligned.ctypes.data, NJ_MODELS.index(model), dist.ctypes.data)
    if rc == -1:
        raise ValueError(_last_error().decode("latin-1"))
    check(rc)
    return dist


def tree_support(left, right, rep_left, rep_right):
    """dafs_host_tree_support (host code in the library): per node of the tree (left, right) the number
    of the replicate trees (rep_left, rep_right: [B, 2n-1]) that hold the node's split, as int64 [2n-1]; -1 for the root and
    for a split with fewer than two leaves on a side.  ValueError for a malformed tree."""
    left = np.ascontiguousarray(left, np.int32).reshape(-1)
    right = np.ascontiguousarray(right, np.int32).reshape(-1)
    rep_left = np.ascontiguousarray(rep_left, np.int32)
    rep_right = np.ascontiguousarray(rep_right, np.int32)
    T = len(left)
    if T % 2 != 1 or len(right) != T or rep_left.ndim != 2 or rep_left.shape[1] != T or rep_right.shape != rep_left.shape:
        raise ValueError("tree_support: a tree of n leaves has 2n - 1 nodes and the replicates are [B, 2n - 1]")
    support = np.zeros(T, np.int32)
    rc = _tree_support((T + 1) // 2, left.ctypes.data, right.ctypes.data, rep_left.shape[0], rep_left.ctypes.data, rep_right.ctypes.data,
                       support.ctypes.data)
    if rc == -1:
        raise ValueError(_last_error().decode("latin-1"))
    check(rc)
    return support.astype(np.int64)


def support_table(names, left, right, support, replicates, seed=12345, model="jc"):
    """dafs_host_support_table: the text of `dafs --phylogeny-support` -- "# rows n replicates B seed S model M", then per
    non-trivial split of the tree "node support B percent size leaves", tab-separated"""
    if model not in NJ_MODELS:
        raise ValueError(phylogeny_refusal(PHY_UNKNOWN_MODEL))
    names = list(names)
    n = len(names)
    left = np.ascontiguousarray(left, np.int32).reshape(-1)
    right = np.ascontiguousarray(right, np.int32).reshape(-1)
    support = np.ascontiguousarray(support, np.int32).reshape(-1)
    if n == 0 or len(left) != 2 * n - 1 or len(right) != 2 * n - 1 or len(support) != 2 * n - 1:
        raise ValueError("support_table: a tree of n names has 2n - 1 nodes")
    return host_text(_support_table, n, c_strings(names), left.ctypes.data, right.ctypes.data, support.ctypes.data, int(replicates),
                     int(seed) & 0xFFFFFFFFFFFFFFFF, NJ_MODELS.index(model))


def newick(names, left, right, length=None, support=None, replicates=None, transfer=None, depth=None):
    """dafs_host_newick: the tree (left, right in build_tree's layout, length per node or None for the topology alone) as one
    Newick line ending in ";\n": "(L:len,R:len)" nested with the left child first, lengths as %.9g, none on the root, names
    quoted where they hold any of ()[]':;, or white space.  ValueError for a malformed tree.  support (per node, -1: none)
    and replicates: dafs_host_newick_support, the support in percent as the label of the joins.
    transfer (per node, -1: none) and replicates: dafs_host_newick_transfer, the transfer bootstrap expectation in percent as
    the labels instead (section 28); depth, if given, must be split_depth(left, right), which the library uses."""
    names = list(names)
    n = len(names)
    left = np.ascontiguousarray(left, np.int32).reshape(-1)
    right = np.ascontiguousarray(right, np.int32).reshape(-1)
    if n == 0 or len(left) != 2 * n - 1 or len(right) != 2 * n - 1:
        raise ValueError("newick: a tree of n names has 2n - 1 nodes")
    if length is not None:
        length = np.ascontiguousarray(length, np.float64).reshape(-1)
        if len(length) != 2 * n - 1:
            raise ValueError("newick: one length per node")
    if transfer is not None:
        transfer = np.ascontiguousarray(transfer, np.int64).reshape(-1)
        if len(transfer) != 2 * n - 1 or replicates is None:
            raise ValueError("newick: one transfer sum per node and the number of replicates")
        if depth is not None and not np.array_equal(np.asarray(depth, np.int64).reshape(-1), split_depth(left, right)):
            raise ValueError("newick: depth is not the depth of the tree's splits")
        return host_text(_newick_transfer, n, c_strings(names), left.ctypes.data, right.ctypes.data,
                         None if length is None else length.ctypes.data, transfer.ctypes.data, int(replicates))
    if support is not None:
        support = np.ascontiguousarray(support, np.int32).reshape(-1)
        if len(support) != 2 * n - 1 or replicates is None:
            raise ValueError("newick: one support value per node and the number of replicates")
        return host_text(_newick_support, n, c_strings(names), left.ctypes.data, right.ctypes.data,
                         None if length is None else length.ctypes.data, support.ctypes.data, int(replicates))
    return host_text(_newick, n, c_strings(names), left.ctypes.data, right.ctypes.data, None if length is None else length.ctypes.data)


def merge_added(ncols, zs):
    """dafs_host_merge_added (host code in the library): k new sequences into a seed of ncols columns from their column maps
    zs (per sequence a uint32 array, NONE for an unmatched residue).  Returns (seed_col, [res_col per sequence], width):
    the merged column of every seed column and of every new residue, and the merged width."""
    lens = np.array([len(z) for z in zs], np.uint32)
    z = np.ascontiguousarray(np.concatenate([np.asarray(z, np.uint32) for z in zs]) if len(zs) else np.zeros(0, np.uint32), np.uint32)
    seed_col = np.zeros(max(ncols, 1), np.uint32)
    res_col = np.zeros(max(len(z), 1), np.uint32)
    width = C.c_uint32()
    check(_merge_added(ncols, len(zs), lens.ctypes.data, z.ctypes.data, seed_col.ctypes.data, res_col.ctypes.data, C.byref(width)))
    cuts = np.cumsum(lens)[:-1] if len(zs) else []
    return seed_col[:ncols], np.split(res_col[:len(z)], cuts) if len(zs) else [], width.value


# ---- host text (dafs_amd/csrc/host_text.cpp, which the command line calls too); stockholm.py and pipeline.py hold the callers ----
def c_strings(strings):
    """a list of str (latin-1) or bytes as a char* array for the library (one entry at least)"""
    bs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in strings]
    if any(b"\0" in b for b in bs):
        raise ValueError("a string for the library holds a NUL byte")
    return (C.c_char_p * max(len(bs), 1))(*bs)


def host_text(fn, *args, outs=1, refusal=ValueError):
    """fn(*args, &text, ...) of a host text function: the returned texts as str (latin-1), freed; a single one as itself.
    DAFS_HIP_EINVAL raises refusal(the library's message)."""
    texts = [C.c_void_p() for _ in range(outs)]
    rc = fn(*args, *[C.byref(t) for t in texts])
    if rc == -1:
        raise refusal(_last_error().decode("latin-1"))
    check(rc)
    try:
        got = [C.string_at(t).decode("latin-1") for t in texts]
    finally:
        for t in texts:
            _host_free(t)
    return got[0] if outs == 1 else got


def split_lines(joined, n):
    """the n strings of a list the library returned joined by newlines"""
    return joined.split("\n") if n else []


def dd_params(**kw):
    p = DDParams()
    _dd_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def make_brackets(ss):
    ss = np.ascontiguousarray(ss, np.uint32)
    buf = C.create_string_buffer(len(ss) + 1)
    _make_brackets(len(ss), ss.ctypes.data, buf)
    return buf.value.decode()


def make_brackets_levels(ss, level):
    """the bracket string of a structure of several levels: "()", "[]", "{}", "<>" for levels 0..3"""
    ss = np.ascontiguousarray(ss, np.uint32)
    level = np.ascontiguousarray(level, np.uint8)
    if len(level) != len(ss):
        raise ValueError("make_brackets_levels: one level per column")
    buf = C.create_string_buffer(len(ss) + 1)
    _make_brackets_levels(len(ss), ss.ctypes.data, level.ctypes.data, buf)
    return buf.value.decode()
