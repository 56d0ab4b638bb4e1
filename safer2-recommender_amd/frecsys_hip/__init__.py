"""frecsys_hip -- ctypes binding of libfrecsys_hip.so (include/frecsys_hip.h).

Thin host-side plumbing over the C-ABI for the Python harnesses (tests,
bench.py, __graft_entry__).  The product's own host layer is C++
(include/frecsys/*.h, tools/run_model.cc); this module adds nothing to the
compute path: every call goes straight to the HIP library, and importing it
without the built library raises (there is no CPU fallback).

Sides / kinds mirror the C-ABI (`SIDE_USER`, `KIND_IALS`, ...).  Arrays are
numpy: CSR row_ptr int64, col int32, embeddings float32 [rows, dim].
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Tuple

import numpy as np

SIDE_USER, SIDE_ITEM, SIDE_EVAL = 0, 1, 2
REC_EXCLUDE_HISTORY = 1
TS_EXACT = 2
SIM_COSINE, SIM_KEEP_SELF = 1, 2
AUD_EXCLUDE_HISTORY = 1
DIV_RAW_SCORES = 2
# the cut-offs and tail levels run_model evaluates (run_model.cc:97-100)
EVAL_K_LIST = (5, 10, 20, 50, 100)
EVAL_ALPHA_LIST = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)
KIND_IALS, KIND_WEIGHTED_U, KIND_WEIGHTED_V, KIND_CVAR_GRAD_U, KIND_CVAR_GRAD_V = range(5)

OK = 0
ERR_INVALID, ERR_HIP, ERR_RCCL, ERR_NOT_SPD, ERR_NAN, ERR_UNSUPPORTED, ERR_NO_DEVICE = range(1, 8)
ERR_IO = 8
SAVE_NO_DATA = 1
LOAD_TABLES_ONLY = 1

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfrecsys_hip.so")
MODEL_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libfrecsys_model.so")

# Every symbol include/frecsys_hip.h declares (checked by the CPU tests).
EXPORTS = (
    "frecsys_device_count", "frecsys_ctx_create", "frecsys_ctx_destroy",
    "frecsys_last_error", "frecsys_last_error_entity", "frecsys_padded_dim",
    "frecsys_partition", "frecsys_comm_unique_id", "frecsys_comm_init",
    "frecsys_shard_range", "frecsys_load_csr", "frecsys_set_embeddings",
    "frecsys_get_embeddings", "frecsys_init_embeddings", "frecsys_snapshot",
    "frecsys_gramian", "frecsys_set_gramian", "frecsys_solve_side", "frecsys_user_loss",
    "frecsys_synchronize", "frecsys_timing", "frecsys_timing_reset", "frecsys_debug_basis",
    "frecsys_eval_topk", "frecsys_train_stats", "frecsys_pp_set_rating_index",
    "frecsys_pp_predict", "frecsys_pp_step", "frecsys_debug_diag_factor",
    "frecsys_history_space_max_h", "frecsys_history_space_max_h_side", "frecsys_comm_world", "frecsys_gram_groups",
    "frecsys_get_gram_groups", "frecsys_set_gram_groups", "frecsys_get_gramian",
    "frecsys_gram_plan", "frecsys_work", "frecsys_snapshot_residual", "frecsys_counter",
    "frecsys_pp_sync", "frecsys_release_workspaces", "frecsys_pp_get_predictions",
    "frecsys_set_transport", "frecsys_recommend", "frecsys_solve_side_cg",
    "frecsys_cg_iterations", "frecsys_list_metrics", "frecsys_metric_cvar",
    "frecsys_rank_metrics", "frecsys_score_pairs", "frecsys_rank_candidates",
    "frecsys_similar", "frecsys_sample_negatives", "frecsys_rank_candidates_metrics",
    "frecsys_sampled_metrics", "frecsys_position_metrics", "frecsys_rank_positions",
    "frecsys_explain", "frecsys_csr_row_lengths", "frecsys_mmr_select", "frecsys_diversify",
    "frecsys_recommend_diverse", "frecsys_list_quality", "frecsys_exposure_summary",
    "frecsys_rank_quality", "frecsys_lists_quality", "frecsys_dpp_select",
    "frecsys_diversify_dpp", "frecsys_recommend_dpp", "frecsys_audience",
    "frecsys_audience_plan", "frecsys_recommend_two_stage", "frecsys_bf16_round",
    "frecsys_two_stage_bound",
)

# Every symbol include/frecsys_model.h declares.
MODEL_EXPORTS = (
    "frecsys_model_config_default", "frecsys_model_create", "frecsys_model_initialize",
    "frecsys_model_train", "frecsys_model_context", "frecsys_model_mean_weight",
    "frecsys_model_destroy", "frecsys_model_last_error", "frecsys_model_dual_state",
    "frecsys_model_recommend", "frecsys_model_recommend_fold_in",
    "frecsys_model_evaluate", "frecsys_model_evaluate_fold_in",
    "frecsys_model_score", "frecsys_model_rank_candidates",
    "frecsys_model_rank_candidates_fold_in",
    "frecsys_model_similar_items", "frecsys_model_similar_users",
    "frecsys_model_evaluate_candidates", "frecsys_model_evaluate_candidates_fold_in",
    "frecsys_model_evaluate_sampled", "frecsys_model_evaluate_sampled_fold_in",
    "frecsys_model_evaluate_ranks", "frecsys_model_evaluate_ranks_fold_in",
    "frecsys_model_save", "frecsys_model_load", "frecsys_model_file_info",
    "frecsys_model_epochs", "frecsys_model_explain", "frecsys_model_explain_fold_in",
    "frecsys_model_recommend_diverse", "frecsys_model_recommend_diverse_fold_in",
    "frecsys_model_diversify", "frecsys_model_evaluate_quality",
    "frecsys_model_evaluate_quality_fold_in", "frecsys_model_list_quality",
    "frecsys_model_recommend_dpp", "frecsys_model_recommend_dpp_fold_in",
    "frecsys_model_diversify_dpp", "frecsys_model_audience",
    "frecsys_model_recommend_two_stage", "frecsys_model_recommend_two_stage_fold_in",
)


class FrecsysError(RuntimeError):
    def __init__(self, code: int, msg: str, entity: int = -1):
        super().__init__(f"frecsys error {code}: {msg}")
        self.code = code
        self.entity = entity


class _Config(ctypes.Structure):
    _fields_ = [("dim", ctypes.c_int32), ("device", ctypes.c_int32),
                ("parity_quirks", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("n_users", ctypes.c_int64), ("n_items", ctypes.c_int64)]


# frecsys_transport (include/frecsys_hip.h)
_ROWS_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int32,
                            ctypes.POINTER(ctypes.c_float), ctypes.c_int64, ctypes.c_int64,
                            ctypes.c_int64, ctypes.c_int64)
_MIN_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64))


class _Transport(ctypes.Structure):
    _fields_ = [("user", ctypes.c_void_p), ("allgather_rows", _ROWS_FN),
                ("allreduce_min_u64", _MIN_FN)]


class _SolveParams(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("reg", ctypes.c_float),
                ("reg_exp", ctypes.c_float), ("unobserved_weight", ctypes.c_float),
                ("alpha", ctypes.c_float), ("stepsize", ctypes.c_float),
                ("from_snapshot", ctypes.c_int32), ("lambda_is_reg", ctypes.c_int32),
                ("entity_weight", ctypes.c_void_p), ("entity_reg", ctypes.c_void_p),
                ("other_weight", ctypes.c_void_p)]


class _CgParams(ctypes.Structure):
    _fields_ = [("max_iterations", ctypes.c_int32), ("tolerance", ctypes.c_float)]


class _ModelConfig(ctypes.Structure):
    _fields_ = [("model_name", ctypes.c_char_p), ("dim", ctypes.c_int32),
                ("l2_reg", ctypes.c_float), ("l2_reg_exp", ctypes.c_float),
                ("uobs_weight", ctypes.c_float), ("stdev", ctypes.c_float),
                ("alpha", ctypes.c_float), ("bandwidth", ctypes.c_float),
                ("stepsize", ctypes.c_float), ("sampling_ratio", ctypes.c_float),
                ("block_size", ctypes.c_int32), ("xi_iterations", ctypes.c_int32),
                ("pd_iterations", ctypes.c_int32), ("use_epanechnikov", ctypes.c_int32),
                ("use_snr", ctypes.c_int32), ("print_train_stats", ctypes.c_int32),
                ("print_residual_stats", ctypes.c_int32), ("print_var_stats", ctypes.c_int32),
                ("seed", ctypes.c_int64), ("device", ctypes.c_int32),
                ("parity_quirks", ctypes.c_int32), ("world", ctypes.c_int32),
                ("rank", ctypes.c_int32), ("comm_id", ctypes.c_void_p),
                ("use_cg", ctypes.c_int32), ("cg_error_tolerance", ctypes.c_float),
                ("cg_max_iterations", ctypes.c_int32)]


class _ModelFileInfo(ctypes.Structure):
    _fields_ = [("model_name", ctypes.c_char * 16), ("config", _ModelConfig),
                ("n_users", ctypes.c_int64), ("n_items", ctypes.c_int64),
                ("n_tuples", ctypes.c_int64), ("epochs_trained", ctypes.c_int64),
                ("flags", ctypes.c_uint64), ("tuples_checksum", ctypes.c_uint64),
                ("version", ctypes.c_uint32)]


_lib = None
_model_lib = None


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libfrecsys_hip.so; raises if it was not built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise FrecsysError(ERR_INVALID, f"{path} missing: run __graft_entry__.build() / make")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    P, I32, I64, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    sig = {
        "frecsys_device_count": (ctypes.c_int, [P]),
        "frecsys_ctx_create": (ctypes.c_int, [P, P]),
        "frecsys_ctx_destroy": (None, [P]),
        "frecsys_last_error": (ctypes.c_char_p, [P]),
        "frecsys_last_error_entity": (I64, [P]),
        "frecsys_padded_dim": (I32, [I32]),
        "frecsys_partition": (ctypes.c_int, [I64, P, I32, P]),
        "frecsys_comm_unique_id": (ctypes.c_int, [P]),
        "frecsys_comm_init": (ctypes.c_int, [P, I32, I32, P]),
        "frecsys_shard_range": (ctypes.c_int, [P, I32, P, P]),
        "frecsys_load_csr": (ctypes.c_int, [P, I32, I64, P, P]),
        "frecsys_set_embeddings": (ctypes.c_int, [P, I32, P, I64]),
        "frecsys_get_embeddings": (ctypes.c_int, [P, I32, P, I64]),
        "frecsys_init_embeddings": (ctypes.c_int, [P, ctypes.c_uint32, F]),
        "frecsys_snapshot": (ctypes.c_int, [P, I32]),
        "frecsys_gramian": (ctypes.c_int, [P, I32, P, I32, P]),
        "frecsys_set_gramian": (ctypes.c_int, [P, I32, P, I64]),
        "frecsys_solve_side": (ctypes.c_int, [P, I32, P]),
        "frecsys_user_loss": (ctypes.c_int, [P, I32, F, I32, P]),
        "frecsys_synchronize": (ctypes.c_int, [P]),
        "frecsys_timing": (ctypes.c_int, [P, ctypes.c_char_p, P, P]),
        "frecsys_timing_reset": (ctypes.c_int, [P]),
        "frecsys_history_space_max_h": (I32, [P]),
        "frecsys_history_space_max_h_side": (I32, [P, I32]),
        "frecsys_comm_world": (ctypes.c_int, [P, P, P, P]),
        "frecsys_gram_groups": (ctypes.c_int, [P, I32, P, P, P, P]),
        "frecsys_get_gram_groups": (ctypes.c_int, [P, I32, P]),
        "frecsys_set_gram_groups": (ctypes.c_int, [P, I32, P]),
        "frecsys_get_gramian": (ctypes.c_int, [P, I32, P, I64]),
        "frecsys_gram_plan": (ctypes.c_int, [I32, I64, I32, I32, P, P, P, P, P]),
        "frecsys_work": (ctypes.c_int, [P, ctypes.c_char_p, P, P, P, P]),
        "frecsys_debug_basis": (ctypes.c_int, [P, I32, P, P, P]),
        "frecsys_debug_diag_factor": (ctypes.c_int, [P, I32, I32, P, P, P]),
        "frecsys_eval_topk": (ctypes.c_int, [P, I32, P]),
        "frecsys_train_stats": (ctypes.c_int, [P, P, P, P, P]),
        "frecsys_pp_set_rating_index": (ctypes.c_int, [P, I32, P]),
        "frecsys_pp_predict": (ctypes.c_int, [P, I32]),
        "frecsys_pp_step": (ctypes.c_int, [P, I32, I32, I32, P, P]),
        "frecsys_snapshot_residual": (ctypes.c_int, [P, I32, P]),
        "frecsys_counter": (ctypes.c_int, [P, ctypes.c_char_p, P]),
        "frecsys_pp_sync": (ctypes.c_int, [P, I32]),
        "frecsys_release_workspaces": (ctypes.c_int, [P]),
        "frecsys_pp_get_predictions": (ctypes.c_int, [P, I32, P]),
        "frecsys_set_transport": (ctypes.c_int, [P, P]),
        "frecsys_recommend": (ctypes.c_int, [P, I32, P, I64, I32, I32, P, P, P]),
        "frecsys_solve_side_cg": (ctypes.c_int, [P, I32, P, P]),
        "frecsys_cg_iterations": (ctypes.c_int, [P, I32, P]),
        "frecsys_list_metrics": (ctypes.c_int, [P, I64, I32, P, P, P, I32, P, P]),
        "frecsys_metric_cvar": (ctypes.c_int, [P, I64, P, I32, P]),
        "frecsys_rank_metrics": (ctypes.c_int, [P, I32, P, I64, I32, P, P, P, P, I32, P, P]),
        "frecsys_score_pairs": (ctypes.c_int, [P, I32, P, P, I64, P]),
        "frecsys_rank_candidates": (ctypes.c_int, [P, I32, P, I64, P, P, I32, I32, P, P, P]),
        "frecsys_similar": (ctypes.c_int, [P, I32, P, I64, I32, I32, P, P, P]),
        "frecsys_audience": (ctypes.c_int, [P, P, I64, I32, I32, P, P, P]),
        "frecsys_audience_plan": (ctypes.c_int, [I32, I64, I64, I32, I32, I32, P]),
        "frecsys_sample_negatives": (ctypes.c_int,
                                     [I64, P, P, I64, P, P, P, P, I32, ctypes.c_uint64, P, P]),
        "frecsys_rank_candidates_metrics": (ctypes.c_int,
                                            [P, I32, P, I64, P, P, I32, P, P, P, P, I32, P, P]),
        "frecsys_sampled_metrics": (ctypes.c_int, [P, I32, P, I64, I32, P, P, P, I32,
                                                   ctypes.c_uint64, P, I32, P, P, P, P]),
        "frecsys_position_metrics": (ctypes.c_int, [P, P, P, I64, P, P]),
        "frecsys_rank_positions": (ctypes.c_int, [P, I32, P, I64, I32, P, P, P, P, P, P, P]),
        "frecsys_explain": (ctypes.c_int, [P, I32, P, P, I64, P, P, I32, P, P, P, P]),
        "frecsys_csr_row_lengths": (ctypes.c_int, [P, I32, P, I64, P]),
        "frecsys_mmr_select": (ctypes.c_int,
                               [P, I64, I32, I64, P, P, I64, I32, I32, F, I32, P, P, P]),
        "frecsys_diversify": (ctypes.c_int, [P, P, P, I64, I32, I32, F, I32, P, P, P]),
        "frecsys_recommend_diverse": (ctypes.c_int,
                                      [P, I32, P, I64, I32, I32, F, I32, P, P, P, P]),
        "frecsys_list_quality": (ctypes.c_int, [P, I64, I32, I64, P, I64, I32, P, I32, P, P, P, P]),
        "frecsys_exposure_summary": (ctypes.c_int, [P, I64, P, P, P, P, P]),
        "frecsys_rank_quality": (ctypes.c_int, [P, I32, P, I64, I32, P, P, I32, I32, F, I32, P, P,
                                                P, P, P, P, P, P]),
        "frecsys_lists_quality": (ctypes.c_int, [P, P, I64, I32, P, I32, P, P, P, P]),
        "frecsys_dpp_select": (ctypes.c_int,
                               [P, I64, I32, I64, P, P, I64, I32, I32, F, F, I32, P, P, P]),
        "frecsys_diversify_dpp": (ctypes.c_int, [P, P, P, I64, I32, I32, F, F, I32, P, P, P]),
        "frecsys_recommend_dpp": (ctypes.c_int,
                                  [P, I32, P, I64, I32, I32, F, F, I32, P, P, P, P]),
        "frecsys_recommend_two_stage": (ctypes.c_int,
                                        [P, I32, P, I64, I32, I32, I32, P, P, P, P, P, P]),
        "frecsys_bf16_round": (ctypes.c_int, [P, I64, P]),
        "frecsys_two_stage_bound": (ctypes.c_double, [I32, ctypes.c_double, ctypes.c_double]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def load_model_library(path: str = MODEL_LIB_PATH) -> ctypes.CDLL:
    """Load libfrecsys_model.so (the C++ model classes behind a C-ABI)."""
    global _model_lib
    if _model_lib is not None:
        return _model_lib
    load_library()
    if not os.path.exists(path):
        raise FrecsysError(ERR_INVALID, f"{path} missing: run __graft_entry__.build() / make")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    P, I32, I64, F = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    sig = {
        "frecsys_model_config_default": (None, [P]),
        "frecsys_model_create": (ctypes.c_int, [P, P, P, I64, P]),
        "frecsys_model_initialize": (ctypes.c_int, [P]),
        "frecsys_model_train": (ctypes.c_int, [P, I32]),
        "frecsys_model_context": (P, [P]),
        "frecsys_model_mean_weight": (ctypes.c_float, [P]),
        "frecsys_model_destroy": (None, [P]),
        "frecsys_model_last_error": (ctypes.c_char_p, []),
        "frecsys_model_dual_state": (ctypes.c_int, [P, P, P, P, P]),
        "frecsys_model_recommend": (ctypes.c_int, [P, P, I64, I32, I32, P, P, P]),
        "frecsys_model_recommend_fold_in": (ctypes.c_int, [P, P, P, I64, I32, I32, P, P, P]),
        "frecsys_model_evaluate": (ctypes.c_int,
                                   [P, P, I64, P, P, P, I32, P, I32, I32, P, P, P]),
        "frecsys_model_evaluate_fold_in": (ctypes.c_int,
                                           [P, P, P, I64, P, P, P, I32, P, I32, I32, P, P, P]),
        "frecsys_model_score": (ctypes.c_int, [P, P, P, I64, P]),
        "frecsys_model_rank_candidates": (ctypes.c_int, [P, P, I64, P, P, I32, I32, P, P, P]),
        "frecsys_model_similar_items": (ctypes.c_int, [P, P, I64, I32, I32, P, P, P]),
        "frecsys_model_similar_users": (ctypes.c_int, [P, P, I64, I32, I32, P, P, P]),
        "frecsys_model_audience": (ctypes.c_int, [P, P, I64, I32, I32, P, P, P]),
        "frecsys_model_rank_candidates_fold_in": (ctypes.c_int,
                                                  [P, P, P, I64, P, P, I32, I32, P, P, P]),
        "frecsys_model_evaluate_candidates": (
            ctypes.c_int, [P, P, I64, P, P, P, P, P, I32, P, I32, I32, P, P, P, P]),
        "frecsys_model_evaluate_candidates_fold_in": (
            ctypes.c_int, [P, P, P, I64, P, P, P, P, P, I32, P, I32, I32, P, P, P, P]),
        "frecsys_model_evaluate_sampled": (
            ctypes.c_int,
            [P, P, I64, P, P, I32, ctypes.c_uint64, P, I32, P, I32, I32, P, P, P, P]),
        "frecsys_model_evaluate_sampled_fold_in": (
            ctypes.c_int,
            [P, P, P, I64, P, P, I32, ctypes.c_uint64, P, I32, P, I32, I32, P, P, P, P]),
        "frecsys_model_evaluate_ranks": (
            ctypes.c_int, [P, P, I64, P, P, P, I32, I32, P, P, P, P, P, P]),
        "frecsys_model_evaluate_ranks_fold_in": (
            ctypes.c_int, [P, P, P, I64, P, P, P, I32, I32, P, P, P, P, P, P]),
        "frecsys_model_save": (ctypes.c_int, [P, ctypes.c_char_p, I32]),
        "frecsys_model_load": (ctypes.c_int, [ctypes.c_char_p, P, P, P, I64, I32, P]),
        "frecsys_model_file_info": (ctypes.c_int, [ctypes.c_char_p, I32, P]),
        "frecsys_model_epochs": (I64, [P]),
        "frecsys_model_explain": (ctypes.c_int, [P, P, I64, P, P, I32, P, P, P, P]),
        "frecsys_model_explain_fold_in": (ctypes.c_int,
                                          [P, P, P, I64, P, P, I32, P, P, P, P]),
        "frecsys_model_recommend_diverse": (ctypes.c_int,
                                            [P, P, I64, I32, I32, F, I32, I32, P, P, P, P]),
        "frecsys_model_recommend_diverse_fold_in": (
            ctypes.c_int, [P, P, P, I64, I32, I32, F, I32, I32, P, P, P, P]),
        "frecsys_model_diversify": (ctypes.c_int, [P, P, P, I64, I32, I32, F, I32, P, P, P]),
        "frecsys_model_evaluate_quality": (
            ctypes.c_int,
            [P, P, I64, P, I32, I32, F, I32, P, P, P, P, I32, I32, P, P, P, P, P, P, P]),
        "frecsys_model_evaluate_quality_fold_in": (
            ctypes.c_int,
            [P, P, P, I64, P, I32, I32, F, I32, P, P, P, P, I32, I32, P, P, P, P, P, P, P]),
        "frecsys_model_list_quality": (ctypes.c_int,
                                       [P, P, I64, I32, P, I32, P, P, P, P, P, P]),
        "frecsys_model_recommend_dpp": (ctypes.c_int,
                                        [P, P, I64, I32, I32, F, F, I32, I32, P, P, P, P]),
        "frecsys_model_recommend_dpp_fold_in": (
            ctypes.c_int, [P, P, P, I64, I32, I32, F, F, I32, I32, P, P, P, P]),
        "frecsys_model_diversify_dpp": (ctypes.c_int,
                                        [P, P, P, I64, I32, I32, F, F, I32, P, P, P]),
        "frecsys_model_recommend_two_stage": (ctypes.c_int,
                                              [P, P, I64, I32, I32, I32, I32, P, P, P, P]),
        "frecsys_model_recommend_two_stage_fold_in": (
            ctypes.c_int, [P, P, P, I64, I32, I32, I32, I32, P, P, P, P]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _model_lib = lib
    return lib


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _check_host(lib, rc: int, model: bool = False):
    """Raise the error of a call that has no context: the library's message
    (frecsys_last_error(NULL), or frecsys_model_last_error for the model ABI)."""
    if rc:
        msg = lib.frecsys_model_last_error() if model else lib.frecsys_last_error(None)
        raise FrecsysError(rc, msg.decode())


def _explain_full(lengths: np.ndarray, tgt_ptr: np.ndarray):
    """The buffer of explain's `full` and its pair pointer: pair p of row i
    holds lengths[i] contributions."""
    per_pair = np.repeat(lengths, np.diff(tgt_ptr))
    fp = np.concatenate([[0], np.cumsum(per_pair)]).astype(np.int64)
    return np.zeros(int(fp[-1]), dtype=np.float32), fp


def device_count() -> int:
    lib = load_library()
    n = ctypes.c_int32(0)
    lib.frecsys_device_count(ctypes.byref(n))
    return int(n.value)


def padded_dim(dim: int) -> int:
    return int(load_library().frecsys_padded_dim(dim))


def partition(row_ptr: np.ndarray, nparts: int) -> np.ndarray:
    """nnz-balanced contiguous split (host-only; no GPU needed)."""
    lib = load_library()
    rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
    out = np.zeros(nparts + 1, dtype=np.int64)
    rc = lib.frecsys_partition(len(rp) - 1, _ptr(rp), nparts, _ptr(out))
    _check_host(lib, rc)
    return out


def gram_plan(dim: int, n_rows: int, world: int = 1, rank: int = 0):
    """Host-only Gramian plan: (rows_per_leaf, n_leaves, n_groups, own_lo,
    own_hi) -- frecsys_gram_plan."""
    lib = load_library()
    rpl, nl = ctypes.c_int64(), ctypes.c_int64()
    ng, lo, hi = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    rc = lib.frecsys_gram_plan(dim, n_rows, world, rank, ctypes.byref(rpl), ctypes.byref(nl),
                               ctypes.byref(ng), ctypes.byref(lo), ctypes.byref(hi))
    _check_host(lib, rc)
    return int(rpl.value), int(nl.value), int(ng.value), int(lo.value), int(hi.value)


class _AudiencePlan(ctypes.Structure):
    _fields_ = [(f, ctypes.c_int32) for f in
                ("thin", "queries_per_pass", "passes", "splits", "chunk_rows", "slots",
                 "merge_rounds")] + [("rows_per_batch", ctypes.c_int64),
                                     ("workspace_bytes", ctypes.c_int64)]


def audience_plan(dim: int, n_users: int, n: int, k: int, cus: int = 256,
                  exclude: bool = False) -> dict:
    """Host-only: what Context.audience launches for n query items against
    n_users users on a device of `cus` compute units -- the fields of
    frecsys_audience_plan_t as a dict.  Reads FRECSYS_AUDIENCE_THIN_MAX,
    FRECSYS_RECOMMEND_SPLITS and FRECSYS_RECOMMEND_WS_MB as the call does."""
    lib = load_library()
    pl = _AudiencePlan()
    rc = lib.frecsys_audience_plan(dim, n_users, n, k, cus, 1 if exclude else 0, ctypes.byref(pl))
    _check_host(lib, rc)
    return {f: int(getattr(pl, f)) for f, _ in _AudiencePlan._fields_}


def _ground_truth(gt_ptr, gt_items):
    gp = np.ascontiguousarray(gt_ptr, dtype=np.int64).reshape(-1)
    gi = np.ascontiguousarray(gt_items, dtype=np.int32).reshape(-1)
    return gp, gi


def list_metrics(lists, gt_ptr, gt_items, k_list) -> Tuple[np.ndarray, np.ndarray]:
    """(recall, ndcg) float32 [n, len(k_list)] of ranked lists (int32 [n,
    list_k]; -1 = empty slot) against a CSR ground truth: the reference's
    RankMetrics on the host (frecsys_list_metrics; no GPU needed)."""
    lib = load_library()
    ls = np.ascontiguousarray(lists, dtype=np.int32)
    assert ls.ndim == 2, ls.shape
    gp, gi = _ground_truth(gt_ptr, gt_items)
    assert len(gp) == ls.shape[0] + 1, (len(gp), ls.shape)
    ks = np.ascontiguousarray(k_list, dtype=np.int32).reshape(-1)
    rec = np.zeros((ls.shape[0], len(ks)), dtype=np.float32)
    ndcg = np.zeros_like(rec)
    rc = lib.frecsys_list_metrics(_ptr(ls), ls.shape[0], ls.shape[1], _ptr(gp), _ptr(gi),
                                  _ptr(ks), len(ks), _ptr(rec), _ptr(ndcg))
    _check_host(lib, rc)
    return rec, ndcg


def _quality_args(lists, k_list, item_weight, n_items, exposure):
    """The arrays of a quality call: lists int32 [n, list_k] (or None), the
    cut-offs, the weights, and the outputs ild, novelty (None without
    weights), exposure (None unless asked for)."""
    ls = None
    if lists is not None:
        ls = np.ascontiguousarray(lists, dtype=np.int32)
        assert ls.ndim == 2, ls.shape
    ks = np.ascontiguousarray(k_list, dtype=np.int32).reshape(-1)
    wt = None
    if item_weight is not None:
        wt = np.ascontiguousarray(item_weight, dtype=np.float32).reshape(-1)
        assert wt.shape == (n_items,), (wt.shape, n_items)
    return ls, ks, wt, (np.zeros((len(ks), n_items), dtype=np.int64) if exposure else None)


def _quality_out(n: int, nk: int, wt):
    ild = np.zeros((n, nk), dtype=np.float32)
    return ild, (np.zeros_like(ild) if wt is not None else None)


def list_quality(item_table, lists, k_list, item_weight=None, exposure: bool = True):
    """(ild float32 [n, nk], novelty float32 [n, nk] or None, exposure int64
    [nk, n_items] or None) of ranked lists (int32 [n, list_k]; negative = empty
    slot) against item_table float32 [n_items, dim] on the host
    (frecsys_list_quality: the definition Context.rank_quality and
    Context.lists_quality compute on the GPU; no GPU needed).  ILD@K = 1 - the
    mean pairwise cosine of the filled slots below K; novelty@K = their mean
    item_weight (None: no novelty); exposure[q, i] = how often item i is listed
    below k_list[q]."""
    lib = load_library()
    tab = np.asarray(item_table, dtype=np.float32)
    assert tab.ndim == 2, tab.shape
    if tab.strides[1] != 4 or tab.strides[0] % 4 or tab.strides[0] < 4 * tab.shape[1]:
        tab = np.ascontiguousarray(tab)
    ls, ks, wt, ex = _quality_args(lists, k_list, item_weight, tab.shape[0], exposure)
    ild, nov = _quality_out(ls.shape[0], len(ks), wt)
    rc = lib.frecsys_list_quality(_ptr(tab), tab.shape[0], tab.shape[1], tab.strides[0] // 4,
                                  _ptr(ls), ls.shape[0], ls.shape[1], _ptr(ks), len(ks), _ptr(wt),
                                  _ptr(ild), _ptr(nov), _ptr(ex))
    _check_host(lib, rc)
    return ild, nov, ex


def exposure_summary(exposure, item_mask=None) -> dict:
    """{"coverage", "gini", "total", "covered"} of one exposure row (int64
    [n_items]) among the items of item_mask (None: all) -- on the host
    (frecsys_exposure_summary): the share of items listed at least once and
    the Gini coefficient of the counts, its numerator summed exactly."""
    lib = load_library()
    ex = np.ascontiguousarray(exposure, dtype=np.int64).reshape(-1)
    mk = None
    if item_mask is not None:
        mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
        assert mk.shape == ex.shape, (mk.shape, ex.shape)
    cov, gini = ctypes.c_double(0.0), ctypes.c_double(0.0)
    total, covered = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = lib.frecsys_exposure_summary(_ptr(ex), len(ex), _ptr(mk), ctypes.byref(cov),
                                      ctypes.byref(gini), ctypes.byref(total),
                                      ctypes.byref(covered))
    _check_host(lib, rc)
    return {"coverage": cov.value, "gini": gini.value, "total": int(total.value),
            "covered": int(covered.value)}


def default_pool(k: int) -> int:
    """The pool the diversified calls draw k items from when none is given."""
    return min(1024, max(k, 4 * k))


def bf16_round(values) -> np.ndarray:
    """float32 array of the same shape: every value rounded to bf16 by
    round-to-nearest-even and widened back, a NaN staying a NaN -- on the host
    (frecsys_bf16_round: the rounding of recommend_two_stage's stage 1, bit for
    bit; no GPU needed)."""
    lib = load_library()
    v = np.ascontiguousarray(values, dtype=np.float32)
    out = np.empty_like(v)
    _check_host(lib, lib.frecsys_bf16_round(_ptr(v), v.size, _ptr(out)))
    return out


def two_stage_bound(dim: int, query_norm: float, item_norm_max: float) -> float:
    """B = c(Dp) * query_norm * item_norm_max of recommend_two_stage's
    certificate, in double on the host (frecsys_two_stage_bound)."""
    return float(load_library().frecsys_two_stage_bound(dim, query_norm, item_norm_max))


def default_two_stage_pool(k: int) -> int:
    """The pool recommend_two_stage retrieves when none is given."""
    return min(1024, max(64, 4 * k))


def _pools(lists, scores):
    ls = np.ascontiguousarray(lists, dtype=np.int32)
    sc = np.ascontiguousarray(scores, dtype=np.float32)
    assert ls.ndim == 2 and ls.shape == sc.shape, (ls.shape, sc.shape)
    return ls, sc


def _diverse_out(n: int, k: int, return_mmr: bool):
    items = np.full((n, max(k, 0)), -1, dtype=np.int32)
    scores = np.zeros(items.shape, dtype=np.float32)
    return items, scores, (np.zeros(items.shape, dtype=np.float32) if return_mmr else None)


def mmr_select(item_table, lists, scores, k: int, lam: float = 0.7, raw_scores: bool = False,
               return_mmr: bool = False):
    """(items int32 [n, k], scores float32 [n, k][, mmr float32 [n, k]]): greedy
    maximal-marginal-relevance selection of k slots from each row's pool
    (lists int32 [n, pool], negative = empty slot; scores float32 [n, pool])
    against item_table float32 [n_items, dim], on the host
    (frecsys_mmr_select: the definition Context.diversify and
    Context.recommend_diverse return bit for bit; no GPU needed)."""
    lib = load_library()
    tab = np.asarray(item_table, dtype=np.float32)
    assert tab.ndim == 2, tab.shape
    if tab.strides[1] != 4 or tab.strides[0] % 4 or tab.strides[0] < 4 * tab.shape[1]:
        tab = np.ascontiguousarray(tab)
    ls, sc = _pools(lists, scores)
    items, out, mmr = _diverse_out(ls.shape[0], k, return_mmr)
    rc = lib.frecsys_mmr_select(_ptr(tab), tab.shape[0], tab.shape[1], tab.strides[0] // 4,
                                _ptr(ls), _ptr(sc), ls.shape[0], ls.shape[1], k, lam,
                                DIV_RAW_SCORES if raw_scores else 0, _ptr(items), _ptr(out),
                                _ptr(mmr))
    _check_host(lib, rc)
    return (items, out, mmr) if return_mmr else (items, out)


def dpp_select(item_table, lists, scores, k: int, theta: float = 4.0, eps: float = 1e-3,
               raw_scores: bool = False, return_gain: bool = False):
    """(items int32 [n, k], scores float32 [n, k][, gain float32 [n, k]]): greedy
    DPP selection (the incremental Cholesky of Chen, Zhang and Zhou) of k slots
    from each row's pool against item_table, on the host (frecsys_dpp_select:
    the definition Context.diversify_dpp and Context.recommend_dpp return bit
    for bit; no GPU needed).  Arrays as for mmr_select; theta scales the
    relevance in the quality 2^(theta rel) (0: pure diversity), and a slot
    whose residual is below eps is taken only in pool order, with gain 0."""
    lib = load_library()
    tab = np.asarray(item_table, dtype=np.float32)
    assert tab.ndim == 2, tab.shape
    if tab.strides[1] != 4 or tab.strides[0] % 4 or tab.strides[0] < 4 * tab.shape[1]:
        tab = np.ascontiguousarray(tab)
    ls, sc = _pools(lists, scores)
    items, out, gain = _diverse_out(ls.shape[0], k, return_gain)
    rc = lib.frecsys_dpp_select(_ptr(tab), tab.shape[0], tab.shape[1], tab.strides[0] // 4,
                                _ptr(ls), _ptr(sc), ls.shape[0], ls.shape[1], k, theta, eps,
                                DIV_RAW_SCORES if raw_scores else 0, _ptr(items), _ptr(out),
                                _ptr(gain))
    _check_host(lib, rc)
    return (items, out, gain) if return_gain else (items, out)


def sample_negatives(n_items: int, gt_ptr, gt_items, n_neg: int, seed: int = 0, rows=None,
                     hist_ptr=None, hist_items=None,
                     item_mask=None) -> Tuple[np.ndarray, np.ndarray]:
    """(neg_count int32 [n], negatives int32 [n, n_neg]): the negatives of
    sampled evaluation on the host (frecsys_sample_negatives; no GPU needed),
    bit for bit what Context.sampled_metrics draws on the device.  Query row i
    has side row id rows[i] (i when rows is None), the ground truth row i of
    gt_ptr / gt_items and, if given, the history row i of hist_ptr /
    hist_items (ids it must not draw).  A whole-pool row (more than half of
    its pool asked for, or a pool below 1/64 of the maskable items) takes its
    whole pool: neg_count = the pool size and its negatives row holds -1."""
    lib = load_library()
    gp, gi = _ground_truth(gt_ptr, gt_items)
    n = len(gp) - 1
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
    assert r is None or len(r) == n, (len(r), n)
    hp = None if hist_ptr is None else np.ascontiguousarray(hist_ptr, dtype=np.int64).reshape(-1)
    hi = None if hist_items is None else np.ascontiguousarray(hist_items,
                                                             dtype=np.int32).reshape(-1)
    assert hp is None or len(hp) == n + 1, (len(hp), n)
    mk = None
    if item_mask is not None:
        mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
        assert mk.shape == (n_items,), mk.shape
    cnt = np.zeros(n, dtype=np.int32)
    neg = np.full((n, max(n_neg, 0)), -1, dtype=np.int32)
    rc = lib.frecsys_sample_negatives(n_items, _ptr(mk), _ptr(r), n, _ptr(hp), _ptr(hi), _ptr(gp),
                                      _ptr(gi), n_neg, seed & 0xFFFFFFFFFFFFFFFF, _ptr(cnt),
                                      _ptr(neg))
    _check_host(lib, rc)
    return cnt, neg


def position_metrics(rank, gt_ptr, eligible) -> Tuple[np.ndarray, np.ndarray]:
    """(mrr, auc) float32 [n] of full-catalogue positions (rank int32
    [gt_ptr[n]], 0-based, -1 = not eligible; eligible int32 [n]: the eligible
    items per row) -- frecsys_position_metrics on the host, no GPU needed; what
    Context.rank_positions computes on the device, bit for bit."""
    lib = load_library()
    rk = np.ascontiguousarray(rank, dtype=np.int32).reshape(-1)
    gp = np.ascontiguousarray(gt_ptr, dtype=np.int64).reshape(-1)
    el = np.ascontiguousarray(eligible, dtype=np.int32).reshape(-1)
    n = len(gp) - 1
    assert len(el) == n, (len(el), n)
    assert n < 1 or len(rk) == gp[-1], (len(rk), gp[-1])
    mrr = np.zeros(n, dtype=np.float32)
    auc = np.zeros(n, dtype=np.float32)
    rc = lib.frecsys_position_metrics(_ptr(rk), _ptr(gp), _ptr(el), n, _ptr(mrr), _ptr(auc))
    _check_host(lib, rc)
    return mrr, auc


def metric_cvar(values, alphas) -> np.ndarray:
    """float32 [len(alphas)]: the reference's lower-tail CVaR of per-user
    metric values (EvaluationResult::cvar verbatim, quirks included --
    frecsys_metric_cvar; no GPU needed)."""
    lib = load_library()
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    a = np.ascontiguousarray(alphas, dtype=np.float32).reshape(-1)
    out = np.zeros(len(a), dtype=np.float32)
    rc = lib.frecsys_metric_cvar(_ptr(v), len(v), _ptr(a), len(a), _ptr(out))
    _check_host(lib, rc)
    return out


# the stored fields of frecsys_model_config (CONFIG of a checkpoint)
_STORED_FLAGS = tuple(n for n, _ in _ModelConfig._fields_
                      if n not in ("model_name", "device", "world", "rank", "comm_id"))


def model_file_info(path: str, verify: bool = True) -> dict:
    """What the checkpoint at `path` holds (frecsys_model_file_info; host only,
    no device): model_name, n_users, n_items, n_tuples, epochs_trained, flags,
    has_data, tuples_checksum, version and `config`, a dict of the stored
    model flags.  verify=False checks the header, the directory and CONFIG;
    verify=True every section's checksum too."""
    lib = load_model_library()
    info = _ModelFileInfo()
    rc = lib.frecsys_model_file_info(os.fsencode(path), int(bool(verify)), ctypes.byref(info))
    _check_host(lib, rc, model=True)
    return {"model_name": info.model_name.decode(), "n_users": info.n_users,
            "n_items": info.n_items, "n_tuples": info.n_tuples,
            "epochs_trained": info.epochs_trained, "flags": info.flags,
            "has_data": bool(info.flags & 1), "tuples_checksum": info.tuples_checksum,
            "version": info.version,
            "config": {n: getattr(info.config, n) for n in _STORED_FLAGS}}


def unique_id() -> bytes:
    lib = load_library()
    buf = (ctypes.c_uint8 * 128)()
    rc = lib.frecsys_comm_unique_id(buf)
    _check_host(lib, rc)
    return bytes(buf)


class Context:
    """One device context (one GPU).  See include/frecsys_hip.h."""

    def __init__(self, dim: int, n_users: int, n_items: int, device: int = -1,
                 parity_quirks: bool = True, _borrowed=None):
        self.lib = load_library()
        self.owned = _borrowed is None
        if _borrowed is not None:  # a model's context (frecsys_model_context)
            self.h = ctypes.c_void_p(_borrowed)
            self.dim = dim
            self.n = {SIDE_USER: n_users, SIDE_ITEM: n_items, SIDE_EVAL: 0}
            return
        cfg = _Config(dim, device, 1 if parity_quirks else 0, 0, n_users, n_items)
        h = ctypes.c_void_p()
        rc = self.lib.frecsys_ctx_create(ctypes.byref(cfg), ctypes.byref(h))
        _check_host(self.lib, rc)
        self.h = h
        self.dim = dim
        self.n = {SIDE_USER: n_users, SIDE_ITEM: n_items, SIDE_EVAL: 0}

    # -- helpers --
    def _check(self, rc: int):
        if rc:
            ent = int(self.lib.frecsys_last_error_entity(self.h))
            raise FrecsysError(rc, self.lib.frecsys_last_error(self.h).decode(), ent)

    def close(self):
        if getattr(self, "h", None):
            if self.owned:
                self.lib.frecsys_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- comm --
    def comm_init(self, world: int, rank: int, uid: Optional[bytes]):
        """uid None: external exchange (no RCCL; the caller moves partial
        Gramians and shard rows between ranks)."""
        buf = None if uid is None else (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        self._check(self.lib.frecsys_comm_init(self.h, world, rank, buf))

    def comm_world(self) -> Tuple[int, int, int]:
        """(world, rank, ranks of the RCCL communicator -- 0 without one)."""
        w, r, n = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self.lib.frecsys_comm_world(self.h, ctypes.byref(w), ctypes.byref(r),
                                                ctypes.byref(n)))
        return int(w.value), int(r.value), int(n.value)

    def gram_groups(self, side: int) -> Tuple[int, int, int, int]:
        """(n_groups, own_lo, own_hi, floats_per_group) of side's Gramian plan."""
        ng, lo, hi, fl = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        self._check(self.lib.frecsys_gram_groups(self.h, side, ctypes.byref(ng), ctypes.byref(lo),
                                                 ctypes.byref(hi), ctypes.byref(fl)))
        return int(ng.value), int(lo.value), int(hi.value), int(fl.value)

    def get_gram_groups(self, side: int) -> np.ndarray:
        ng, _, _, fl = self.gram_groups(side)
        out = np.zeros((ng, fl), dtype=np.float32)
        self._check(self.lib.frecsys_get_gram_groups(self.h, side, _ptr(out)))
        return out

    def set_gram_groups(self, side: int, slabs: np.ndarray):
        ng, _, _, fl = self.gram_groups(side)
        a = np.ascontiguousarray(slabs, dtype=np.float32)
        assert a.shape == (ng, fl), (a.shape, ng, fl)
        self._check(self.lib.frecsys_set_gram_groups(self.h, side, _ptr(a)))

    def shard_range(self, side: int) -> Tuple[int, int]:
        lo, hi = ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.frecsys_shard_range(self.h, side, ctypes.byref(lo), ctypes.byref(hi)))
        return int(lo.value), int(hi.value)

    # -- data --
    def load_csr(self, side: int, row_ptr: np.ndarray, col: np.ndarray):
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        cl = np.ascontiguousarray(col, dtype=np.int32)
        self._check(self.lib.frecsys_load_csr(self.h, side, len(rp) - 1, _ptr(rp), _ptr(cl)))
        if side == SIDE_EVAL:
            self.n[SIDE_EVAL] = len(rp) - 1

    def set_embeddings(self, side: int, emb: np.ndarray):
        e = np.ascontiguousarray(emb, dtype=np.float32)
        assert e.shape == (self.n[side], self.dim), (e.shape, self.n[side], self.dim)
        self._check(self.lib.frecsys_set_embeddings(self.h, side, _ptr(e), self.dim))

    def get_embeddings(self, side: int) -> np.ndarray:
        out = np.empty((self.n[side], self.dim), dtype=np.float32)
        self._check(self.lib.frecsys_get_embeddings(self.h, side, _ptr(out), self.dim))
        return out

    def init_embeddings(self, seed: int, stdev: float):
        self._check(self.lib.frecsys_init_embeddings(self.h, seed, stdev))

    def snapshot(self, side: int):
        self._check(self.lib.frecsys_snapshot(self.h, side))

    def snapshot_residual(self, side: int) -> float:
        """sum over rows of ||X_r - snapshot_r||^2 (double, on the device)."""
        sq = ctypes.c_double()
        self._check(self.lib.frecsys_snapshot_residual(self.h, side, ctypes.byref(sq)))
        return float(sq.value)

    def counter(self, what: str) -> int:
        """Cumulative event counter: "hspace_reruns", "tagged_timeouts" or
        "ws_shrinks"; "recommend_splits": the item splits of the last
        recommend call; "live_device_bytes": the device memory the buffers
        of every context of the process hold now."""
        v = ctypes.c_int64()
        self._check(self.lib.frecsys_counter(self.h, what.encode(), ctypes.byref(v)))
        return int(v.value)

    def release_workspaces(self) -> None:
        """Free the wide-dim workspaces (resized at the next solve) and the
        ranking workspaces of recommend / similar (resized at the next call)."""
        self._check(self.lib.frecsys_release_workspaces(self.h))

    # -- compute --
    def gramian(self, side: int, weights: Optional[np.ndarray] = None,
                from_snapshot: bool = False, fetch: bool = True) -> Optional[np.ndarray]:
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
        out = np.empty((self.dim, self.dim), dtype=np.float32) if fetch else None
        self._check(self.lib.frecsys_gramian(self.h, side, _ptr(w), 1 if from_snapshot else 0,
                                             _ptr(out)))
        return out

    def get_gramian(self, side: int) -> np.ndarray:
        """G[side] as the context holds it (no recomputation)."""
        out = np.empty((self.dim, self.dim), dtype=np.float32)
        self._check(self.lib.frecsys_get_gramian(self.h, side, _ptr(out), self.dim))
        return out

    def set_gramian(self, side: int, G: np.ndarray):
        g = np.ascontiguousarray(G, dtype=np.float32)
        assert g.shape == (self.dim, self.dim), g.shape
        self._check(self.lib.frecsys_set_gramian(self.h, side, _ptr(g), self.dim))

    def solve_side(self, side: int, kind: int, reg: float, unobserved_weight: float,
                   reg_exp: float = 1.0, alpha: float = 0.0, stepsize: float = 0.0,
                   from_snapshot: bool = False, entity_weight=None, entity_reg=None,
                   other_weight=None):
        ew = None if entity_weight is None else np.ascontiguousarray(entity_weight, np.float32)
        er = None if entity_reg is None else np.ascontiguousarray(entity_reg, np.float32)
        ow = None if other_weight is None else np.ascontiguousarray(other_weight, np.float32)
        p = _SolveParams(kind, reg, reg_exp, unobserved_weight, alpha, stepsize,
                         1 if from_snapshot else 0, 0,
                         None if ew is None else ew.ctypes.data,
                         None if er is None else er.ctypes.data,
                         None if ow is None else ow.ctypes.data)
        self._check(self.lib.frecsys_solve_side(self.h, side, ctypes.byref(p)))

    def solve_side_cg(self, side: int, kind: int, reg: float, unobserved_weight: float,
                      max_iterations: int = 100, tolerance: float = 1e-10,
                      reg_exp: float = 1.0, alpha: float = 0.0, from_snapshot: bool = False,
                      lambda_is_reg: bool = False, entity_weight=None, entity_reg=None,
                      other_weight=None):
        """solve_side by Jacobi-preconditioned conjugate gradients from a zero
        start (frecsys_solve_side_cg): stops at ||r||^2 < tolerance^2 ||b||^2
        or after max_iterations."""
        ew = None if entity_weight is None else np.ascontiguousarray(entity_weight, np.float32)
        er = None if entity_reg is None else np.ascontiguousarray(entity_reg, np.float32)
        ow = None if other_weight is None else np.ascontiguousarray(other_weight, np.float32)
        p = _SolveParams(kind, reg, reg_exp, unobserved_weight, alpha, 0.0,
                         1 if from_snapshot else 0, 1 if lambda_is_reg else 0,
                         None if ew is None else ew.ctypes.data,
                         None if er is None else er.ctypes.data,
                         None if ow is None else ow.ctypes.data)
        cg = _CgParams(max_iterations, tolerance)
        self._check(self.lib.frecsys_solve_side_cg(self.h, side, ctypes.byref(p),
                                                   ctypes.byref(cg)))

    def cg_iterations(self, side: int) -> np.ndarray:
        """int32 [rows of side]: the iteration count of the last solve_side_cg
        per row; -1 for a row not solved here."""
        out = np.full(max(self.n[side], 1), -1, dtype=np.int32)
        self._check(self.lib.frecsys_cg_iterations(self.h, side, _ptr(out)))
        return out[:self.n[side]]

    def user_loss(self, side: int, beta: float, half: bool, fetch: bool = True):
        out = np.zeros(self.n[side], dtype=np.float32) if fetch else None
        self._check(self.lib.frecsys_user_loss(self.h, side, beta, 1 if half else 0, _ptr(out)))
        return out

    def synchronize(self):
        self._check(self.lib.frecsys_synchronize(self.h))

    def timing(self, what: str) -> Tuple[float, int]:
        ms, n = ctypes.c_double(), ctypes.c_int64()
        self._check(self.lib.frecsys_timing(self.h, what.encode(), ctypes.byref(ms),
                                            ctypes.byref(n)))
        return float(ms.value), int(n.value)

    def work(self, what: str):
        """(flops, bytes, entities, launches) of timer key `what`: the
        algorithmic work the library launched (frecsys_work)."""
        f, b = ctypes.c_double(), ctypes.c_double()
        e, n = ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.frecsys_work(self.h, what.encode(), ctypes.byref(f), ctypes.byref(b),
                                          ctypes.byref(e), ctypes.byref(n)))
        return float(f.value), float(b.value), int(e.value), int(n.value)

    def history_space_max_h(self, side=None) -> int:
        if side is None:
            return int(self.lib.frecsys_history_space_max_h(self.h))
        return int(self.lib.frecsys_history_space_max_h_side(self.h, side))

    def timing_reset(self):
        self._check(self.lib.frecsys_timing_reset(self.h))

    def eval_topk(self, k: int):
        """[EVAL rows, k] int32: best k items per fold-in row, history excluded,
        score descending, ties by item id."""
        out = np.zeros((self.n[SIDE_EVAL], k), dtype=np.int32)
        self._check(self.lib.frecsys_eval_topk(self.h, k, _ptr(out)))
        return out

    def recommend(self, side: int, k: int, rows=None, exclude_history: bool = True,
                  item_mask=None) -> Tuple[np.ndarray, np.ndarray]:
        """(items int32 [n, k], scores float32 [n, k]): the k best eligible
        items of each query row of `side` (SIDE_USER or SIDE_EVAL) by score
        descending, item id ascending -- frecsys_recommend, fused scoring +
        top-K on the GPU.  rows: row ids (any order, repeats allowed; None =
        every row of the side); exclude_history drops the row's CSR history;
        item_mask [n_items]: non-zero = candidate.  Slots beyond the eligible
        count hold item -1 and score -FLT_MAX."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = self.n[side] if r is None else len(r)
        mk = None
        if item_mask is not None:
            mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n[SIDE_ITEM],), mk.shape
        items = np.full((n, k) if k > 0 else (n, 0), -1, dtype=np.int32)
        scores = np.zeros(items.shape, dtype=np.float32)
        self._check(self.lib.frecsys_recommend(self.h, side, _ptr(r), n, k,
                                               REC_EXCLUDE_HISTORY if exclude_history else 0,
                                               _ptr(mk), _ptr(items), _ptr(scores)))
        return items, scores

    def recommend_two_stage(self, side: int, k: int, pool: Optional[int] = None, rows=None,
                            exclude_history: bool = True, item_mask=None, exact: bool = True,
                            return_pool: bool = False):
        """(items int32 [n, k], scores float32 [n, k], certified uint8 [n][,
        pool_items int32 [n, pool], pool_scores float32 [n, pool]]):
        retrieve-then-rank (frecsys_recommend_two_stage).  A bf16 scan on the
        matrix cores picks each row's `pool` best eligible items (default
        default_two_stage_pool(k)), the pool is re-scored by recommend's exact
        chain, and certified[r] = 1 where an error bound proves the list to be
        recommend(side, k, ...)'s bit for bit.  exact re-runs the rows that are
        not certified through recommend's scan (certified[r] = 2), so every row
        carries recommend's bits; without it such a row holds the k best of
        its pool.  rows, exclude_history, item_mask as for recommend."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = self.n[side] if r is None else len(r)
        mk = None
        if item_mask is not None:
            mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n[SIDE_ITEM],), mk.shape
        p = default_two_stage_pool(k) if pool is None else pool
        items = np.full((n, k) if k > 0 else (n, 0), -1, dtype=np.int32)
        scores = np.zeros(items.shape, dtype=np.float32)
        cert = np.zeros(n, dtype=np.uint8)
        pi = np.full((n, max(p, 0)), -1, dtype=np.int32) if return_pool else None
        ps = np.zeros(pi.shape, dtype=np.float32) if return_pool else None
        flags = (REC_EXCLUDE_HISTORY if exclude_history else 0) | (TS_EXACT if exact else 0)
        self._check(self.lib.frecsys_recommend_two_stage(
            self.h, side, _ptr(r), n, k, p, flags, _ptr(mk), _ptr(items), _ptr(scores),
            _ptr(cert), _ptr(pi), _ptr(ps)))
        return (items, scores, cert, pi, ps) if return_pool else (items, scores, cert)

    def recommend_diverse(self, side: int, k: int, pool: Optional[int] = None, lam: float = 0.7,
                          rows=None, raw_scores: bool = False, exclude_history: bool = True,
                          item_mask=None, return_mmr: bool = False):
        """(items int32 [n, k], scores float32 [n, k][, mmr float32 [n, k]]):
        mmr_select of recommend(side, pool, ...)'s lists against the item
        table, bit for bit, with the pools never leaving the GPU
        (frecsys_recommend_diverse).  pool defaults to default_pool(k); lam = 1
        returns recommend(side, k, ...)."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = self.n[side] if r is None else len(r)
        mk = None
        if item_mask is not None:
            mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n[SIDE_ITEM],), mk.shape
        items, scores, mmr = _diverse_out(n, k, return_mmr)
        flags = (REC_EXCLUDE_HISTORY if exclude_history else 0) | \
            (DIV_RAW_SCORES if raw_scores else 0)
        self._check(self.lib.frecsys_recommend_diverse(
            self.h, side, _ptr(r), n, k, default_pool(k) if pool is None else pool, lam, flags,
            _ptr(mk), _ptr(items), _ptr(scores), _ptr(mmr)))
        return (items, scores, mmr) if return_mmr else (items, scores)

    def diversify(self, lists, scores, k: int, lam: float = 0.7, raw_scores: bool = False,
                  return_mmr: bool = False):
        """The same selection from caller-supplied pools (lists int32 [n,
        pool], negative = empty slot; scores float32 [n, pool]) against the
        context's item table, on the GPU (frecsys_diversify): mmr_select's
        result bit for bit."""
        ls, sc = _pools(lists, scores)
        items, out, mmr = _diverse_out(ls.shape[0], k, return_mmr)
        self._check(self.lib.frecsys_diversify(self.h, _ptr(ls), _ptr(sc), ls.shape[0],
                                               ls.shape[1], k, lam,
                                               DIV_RAW_SCORES if raw_scores else 0, _ptr(items),
                                               _ptr(out), _ptr(mmr)))
        return (items, out, mmr) if return_mmr else (items, out)

    def recommend_dpp(self, side: int, k: int, pool: Optional[int] = None, theta: float = 4.0,
                      eps: float = 1e-3, rows=None, raw_scores: bool = False,
                      exclude_history: bool = True, item_mask=None, return_gain: bool = False):
        """(items int32 [n, k], scores float32 [n, k][, gain float32 [n, k]]):
        dpp_select of recommend(side, pool, ...)'s lists against the item
        table, bit for bit, with the pools never leaving the GPU
        (frecsys_recommend_dpp).  pool defaults to default_pool(k)."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = self.n[side] if r is None else len(r)
        mk = None
        if item_mask is not None:
            mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n[SIDE_ITEM],), mk.shape
        items, scores, gain = _diverse_out(n, k, return_gain)
        flags = (REC_EXCLUDE_HISTORY if exclude_history else 0) | \
            (DIV_RAW_SCORES if raw_scores else 0)
        self._check(self.lib.frecsys_recommend_dpp(
            self.h, side, _ptr(r), n, k, default_pool(k) if pool is None else pool, theta, eps,
            flags, _ptr(mk), _ptr(items), _ptr(scores), _ptr(gain)))
        return (items, scores, gain) if return_gain else (items, scores)

    def diversify_dpp(self, lists, scores, k: int, theta: float = 4.0, eps: float = 1e-3,
                      raw_scores: bool = False, return_gain: bool = False):
        """The same selection from caller-supplied pools against the context's
        item table, on the GPU (frecsys_diversify_dpp): dpp_select's result bit
        for bit."""
        ls, sc = _pools(lists, scores)
        items, out, gain = _diverse_out(ls.shape[0], k, return_gain)
        self._check(self.lib.frecsys_diversify_dpp(self.h, _ptr(ls), _ptr(sc), ls.shape[0],
                                                   ls.shape[1], k, theta, eps,
                                                   DIV_RAW_SCORES if raw_scores else 0,
                                                   _ptr(items), _ptr(out), _ptr(gain)))
        return (items, out, gain) if return_gain else (items, out)

    def rank_quality(self, side: int, k_list, rows=None, pool: Optional[int] = None,
                     lam: float = 0.7, raw_scores: bool = False, item_weight=None, gt=None,
                     exclude_history: bool = True, item_mask=None, ild: bool = True,
                     exposure: bool = True) -> dict:
        """List quality of a serving configuration, computed on the GPU without
        the lists leaving it (frecsys_rank_quality): a dict of "ild" float32
        [n, nk], "novelty" float32 [n, nk] (item_weight [n_items] given),
        "exposure" int64 [nk, n_items], "recall" / "ndcg" float32 [n, nk] (gt =
        (gt_ptr, gt_items) given) -- None for what was not asked for.  The lists
        are recommend(side, max(k_list), ...)'s (pool None) or
        recommend_diverse(side, max(k_list), pool, lam, ...)'s; the values are
        list_quality's and list_metrics' of those lists (ILD and novelty to the
        last fp32 bit or the one beside it, the rest exactly)."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = self.n[side] if r is None else len(r)
        mk = None
        if item_mask is not None:
            mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n[SIDE_ITEM],), mk.shape
        _, ks, wt, ex = _quality_args(None, k_list, item_weight, self.n[SIDE_ITEM], exposure)
        out_ild, nov = _quality_out(n, len(ks), wt)
        if not ild:
            out_ild = None
        gp = gi = rec = ndcg = None
        if gt is not None:
            gp, gi = _ground_truth(*gt)
            assert len(gp) == n + 1, (len(gp), n)
            rec = np.zeros((n, len(ks)), dtype=np.float32)
            ndcg = np.zeros_like(rec)
        self._check(self.lib.frecsys_rank_quality(
            self.h, side, _ptr(r), n, REC_EXCLUDE_HISTORY if exclude_history else 0, _ptr(mk),
            _ptr(ks), len(ks), 0 if pool is None else pool, lam,
            DIV_RAW_SCORES if raw_scores else 0, _ptr(wt), _ptr(gp), _ptr(gi), _ptr(out_ild),
            _ptr(nov), _ptr(rec), _ptr(ndcg), _ptr(ex)))
        return {"ild": out_ild, "novelty": nov, "exposure": ex, "recall": rec, "ndcg": ndcg,
                "k_list": ks}

    def lists_quality(self, lists, k_list, item_weight=None, ild: bool = True,
                      exposure: bool = True) -> dict:
        """The same measures of caller-supplied lists (int32 [n, list_k];
        negative = empty slot) against the context's item table, on the GPU
        (frecsys_lists_quality): a dict of "ild", "novelty" and "exposure"."""
        ls, ks, wt, ex = _quality_args(lists, k_list, item_weight, self.n[SIDE_ITEM], exposure)
        out_ild, nov = _quality_out(ls.shape[0], len(ks), wt)
        if not ild:
            out_ild = None
        self._check(self.lib.frecsys_lists_quality(self.h, _ptr(ls), ls.shape[0], ls.shape[1],
                                                   _ptr(ks), len(ks), _ptr(wt), _ptr(out_ild),
                                                   _ptr(nov), _ptr(ex)))
        return {"ild": out_ild, "novelty": nov, "exposure": ex, "k_list": ks}

    def rank_metrics(self, side: int, k_list, gt_ptr, gt_items, rows=None,
                     exclude_history: bool = True,
                     item_mask=None) -> Tuple[np.ndarray, np.ndarray]:
        """(recall, ndcg) float32 [n, len(k_list)]: list_metrics of
        recommend(side, max(k_list), ...)'s ranking, bitwise, computed on the
        GPU without the lists leaving it (frecsys_rank_metrics).  Ground-truth
        row i (CSR gt_ptr / gt_items; not empty) belongs to query row i."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = self.n[side] if r is None else len(r)
        mk = None
        if item_mask is not None:
            mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n[SIDE_ITEM],), mk.shape
        gp, gi = _ground_truth(gt_ptr, gt_items)
        assert len(gp) == n + 1, (len(gp), n)
        ks = np.ascontiguousarray(k_list, dtype=np.int32).reshape(-1)
        rec = np.zeros((n, len(ks)), dtype=np.float32)
        ndcg = np.zeros_like(rec)
        self._check(self.lib.frecsys_rank_metrics(self.h, side, _ptr(r), n,
                                                  REC_EXCLUDE_HISTORY if exclude_history else 0,
                                                  _ptr(mk), _ptr(gp), _ptr(gi), _ptr(ks), len(ks),
                                                  _ptr(rec), _ptr(ndcg)))
        return rec, ndcg

    def rank_positions(self, side: int, gt_ptr, gt_items, rows=None,
                       exclude_history: bool = True, item_mask=None, metrics: bool = True):
        """(rank int32 [gt_ptr[n]], eligible int32 [n], mrr float32 [n], auc
        float32 [n]) -- without the last two when metrics is False: the exact
        0-based position of every ground-truth entry among the eligible items
        of its query row (the slot recommend would list it in if its k were
        large enough; -1: the item is masked out or in the excluded history),
        the eligible count, and position_metrics of those ranks computed on
        the GPU -- frecsys_rank_positions, a fused score-and-count scan.  rows,
        exclude_history and item_mask as for recommend; ground-truth row i (CSR
        gt_ptr / gt_items; not empty) belongs to query row i."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = self.n[side] if r is None else len(r)
        mk = None
        if item_mask is not None:
            mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n[SIDE_ITEM],), mk.shape
        gp, gi = _ground_truth(gt_ptr, gt_items)
        assert len(gp) == n + 1, (len(gp), n)
        rank = np.full(len(gi), -1, dtype=np.int32)
        elig = np.zeros(n, dtype=np.int32)
        mrr = np.zeros(n, dtype=np.float32) if metrics else None
        auc = np.zeros(n, dtype=np.float32) if metrics else None
        self._check(self.lib.frecsys_rank_positions(self.h, side, _ptr(r), n,
                                                    REC_EXCLUDE_HISTORY if exclude_history else 0,
                                                    _ptr(mk), _ptr(gp), _ptr(gi), _ptr(rank),
                                                    _ptr(elig), _ptr(mrr), _ptr(auc)))
        return (rank, elig, mrr, auc) if metrics else (rank, elig)

    def score_pairs(self, side: int, rows, items) -> np.ndarray:
        """float32 [n]: the score of item items[i] for row rows[i] of `side`
        (SIDE_USER or SIDE_EVAL) -- frecsys_score_pairs; bit for bit the score
        recommend lists for that row and item."""
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        it = np.ascontiguousarray(items, dtype=np.int32).reshape(-1)
        assert r.shape == it.shape, (r.shape, it.shape)
        out = np.zeros(len(r), dtype=np.float32)
        self._check(self.lib.frecsys_score_pairs(self.h, side, _ptr(r), _ptr(it), len(r),
                                                 _ptr(out)))
        return out

    def csr_row_lengths(self, side: int, rows=None, n: Optional[int] = None) -> np.ndarray:
        """int64 [n]: the history length of CSR row rows[i] of `side` (row i
        without rows) as loaded -- frecsys_csr_row_lengths."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = len(r) if r is not None else int(n)
        out = np.zeros(n, dtype=np.int64)
        self._check(self.lib.frecsys_csr_row_lengths(self.h, side, _ptr(r), n, _ptr(out)))
        return out

    def explain(self, side: int, kind: int, reg: float, unobserved_weight: float, tgt_ptr,
                tgt_items, rows=None, top: int = 10, full: bool = False, reg_exp: float = 1.0,
                lambda_is_reg: bool = False, entity_weight=None):
        """(score float32 [pairs], top_items int32 [pairs, top], top_contrib
        float32 [pairs, top][, full float32, full_ptr int64 [pairs + 1]]): the
        score of every (query row, target) pair split exactly over the row's
        history entries -- frecsys_explain.  Query row i is CSR row rows[i] of
        `side` (SIDE_USER or SIDE_EVAL; row i without rows) with the targets
        tgt_items[tgt_ptr[i]:tgt_ptr[i + 1]]; kind (KIND_IALS / KIND_WEIGHTED_U)
        and the parameters are solve_side's.  score is the score of the exact
        projection of the history against the current item table and G[ITEM];
        the lists hold the `top` largest contributions (ties by CSR position)
        with their history item ids, -1 / 0 behind the history length; with
        full, pair p's contributions in CSR order are
        full[full_ptr[p]:full_ptr[p + 1]] and sum to score[p]."""
        tp = np.ascontiguousarray(tgt_ptr, dtype=np.int64).reshape(-1)
        ti = np.ascontiguousarray(tgt_items, dtype=np.int32).reshape(-1)
        n = len(tp) - 1
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        assert r is None or len(r) == n, (len(r), n)
        ew = None if entity_weight is None else np.ascontiguousarray(entity_weight, np.float32)
        p = _SolveParams(kind, reg, reg_exp, unobserved_weight, 0.0, 0.0, 0,
                         1 if lambda_is_reg else 0, None if ew is None else ew.ctypes.data,
                         None, None)
        pairs = int(tp[-1]) if n >= 0 and len(tp) else 0
        score = np.zeros(max(pairs, 0), dtype=np.float32)
        items = np.full((max(pairs, 0), max(top, 0)), -1, dtype=np.int32)
        contrib = np.zeros(items.shape, dtype=np.float32)
        fl = fp = None
        if full:
            fl, fp = _explain_full(self.csr_row_lengths(side, r, n), tp)
        self._check(self.lib.frecsys_explain(self.h, side, ctypes.byref(p), _ptr(r), n, _ptr(tp),
                                             _ptr(ti), top, _ptr(score), _ptr(items),
                                             _ptr(contrib), _ptr(fl)))
        return (score, items, contrib, fl, fp) if full else (score, items, contrib)

    def rank_candidates(self, side: int, k: int, cand_ptr, cand_items, rows=None,
                        exclude_history: bool = True,
                        item_mask=None) -> Tuple[np.ndarray, np.ndarray]:
        """(items int32 [n, k], scores float32 [n, k]): the k best distinct
        eligible ids of each query row's own candidate list (CSR cand_ptr
        int64 [n + 1] / cand_items int32; list i belongs to query row i) by
        score descending, item id ascending -- frecsys_rank_candidates.  rows,
        exclude_history, item_mask and the -1 / -FLT_MAX fill as in
        recommend; the scores are recommend's bit for bit."""
        cp = np.ascontiguousarray(cand_ptr, dtype=np.int64).reshape(-1)
        ci = np.ascontiguousarray(cand_items, dtype=np.int32).reshape(-1)
        n = len(cp) - 1
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        assert r is None or len(r) == n, (len(r), n)
        mk = None
        if item_mask is not None:
            mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n[SIDE_ITEM],), mk.shape
        items = np.full((n, k) if k > 0 else (n, 0), -1, dtype=np.int32)
        scores = np.zeros(items.shape, dtype=np.float32)
        self._check(self.lib.frecsys_rank_candidates(
            self.h, side, _ptr(r), n, _ptr(cp), _ptr(ci), k,
            REC_EXCLUDE_HISTORY if exclude_history else 0, _ptr(mk), _ptr(items), _ptr(scores)))
        return items, scores

    def rank_candidates_metrics(self, side: int, k_list, cand_ptr, cand_items, gt_ptr, gt_items,
                                rows=None, exclude_history: bool = True,
                                item_mask=None) -> Tuple[np.ndarray, np.ndarray]:
        """(recall, ndcg) float32 [n, len(k_list)]: list_metrics of
        rank_candidates(side, max(k_list), cand_ptr, cand_items, ...)'s lists,
        bitwise, without the lists leaving the GPU
        (frecsys_rank_candidates_metrics).  Candidate list i and ground-truth
        row i belong to query row i; a ground-truth id outside the list, masked
        or in the excluded history is never a hit."""
        cp = np.ascontiguousarray(cand_ptr, dtype=np.int64).reshape(-1)
        ci = np.ascontiguousarray(cand_items, dtype=np.int32).reshape(-1)
        n = len(cp) - 1
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        assert r is None or len(r) == n, (len(r), n)
        mk = None
        if item_mask is not None:
            mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n[SIDE_ITEM],), mk.shape
        gp, gi = _ground_truth(gt_ptr, gt_items)
        assert len(gp) == n + 1, (len(gp), n)
        ks = np.ascontiguousarray(k_list, dtype=np.int32).reshape(-1)
        rec = np.zeros((n, len(ks)), dtype=np.float32)
        ndcg = np.zeros_like(rec)
        self._check(self.lib.frecsys_rank_candidates_metrics(
            self.h, side, _ptr(r), n, _ptr(cp), _ptr(ci),
            REC_EXCLUDE_HISTORY if exclude_history else 0, _ptr(mk), _ptr(gp), _ptr(gi), _ptr(ks),
            len(ks), _ptr(rec), _ptr(ndcg)))
        return rec, ndcg

    def sampled_metrics(self, side: int, k_list, gt_ptr, gt_items, n_neg: int, seed: int = 0,
                        rows=None, exclude_history: bool = True, item_mask=None,
                        return_negatives: bool = False):
        """(recall, ndcg) float32 [n, len(k_list)] of sampled evaluation
        (frecsys_sampled_metrics): each query row ranks its distinct ground
        truth against n_neg negatives drawn on the GPU from the eligible items
        outside its ground truth (and, with exclude_history, its history) by
        the generator of sample_negatives -- or against its whole pool where
        that is small.  With return_negatives also (neg_count int32 [n],
        negatives int32 [n, n_neg]) as sample_negatives returns them.  Sampled
        metrics are not estimates of rank_metrics' full-catalogue values."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = self.n[side] if r is None else len(r)
        mk = None
        if item_mask is not None:
            mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n[SIDE_ITEM],), mk.shape
        gp, gi = _ground_truth(gt_ptr, gt_items)
        assert len(gp) == n + 1, (len(gp), n)
        ks = np.ascontiguousarray(k_list, dtype=np.int32).reshape(-1)
        rec = np.zeros((n, len(ks)), dtype=np.float32)
        ndcg = np.zeros_like(rec)
        cnt = neg = None
        if return_negatives:
            cnt = np.zeros(n, dtype=np.int32)
            neg = np.full((n, max(n_neg, 0)), -1, dtype=np.int32)
        self._check(self.lib.frecsys_sampled_metrics(
            self.h, side, _ptr(r), n, REC_EXCLUDE_HISTORY if exclude_history else 0, _ptr(mk),
            _ptr(gp), _ptr(gi), n_neg, seed & 0xFFFFFFFFFFFFFFFF, _ptr(ks), len(ks), _ptr(rec),
            _ptr(ndcg), _ptr(cnt), _ptr(neg)))
        if return_negatives:
            return rec, ndcg, cnt, neg
        return rec, ndcg

    def similar(self, side: int, k: int, rows=None, cosine: bool = True, keep_self: bool = False,
                mask=None) -> Tuple[np.ndarray, np.ndarray]:
        """(ids int32 [n, k], scores float32 [n, k]): the k nearest rows of
        the table of `side` (SIDE_USER or SIDE_ITEM) for each query row of the
        same table, by score descending, id ascending -- frecsys_similar.  The
        score is the cosine (cosine=True) or recommend's dot product; without
        keep_self a query never lists its own id.  rows: row ids (any order,
        repeats allowed; None = every row of the side); mask [rows of side]:
        non-zero = candidate.  Slots beyond the eligible count hold id -1 and
        score -FLT_MAX."""
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = self.n[side] if r is None else len(r)
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n[side],), mk.shape
        ids = np.full((n, k) if k > 0 else (n, 0), -1, dtype=np.int32)
        scores = np.zeros(ids.shape, dtype=np.float32)
        flags = (SIM_COSINE if cosine else 0) | (SIM_KEEP_SELF if keep_self else 0)
        self._check(self.lib.frecsys_similar(self.h, side, _ptr(r), n, k, flags, _ptr(mk),
                                             _ptr(ids), _ptr(scores)))
        return ids, scores

    def audience(self, k: int, items=None, exclude_history: bool = True,
                 mask=None) -> Tuple[np.ndarray, np.ndarray]:
        """(users int32 [n, k], scores float32 [n, k]): the k best users for
        each query item (a row of the ITEM table), by score descending, user
        id ascending -- frecsys_audience.  The score is recommend's for that
        (user, item) pair, bit for bit.  items: item ids (any order, repeats
        allowed; None = every item); exclude_history drops the users in the
        item's row of the ITEM-side CSR; mask [users]: non-zero = candidate.
        Slots beyond the eligible count hold id -1 and score -FLT_MAX."""
        r = None if items is None else np.ascontiguousarray(items, dtype=np.int64).reshape(-1)
        n = self.n[SIDE_ITEM] if r is None else len(r)
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n[SIDE_USER],), mk.shape
        users = np.full((n, k) if k > 0 else (n, 0), -1, dtype=np.int32)
        scores = np.zeros(users.shape, dtype=np.float32)
        flags = AUD_EXCLUDE_HISTORY if exclude_history else 0
        self._check(self.lib.frecsys_audience(self.h, _ptr(r), n, k, flags, _ptr(mk),
                                              _ptr(users), _ptr(scores)))
        return users, scores

    def pp_set_rating_index(self, side: int, rix: np.ndarray):
        r = np.ascontiguousarray(rix, dtype=np.int32)
        self._check(self.lib.frecsys_pp_set_rating_index(self.h, side, _ptr(r)))

    def pp_sync(self, side: int):
        """External-exchange completion of a sharded pp_step (frecsys_pp_sync)."""
        self._check(self.lib.frecsys_pp_sync(self.h, side))

    def pp_predict(self, side: int):
        self._check(self.lib.frecsys_pp_predict(self.h, side))

    def pp_predictions(self, side: int, nnz: int) -> np.ndarray:
        """The prediction vector (frecsys_pp_get_predictions), nnz floats."""
        out = np.empty(max(nnz, 1), np.float32)
        self._check(self.lib.frecsys_pp_get_predictions(self.h, side, _ptr(out)))
        return out[:nnz]

    def set_transport(self, allgather_rows, allreduce_min_u64):
        """Exchange callbacks of external-exchange mode (frecsys_set_transport):
        allgather_rows(side, rows, lo, hi) fills every rank's rows of the
        (n_rows, ld) float32 array in place (rows [lo, hi) are this rank's);
        allreduce_min_u64(value) -> the minimum over ranks.  None clears."""
        if allgather_rows is None:
            self._transport = None
            self._check(self.lib.frecsys_set_transport(self.h, None))
            return

        def rows_cb(user, side, ptr, n, ld, lo, hi):
            try:
                arr = np.ctypeslib.as_array(ptr, shape=(max(n, 1) * ld,))[:n * ld].reshape(n, ld)
                allgather_rows(int(side), arr, int(lo), int(hi))
                return 0
            except Exception:  # noqa: BLE001 -- reported to the library as a failed exchange
                import traceback
                traceback.print_exc()
                return 1

        def min_cb(user, vp):
            try:
                vp[0] = int(allreduce_min_u64(int(vp[0])))
                return 0
            except Exception:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                return 1

        t = _Transport(None, _ROWS_FN(rows_cb), _MIN_FN(min_cb))
        self._transport = t  # the callbacks live as long as the context uses them
        self._check(self.lib.frecsys_set_transport(self.h, ctypes.byref(t)))

    def pp_step(self, side: int, start: int, end: int, reg: float, w: float,
                reg_exp: float = 1.0, kind: int = 0, alpha: float = 0.0, entity_weight=None,
                entity_reg=None, other_weight=None) -> float:
        ew = None if entity_weight is None else np.ascontiguousarray(entity_weight, np.float32)
        er = None if entity_reg is None else np.ascontiguousarray(entity_reg, np.float32)
        ow = None if other_weight is None else np.ascontiguousarray(other_weight, np.float32)
        p = _SolveParams(kind, reg, reg_exp, w, alpha, 0.0, 0, 0,
                         None if ew is None else ew.ctypes.data,
                         None if er is None else er.ctypes.data,
                         None if ow is None else ow.ctypes.data)
        res = ctypes.c_double(0.0)
        self._check(self.lib.frecsys_pp_step(self.h, side, start, end, ctypes.byref(p),
                                             ctypes.byref(res)))
        return res.value

    def train_stats(self):
        """(observed, unobserved, ||U_r||^2, ||V_r||^2): ComputeLosses' parts."""
        obs = ctypes.c_double(0.0)
        unobs = ctypes.c_double(0.0)
        un = np.zeros(self.n[SIDE_USER], dtype=np.float32)
        vn = np.zeros(self.n[SIDE_ITEM], dtype=np.float32)
        self._check(self.lib.frecsys_train_stats(self.h, ctypes.byref(obs), ctypes.byref(unobs),
                                                 _ptr(un), _ptr(vn)))
        return obs.value, unobs.value, un, vn

    def debug_diag_factor(self, tiles: np.ndarray, blocked: bool):
        """L^-1 of each 32x32 SPD tile (diagnostic): (linv [n,32,32], ok [n])."""
        a = np.ascontiguousarray(tiles, dtype=np.float32).reshape(-1, 32, 32)
        out = np.zeros_like(a)
        ok = np.zeros(len(a), dtype=np.int32)
        self._check(self.lib.frecsys_debug_diag_factor(self.h, 1 if blocked else 0, len(a),
                                                       _ptr(a), _ptr(out), _ptr(ok)))
        return out, ok

    def debug_basis(self, side: int):
        """(Q, diag, sub) with G[side] = Q T Q^T (diagnostic, Dp >= 64)."""
        Dp = padded_dim(self.dim)
        q = np.zeros((Dp, Dp), dtype=np.float32)
        dg = np.zeros(Dp, dtype=np.float32)
        sb = np.zeros(Dp, dtype=np.float32)
        self._check(self.lib.frecsys_debug_basis(self.h, side, _ptr(q), _ptr(dg), _ptr(sb)))
        return q, dg, sb


class Model:
    """One model of include/frecsys_model.h: the run_model factory over the
    C++ classes.  `users`, `items`: the training tuples in file order;
    keyword arguments are the run_model flags (frecsys_model_config)."""

    def __init__(self, model_name: str, users: np.ndarray, items: np.ndarray, **flags):
        self.lib = load_model_library()
        cfg = _ModelConfig()
        self.lib.frecsys_model_config_default(ctypes.byref(cfg))
        self._name = model_name.encode()
        cfg.model_name = self._name
        self._cid = None
        self._apply_flags(cfg, flags)
        u = np.ascontiguousarray(users, dtype=np.int32)
        it = np.ascontiguousarray(items, dtype=np.int32)
        assert u.shape == it.shape
        h = ctypes.c_void_p()
        self._check(self.lib.frecsys_model_create(ctypes.byref(cfg), _ptr(u), _ptr(it), len(u),
                                                  ctypes.byref(h)))
        self.h = h
        self.dim = cfg.dim
        self.n_users = int(u.max()) + 1
        self.n_items = int(it.max()) + 1

    def _check(self, rc: int):
        _check_host(self.lib, rc, model=True)

    def _apply_flags(self, cfg, flags):
        for k, v in flags.items():
            if k == "comm_id":
                if v is not None:
                    self._cid = (ctypes.c_uint8 * 128).from_buffer_copy(v)
                    cfg.comm_id = ctypes.cast(self._cid, ctypes.c_void_p)
                continue
            if not hasattr(cfg, k):
                raise TypeError(f"unknown model flag {k}")
            setattr(cfg, k, int(v) if isinstance(v, bool) else v)

    def save(self, path: str, include_data: bool = True):
        """Write the model to `path` (frecsys_model_save): tables, dual state,
        everything an exact resume needs and, with include_data, the training
        tuples.  Atomic: an existing file is replaced only by a complete one."""
        self._check(self.lib.frecsys_model_save(self.h, os.fsencode(path),
                                                0 if include_data else SAVE_NO_DATA))

    @classmethod
    def load(cls, path: str, users=None, items=None, tables_only: bool = False, **flags):
        """A model from a checkpoint (frecsys_model_load).  Without tuples: the
        file's own (resume), or none when it holds none (serve-only: no train,
        no exclude_seen).  With the saved run's tuples: resume, checked against
        the file's checksum.  tables_only: a new model of the caller's tuples
        (which may span more users / items) whose U and V start from the
        file's.  `flags` are Model(...)'s, applied on top of the stored ones;
        model_name and dim cannot change."""
        self = cls.__new__(cls)
        self.lib = load_model_library()
        info = _ModelFileInfo()
        self._check(self.lib.frecsys_model_file_info(os.fsencode(path), 0, ctypes.byref(info)))
        cfg = _ModelConfig()
        ctypes.pointer(cfg)[0] = info.config
        self._name = bytes(info.model_name.decode(), "ascii")
        cfg.model_name = self._name
        self._cid = None
        name = flags.pop("model_name", None)
        if name is not None:
            self._name = name.encode()
            cfg.model_name = self._name
        self._apply_flags(cfg, flags)
        if (users is None) != (items is None):
            raise TypeError("users and items go together")
        u = it = None
        if users is not None:
            u = np.ascontiguousarray(users, dtype=np.int32)
            it = np.ascontiguousarray(items, dtype=np.int32)
            assert u.shape == it.shape
        h = ctypes.c_void_p()
        self._check(self.lib.frecsys_model_load(
            os.fsencode(path), ctypes.byref(cfg), _ptr(u), _ptr(it), 0 if u is None else len(u),
            LOAD_TABLES_ONLY if tables_only else 0, ctypes.byref(h)))
        self.h = h
        self.dim = cfg.dim
        self.n_users, self.n_items = info.n_users, info.n_items
        if tables_only:
            self.n_users, self.n_items = int(u.max()) + 1, int(it.max()) + 1
        return self

    @property
    def epochs(self) -> int:
        """Train() calls so far, those before a resumed model's save included."""
        return int(self.lib.frecsys_model_epochs(self.h))

    def initialize(self):
        self._check(self.lib.frecsys_model_initialize(self.h))

    def train(self, epochs: int = 1):
        self._check(self.lib.frecsys_model_train(self.h, epochs))

    def context(self) -> Context:
        """The model's device context (borrowed: closing it is a no-op)."""
        ctx = Context(self.dim, self.n_users, self.n_items,
                      _borrowed=self.lib.frecsys_model_context(self.h))
        ctx._owner = self  # the native context lives as long as the model
        return ctx

    def dual_state(self):
        """(omega [n_users], user losses [n_users], item_reg [n_items], xi) of
        ERM-MF / CVaR-MF / SAFER2 (frecsys_model_dual_state)."""
        w = np.zeros(self.n_users, dtype=np.float32)
        l = np.zeros(self.n_users, dtype=np.float32)
        r = np.zeros(self.n_items, dtype=np.float32)
        xi = ctypes.c_float(0.0)
        self._check(self.lib.frecsys_model_dual_state(self.h, _ptr(w), _ptr(l), _ptr(r),
                                                      ctypes.byref(xi)))
        return w, l, r, float(xi.value)

    def mean_weight(self) -> float:
        return float(self.lib.frecsys_model_mean_weight(self.h))

    def _mask(self, item_mask):
        if item_mask is None:
            return None
        mk = np.ascontiguousarray(np.asarray(item_mask) != 0, dtype=np.uint8)
        assert mk.shape == (self.n_items,), mk.shape
        return mk

    # Every query comes for trained users and, as <name>_fold_in, for unseen
    # users given by their histories.  The public pairs share one private body
    # each, which takes the query rows as `head`, the leading arrays of the
    # C call, and their count n.

    @staticmethod
    def _head(users=None, hist=None):
        """(head, n) of trained `users`, or of hist = (hist_ptr, hist_items)."""
        if hist is None:
            u = np.ascontiguousarray(users, dtype=np.int64).reshape(-1)
            return [u], len(u)
        hp = np.ascontiguousarray(hist[0], dtype=np.int64).reshape(-1)
        hi = np.ascontiguousarray(hist[1], dtype=np.int32).reshape(-1)
        return [hp, hi], len(hp) - 1

    def _call(self, name: str, head, n: int, *tail):
        """frecsys_model_<name>, or its _fold_in form for a history head."""
        fn = getattr(self.lib, "frecsys_model_" + name + ("_fold_in" if len(head) == 2 else ""))
        self._check(fn(self.h, *[_ptr(x) for x in head], n, *tail))

    def _recommend(self, head, n, k, exclude_seen, item_mask):
        mk = self._mask(item_mask)
        items = np.full((n, max(k, 0)), -1, dtype=np.int32)
        scores = np.zeros(items.shape, dtype=np.float32)
        self._call("recommend", head, n, k, int(bool(exclude_seen)), _ptr(mk), _ptr(items),
                   _ptr(scores))
        return items, scores

    def recommend(self, users, k: int, exclude_seen: bool = True, item_mask=None):
        """(items int32 [n, k], scores float32 [n, k]) for trained users
        (frecsys_model_recommend): best k items by score, ties by item id;
        exclude_seen drops the training history; item -1 / score -FLT_MAX
        beyond the eligible count."""
        return self._recommend(*self._head(users), k, exclude_seen, item_mask)

    def recommend_fold_in(self, hist_ptr, hist_items, k: int, exclude_seen: bool = True,
                          item_mask=None):
        """The same for unseen users given by their histories (CSR: hist_ptr
        int64 [n + 1], hist_items int32): the model's fold-in projection, then
        the ranking (frecsys_model_recommend_fold_in).  The projected rows stay
        in the EVAL side of the model's context."""
        return self._recommend(*self._head(hist=(hist_ptr, hist_items)), k, exclude_seen,
                               item_mask)

    def _recommend_two_stage(self, head, n, k, pool, exact, exclude_seen, item_mask):
        mk = self._mask(item_mask)
        items = np.full((n, max(k, 0)), -1, dtype=np.int32)
        scores = np.zeros(items.shape, dtype=np.float32)
        cert = np.zeros(n, dtype=np.uint8)
        self._call("recommend_two_stage", head, n, k, 0 if pool is None else pool,
                   int(bool(exact)), int(bool(exclude_seen)), _ptr(mk), _ptr(items), _ptr(scores),
                   _ptr(cert))
        return items, scores, cert

    def recommend_two_stage(self, users, k: int, pool: Optional[int] = None, exact: bool = True,
                            exclude_seen: bool = True, item_mask=None):
        """(items int32 [n, k], scores float32 [n, k], certified uint8 [n]) for
        trained users (frecsys_model_recommend_two_stage): recommend(users, k)
        by a bf16 retrieval scan and an exact re-scoring of each row's pool
        (Context.recommend_two_stage).  certified: 1 = proven equal to
        recommend's list, 2 = re-run exactly (exact), 0 = neither."""
        return self._recommend_two_stage(*self._head(users), k, pool, exact, exclude_seen,
                                         item_mask)

    def recommend_two_stage_fold_in(self, hist_ptr, hist_items, k: int,
                                    pool: Optional[int] = None, exact: bool = True,
                                    exclude_seen: bool = True, item_mask=None):
        """The same for unseen users given by their histories, as
        recommend_fold_in (frecsys_model_recommend_two_stage_fold_in)."""
        return self._recommend_two_stage(*self._head(hist=(hist_ptr, hist_items)), k, pool, exact,
                                         exclude_seen, item_mask)

    def _recommend_diverse(self, head, n, k, pool, lam, raw_scores, exclude_history, item_mask,
                           return_mmr):
        mk = self._mask(item_mask)
        items, scores, mmr = _diverse_out(n, k, return_mmr)
        self._call("recommend_diverse", head, n, k, default_pool(k) if pool is None else pool,
                   lam, int(bool(raw_scores)), int(bool(exclude_history)), _ptr(mk), _ptr(items),
                   _ptr(scores), _ptr(mmr))
        return (items, scores, mmr) if return_mmr else (items, scores)

    def recommend_diverse(self, users, k: int, pool: Optional[int] = None, lam: float = 0.7,
                          raw_scores: bool = False, exclude_history: bool = True, item_mask=None,
                          return_mmr: bool = False):
        """(items int32 [n, k], scores float32 [n, k][, mmr float32 [n, k]]) for
        trained users (frecsys_model_recommend_diverse): greedy MMR re-ranking
        of recommend(users, pool)'s lists down to k against the item table --
        mmr_select's result bit for bit, computed on the GPU.  pool defaults to
        min(1024, max(k, 4 k)); lam = 1 returns recommend(users, k)."""
        return self._recommend_diverse(*self._head(users), k, pool, lam, raw_scores,
                                       exclude_history, item_mask, return_mmr)

    def recommend_diverse_fold_in(self, hist_ptr, hist_items, k: int, pool: Optional[int] = None,
                                  lam: float = 0.7, raw_scores: bool = False,
                                  exclude_history: bool = True, item_mask=None,
                                  return_mmr: bool = False):
        """The same for unseen users given by their histories (CSR), as
        recommend_fold_in (frecsys_model_recommend_diverse_fold_in)."""
        return self._recommend_diverse(*self._head(hist=(hist_ptr, hist_items)), k, pool, lam,
                                       raw_scores, exclude_history, item_mask, return_mmr)

    def diversify(self, lists, scores, k: int, lam: float = 0.7, raw_scores: bool = False,
                  return_mmr: bool = False):
        """The same selection from caller-supplied pools (lists int32 [n,
        pool], negative = empty slot; scores float32 [n, pool]) against the
        model's item table (frecsys_model_diversify)."""
        ls, sc = _pools(lists, scores)
        items, out, mmr = _diverse_out(ls.shape[0], k, return_mmr)
        self._check(self.lib.frecsys_model_diversify(self.h, _ptr(ls), _ptr(sc), ls.shape[0],
                                                     ls.shape[1], k, lam, int(bool(raw_scores)),
                                                     _ptr(items), _ptr(out), _ptr(mmr)))
        return (items, out, mmr) if return_mmr else (items, out)

    def _recommend_dpp(self, head, n, k, pool, theta, eps, raw_scores, exclude_seen, item_mask,
                       return_gain):
        mk = self._mask(item_mask)
        items, scores, gain = _diverse_out(n, k, return_gain)
        self._call("recommend_dpp", head, n, k, default_pool(k) if pool is None else pool, theta,
                   eps, int(bool(raw_scores)), int(bool(exclude_seen)), _ptr(mk), _ptr(items),
                   _ptr(scores), _ptr(gain))
        return (items, scores, gain) if return_gain else (items, scores)

    def recommend_dpp(self, users, k: int, pool: Optional[int] = None, theta: float = 4.0,
                      eps: float = 1e-3, exclude_seen: bool = True, item_mask=None,
                      raw_scores: bool = False, return_gain: bool = False):
        """(items int32 [n, k], scores float32 [n, k][, gain float32 [n, k]]) for
        trained users (frecsys_model_recommend_dpp): greedy DPP re-ranking of
        recommend(users, pool)'s lists down to k against the item table --
        dpp_select's result bit for bit, computed on the GPU.  pool defaults to
        default_pool(k); theta = 0 is pure diversity."""
        return self._recommend_dpp(*self._head(users), k, pool, theta, eps, raw_scores,
                                   exclude_seen, item_mask, return_gain)

    def recommend_dpp_fold_in(self, hist_ptr, hist_items, k: int, pool: Optional[int] = None,
                              theta: float = 4.0, eps: float = 1e-3, exclude_seen: bool = True,
                              item_mask=None, raw_scores: bool = False,
                              return_gain: bool = False):
        """The same for unseen users given by their histories (CSR), as
        recommend_fold_in (frecsys_model_recommend_dpp_fold_in)."""
        return self._recommend_dpp(*self._head(hist=(hist_ptr, hist_items)), k, pool, theta, eps,
                                   raw_scores, exclude_seen, item_mask, return_gain)

    def diversify_dpp(self, lists, scores, k: int, theta: float = 4.0, eps: float = 1e-3,
                      raw_scores: bool = False, return_gain: bool = False):
        """The same selection from caller-supplied pools against the model's
        item table (frecsys_model_diversify_dpp)."""
        ls, sc = _pools(lists, scores)
        items, out, gain = _diverse_out(ls.shape[0], k, return_gain)
        self._check(self.lib.frecsys_model_diversify_dpp(
            self.h, _ptr(ls), _ptr(sc), ls.shape[0], ls.shape[1], k, theta, eps,
            int(bool(raw_scores)), _ptr(items), _ptr(out), _ptr(gain)))
        return (items, out, gain) if return_gain else (items, out)

    def item_self_information(self) -> np.ndarray:
        """float32 [n_items]: -log2(max(h_i, 1) / n_users) with h_i the number
        of training users of item i (the item side's CSR lengths) -- the usual
        item_weight of novelty.  Needs the training data on the device: raises
        on a serve-only model."""
        h = self.context().csr_row_lengths(SIDE_ITEM, n=self.n_items)
        return (-np.log2(np.maximum(h, 1).astype(np.float64) / self.n_users)).astype(np.float32)

    @staticmethod
    def _quality_dict(ks, ild, nov, ex, summary):
        nk = len(ks)
        return {"ild": ild, "novelty": nov, "exposure": ex, "k_list": ks,
                "mean_ild": summary[:nk].copy(),
                "mean_novelty": summary[nk:2 * nk].copy() if nov is not None else None,
                "coverage": summary[2 * nk:3 * nk].copy(), "gini": summary[3 * nk:4 * nk].copy()}

    def _evaluate_quality(self, head, n, k_list, pool, lam, gt, item_weight, exclude_seen,
                          item_mask, alpha_list=EVAL_ALPHA_LIST):
        mk = self._mask(item_mask)
        _, ks, wt, ex = _quality_args(None, k_list, item_weight, self.n_items, True)
        nk = len(ks)
        ild, nov = _quality_out(n, nk, wt)
        al = np.ascontiguousarray(alpha_list, dtype=np.float32).reshape(-1)
        na = len(al)
        gp = gi = rec = ndcg = None
        if gt is not None:
            gp, gi = _ground_truth(*gt)
            assert len(gp) == n + 1, (len(gp), n)
            rec = np.zeros((n, nk), dtype=np.float32)
            ndcg = np.zeros_like(rec)
        summary = np.zeros((6 + 2 * na) * nk, dtype=np.float64)
        self._call("evaluate_quality", head, n, _ptr(ks), nk, 0 if pool is None else pool, lam, 0,
                   _ptr(wt), _ptr(gp), _ptr(gi), _ptr(al), na, int(bool(exclude_seen)), _ptr(mk),
                   _ptr(ild), _ptr(nov), _ptr(rec), _ptr(ndcg), _ptr(ex), _ptr(summary))
        out = self._quality_dict(ks, ild, nov, ex, summary)
        if gt is not None:
            t = summary[4 * nk:].astype(np.float32)
            out.update({"recall": rec, "ndcg": ndcg, "alpha_list": al,
                        "mean_recall": t[:nk].copy(), "mean_ndcg": t[nk:2 * nk].copy(),
                        "recall_cvar": t[2 * nk:(2 + na) * nk].reshape(na, nk).copy(),
                        "ndcg_cvar": t[(2 + na) * nk:].reshape(na, nk).copy()})
        return out

    def evaluate_quality(self, users, k_list, pool: Optional[int] = None, lam: float = 0.7,
                         gt=None, item_weight=None, exclude_seen: bool = True, item_mask=None):
        """What a serving configuration buys, for trained users
        (frecsys_model_evaluate_quality), measured on the GPU: a dict of per-user
        "ild" and "novelty" (item_weight [n_items] given, e.g.
        item_self_information()) float32 [n, nk], "exposure" int64 [nk,
        n_items], and per cut-off "mean_ild", "mean_novelty", "coverage" and
        "gini" (of the exposure among the items of item_mask).  pool None: the
        lists are recommend(users, max(k_list))'s; else
        recommend_diverse(users, max(k_list), pool, lam)'s.  gt = (gt_ptr,
        gt_items) adds evaluate()'s "recall", "ndcg" and summary of the same
        lists."""
        return self._evaluate_quality(*self._head(users), k_list, pool, lam, gt, item_weight,
                                      exclude_seen, item_mask)

    def evaluate_quality_fold_in(self, hist_ptr, hist_items, k_list, pool: Optional[int] = None,
                                 lam: float = 0.7, gt=None, item_weight=None,
                                 exclude_seen: bool = True, item_mask=None):
        """The same for unseen users given by their histories (CSR), as
        recommend_fold_in (frecsys_model_evaluate_quality_fold_in)."""
        return self._evaluate_quality(*self._head(hist=(hist_ptr, hist_items)), k_list, pool, lam,
                                      gt, item_weight, exclude_seen, item_mask)

    def list_quality(self, lists, k_list, item_weight=None, item_mask=None):
        """The same measures of caller-supplied lists (int32 [n, list_k];
        negative = empty slot) against the model's item table
        (frecsys_model_list_quality); item_mask selects the items of "coverage"
        and "gini"."""
        mk = self._mask(item_mask)
        ls, ks, wt, ex = _quality_args(lists, k_list, item_weight, self.n_items, True)
        ild, nov = _quality_out(ls.shape[0], len(ks), wt)
        summary = np.zeros(4 * len(ks), dtype=np.float64)
        self._check(self.lib.frecsys_model_list_quality(
            self.h, _ptr(ls), ls.shape[0], ls.shape[1], _ptr(ks), len(ks), _ptr(wt), _ptr(mk),
            _ptr(ild), _ptr(nov), _ptr(ex), _ptr(summary)))
        return self._quality_dict(ks, ild, nov, ex, summary)

    def _explain(self, head, n, tgt_ptr, tgt_items, top, full):
        tp = np.ascontiguousarray(tgt_ptr, dtype=np.int64).reshape(-1)
        ti = np.ascontiguousarray(tgt_items, dtype=np.int32).reshape(-1)
        assert len(tp) == n + 1, (len(tp), n)
        pairs = int(tp[-1])
        score = np.zeros(pairs, dtype=np.float32)
        items = np.full((pairs, max(top, 0)), -1, dtype=np.int32)
        contrib = np.zeros(items.shape, dtype=np.float32)
        fl = fp = None
        if full and len(head) == 2:  # sized by the histories given
            fl, fp = _explain_full(np.diff(head[0]), tp)
        elif full:  # ... or by the training CSR
            # a call without rows loads the training CSR if Train() has not
            self._call("explain", [None], 0, None, None, top, None, None, None, None)
            fl, fp = _explain_full(self.context().csr_row_lengths(SIDE_USER, head[0]), tp)
        self._call("explain", head, n, _ptr(tp), _ptr(ti), top, _ptr(score), _ptr(items),
                   _ptr(contrib), _ptr(fl))
        return (score, items, contrib, fl, fp) if full else (score, items, contrib)

    def explain(self, users, tgt_ptr, tgt_items, top: int = 10, full: bool = False):
        """(score, top_items, top_contrib[, full, full_ptr]) for trained users
        (frecsys_model_explain; outputs as Context.explain's): why item
        tgt_items[tgt_ptr[i]:tgt_ptr[i + 1]] scores what it does for users[i],
        split exactly over the user's training history.  The model supplies the
        solve parameters of its own fold-in (omega = 1), so `score` is the
        score of the exact projection of that history against the current item
        table -- recommend_fold_in's score for the same history -- not score()'s
        U[user] . V[item].  For ialspp / safer2pp it is the exact minimiser of
        the objective their block steps descend; their own fold-in stops after
        8 block epochs.  Needs the training tuples (not a serve-only model)."""
        return self._explain(*self._head(users), tgt_ptr, tgt_items, top, full)

    def explain_fold_in(self, hist_ptr, hist_items, tgt_ptr, tgt_items, top: int = 10,
                        full: bool = False):
        """The same for unseen users given by their histories (CSR hist_ptr /
        hist_items; target list i belongs to history row i):
        frecsys_model_explain_fold_in.  Bit for bit explain()'s result for a
        user with the same history.  The histories are loaded as the EVAL side
        of the model's context."""
        return self._explain(*self._head(hist=(hist_ptr, hist_items)), tgt_ptr, tgt_items, top,
                             full)

    def score(self, users, items) -> np.ndarray:
        """float32 [n]: the model's score of items[i] for trained user
        users[i] (frecsys_model_score); recommend's scores bit for bit."""
        u = np.ascontiguousarray(users, dtype=np.int64).reshape(-1)
        it = np.ascontiguousarray(items, dtype=np.int32).reshape(-1)
        assert u.shape == it.shape, (u.shape, it.shape)
        out = np.zeros(len(u), dtype=np.float32)
        self._check(self.lib.frecsys_model_score(self.h, _ptr(u), _ptr(it), len(u), _ptr(out)))
        return out

    @staticmethod
    def _candidates(cand_ptr, cand_items, n):
        cp = np.ascontiguousarray(cand_ptr, dtype=np.int64).reshape(-1)
        ci = np.ascontiguousarray(cand_items, dtype=np.int32).reshape(-1)
        assert len(cp) == n + 1, (len(cp), n)
        return cp, ci

    def _rank_candidates(self, head, n, cand_ptr, cand_items, k, exclude_seen, item_mask):
        cp, ci = self._candidates(cand_ptr, cand_items, n)
        mk = self._mask(item_mask)
        items = np.full((n, max(k, 0)), -1, dtype=np.int32)
        scores = np.zeros(items.shape, dtype=np.float32)
        self._call("rank_candidates", head, n, _ptr(cp), _ptr(ci), k, int(bool(exclude_seen)),
                   _ptr(mk), _ptr(items), _ptr(scores))
        return items, scores

    def rank_candidates(self, users, cand_ptr, cand_items, k: int, exclude_seen: bool = True,
                        item_mask=None):
        """(items int32 [n, k], scores float32 [n, k]): the k best distinct
        ids of each trained user's own candidate list (CSR cand_ptr /
        cand_items; list i belongs to users[i]) -- frecsys_model_rank_candidates;
        exclude_seen, item_mask and the fill as in recommend."""
        return self._rank_candidates(*self._head(users), cand_ptr, cand_items, k, exclude_seen,
                                     item_mask)

    def _similar(self, fn, n_side: int, rows, k: int, metric: str, include_self: bool, mask):
        if metric not in ("cosine", "dot"):
            raise ValueError(f"metric must be 'cosine' or 'dot', not {metric!r}")
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
            assert mk.shape == (n_side,), mk.shape
        ids = np.full((len(r), k) if k > 0 else (len(r), 0), -1, dtype=np.int32)
        scores = np.zeros(ids.shape, dtype=np.float32)
        flags = (SIM_COSINE if metric == "cosine" else 0) | (SIM_KEEP_SELF if include_self else 0)
        self._check(fn(self.h, _ptr(r), len(r), k, flags, _ptr(mk), _ptr(ids), _ptr(scores)))
        return ids, scores

    def similar_items(self, items, k: int, metric: str = "cosine", include_self: bool = False,
                      item_mask=None):
        """(ids int32 [n, k], scores float32 [n, k]): the k items nearest to
        each of the trained items `items` (rows of V) by metric "cosine" or
        "dot" (recommend's score), ties by id -- frecsys_model_similar_items.
        Without include_self an item never lists itself; item_mask [n_items]:
        non-zero = candidate; -1 / -FLT_MAX beyond the eligible count."""
        return self._similar(self.lib.frecsys_model_similar_items, self.n_items, items, k, metric,
                             include_self, item_mask)

    def similar_users(self, users, k: int, metric: str = "cosine", include_self: bool = False,
                      user_mask=None):
        """The same among the trained users (rows of U) --
        frecsys_model_similar_users; user_mask [n_users]."""
        return self._similar(self.lib.frecsys_model_similar_users, self.n_users, users, k, metric,
                             include_self, user_mask)

    def audience(self, items, k: int, exclude_seen: bool = True, user_mask=None):
        """(users int32 [n, k], scores float32 [n, k]): the k best users for
        each of the trained items `items` (rows of V), by score descending,
        user id ascending -- frecsys_model_audience.  The scores are score()'s
        bits; exclude_seen drops the users who have the item in the training
        tuples; user_mask [n_users]: non-zero = candidate; -1 / -FLT_MAX
        beyond the eligible count."""
        r = np.ascontiguousarray(items, dtype=np.int64).reshape(-1)
        mk = None
        if user_mask is not None:
            mk = np.ascontiguousarray(np.asarray(user_mask) != 0, dtype=np.uint8)
            assert mk.shape == (self.n_users,), mk.shape
        users = np.full((len(r), k) if k > 0 else (len(r), 0), -1, dtype=np.int32)
        scores = np.zeros(users.shape, dtype=np.float32)
        self._check(self.lib.frecsys_model_audience(self.h, _ptr(r), len(r), k,
                                                    1 if exclude_seen else 0, _ptr(mk),
                                                    _ptr(users), _ptr(scores)))
        return users, scores

    def rank_candidates_fold_in(self, hist_ptr, hist_items, cand_ptr, cand_items, k: int,
                                exclude_seen: bool = True, item_mask=None):
        """The same for unseen users given by their histories (CSR hist_ptr /
        hist_items): the model's fold-in projection, then the ranking of
        candidate list i for history row i
        (frecsys_model_rank_candidates_fold_in).  The projected rows stay in
        the EVAL side of the model's context."""
        return self._rank_candidates(*self._head(hist=(hist_ptr, hist_items)), cand_ptr,
                                     cand_items, k, exclude_seen, item_mask)

    def _eval_metrics(self, name, head, n, cand, gt_ptr, gt_items, sample, k_list, alpha_list,
                      exclude_seen, item_mask=None, masked: bool = True):
        """The Recall / NDCG evaluations frecsys_model_<name>: `cand` is the
        candidate CSR or None, `sample` (n_neg, seed) or None; evaluate itself
        takes no item mask (masked=False)."""
        gp, gi = _ground_truth(gt_ptr, gt_items)
        assert len(gp) == n + 1, (len(gp), n)
        ks = np.ascontiguousarray(k_list, dtype=np.int32).reshape(-1)
        al = np.ascontiguousarray(alpha_list, dtype=np.float32).reshape(-1)
        nk, na = len(ks), len(al)
        mk = self._mask(item_mask)
        rec = np.zeros((n, nk), dtype=np.float32)
        ndcg = np.zeros_like(rec)
        summary = np.zeros((2 + 2 * na) * nk, dtype=np.float32)
        args = []
        if cand is not None:
            args += [_ptr(x) for x in self._candidates(cand[0], cand[1], n)]
        args += [_ptr(gp), _ptr(gi)]
        if sample is not None:
            args += [sample[0], sample[1] & 0xFFFFFFFFFFFFFFFF]
        args += [_ptr(ks), nk, _ptr(al), na, int(bool(exclude_seen))]
        if masked:
            args += [_ptr(mk)]
        self._call(name, head, n, *args, _ptr(rec), _ptr(ndcg), _ptr(summary))
        return {"recall": rec, "ndcg": ndcg, "k_list": ks, "alpha_list": al,
                "mean_recall": summary[:nk].copy(), "mean_ndcg": summary[nk:2 * nk].copy(),
                "recall_cvar": summary[2 * nk:(2 + na) * nk].reshape(na, nk).copy(),
                "ndcg_cvar": summary[(2 + na) * nk:].reshape(na, nk).copy()}

    def evaluate(self, users, gt_ptr, gt_items, k_list=EVAL_K_LIST, alpha_list=EVAL_ALPHA_LIST,
                 exclude_seen: bool = True):
        """Ranking quality of trained users (frecsys_model_evaluate): a dict of
        per-user "recall" and "ndcg" float32 [n, nk] and the summary the
        reference logs -- "mean_recall", "mean_ndcg" [nk], "recall_cvar",
        "ndcg_cvar" [na, nk] (EvaluationResult's means and cvar()).  Row i of
        the CSR ground truth belongs to users[i]; the defaults are run_model's
        (run_model.cc:97-100)."""
        return self._eval_metrics("evaluate", *self._head(users), None, gt_ptr, gt_items, None,
                                  k_list, alpha_list, exclude_seen, masked=False)

    def evaluate_fold_in(self, hist_ptr, hist_items, gt_ptr, gt_items, k_list=EVAL_K_LIST,
                         alpha_list=EVAL_ALPHA_LIST, exclude_seen: bool = True):
        """The same for unseen users given by their histories (CSR hist_ptr /
        hist_items): the model's fold-in projection, then the metrics of the
        projected rows (frecsys_model_evaluate_fold_in) -- the reference's
        EvaluateDataset.  The projected rows stay in the EVAL side."""
        return self._eval_metrics("evaluate", *self._head(hist=(hist_ptr, hist_items)), None,
                                  gt_ptr, gt_items, None, k_list, alpha_list, exclude_seen,
                                  masked=False)

    def _eval_ranks(self, head, n, gt_ptr, gt_items, alpha_list, exclude_seen, item_mask):
        gp, gi = _ground_truth(gt_ptr, gt_items)
        assert len(gp) == n + 1, (len(gp), n)
        al = np.ascontiguousarray(alpha_list, dtype=np.float32).reshape(-1)
        na = len(al)
        mk = self._mask(item_mask)
        rank = np.full(len(gi), -1, dtype=np.int32)
        elig = np.zeros(n, dtype=np.int32)
        mrr = np.zeros(n, dtype=np.float32)
        auc = np.zeros(n, dtype=np.float32)
        summary = np.zeros(2 + 2 * na, dtype=np.float32)
        self._call("evaluate_ranks", head, n, _ptr(gp), _ptr(gi), _ptr(al), na,
                   int(bool(exclude_seen)), _ptr(mk), _ptr(rank), _ptr(elig), _ptr(mrr), _ptr(auc),
                   _ptr(summary))
        return {"rank": rank, "eligible": elig, "mrr": mrr, "auc": auc, "alpha_list": al,
                "mean_mrr": float(summary[0]), "mean_auc": float(summary[1]),
                "mrr_cvar": summary[2:2 + na].copy(), "auc_cvar": summary[2 + na:].copy()}

    def evaluate_ranks(self, users, gt_ptr, gt_items, alpha_list=EVAL_ALPHA_LIST,
                       exclude_seen: bool = True, item_mask=None):
        """Full-catalogue ranking quality of trained users
        (frecsys_model_evaluate_ranks): a dict of "rank" int32 [gt_ptr[n]] (the
        exact 0-based position recommend would list each held-out item at with
        a large enough k; -1 = not eligible), "eligible" int32 [n], per-user
        "mrr" and "auc" float32 [n], and "mean_mrr", "mean_auc", "mrr_cvar",
        "auc_cvar" [na] by evaluate()'s own mean and cvar().  Unlike Recall@K /
        NDCG@K these tell apart users whose held-out items rank below 1024."""
        return self._eval_ranks(*self._head(users), gt_ptr, gt_items, alpha_list, exclude_seen,
                                item_mask)

    def evaluate_ranks_fold_in(self, hist_ptr, hist_items, gt_ptr, gt_items,
                               alpha_list=EVAL_ALPHA_LIST, exclude_seen: bool = True,
                               item_mask=None):
        """The same for unseen users given by their histories (CSR hist_ptr /
        hist_items): the model's fold-in projection, then the positions of the
        projected rows (frecsys_model_evaluate_ranks_fold_in).  The projected
        rows stay in the EVAL side."""
        return self._eval_ranks(*self._head(hist=(hist_ptr, hist_items)), gt_ptr, gt_items,
                                alpha_list, exclude_seen, item_mask)

    def evaluate_candidates(self, users, cand_ptr, cand_items, gt_ptr, gt_items,
                            k_list=EVAL_K_LIST, alpha_list=EVAL_ALPHA_LIST,
                            exclude_seen: bool = True, item_mask=None):
        """evaluate()'s dict for trained users whose rankings are restricted
        to caller-supplied candidate lists (CSR cand_ptr / cand_items; list i
        and ground-truth row i belong to users[i]) --
        frecsys_model_evaluate_candidates: the metrics of rank_candidates'
        lists, computed on the GPU."""
        return self._eval_metrics("evaluate_candidates", *self._head(users),
                                  (cand_ptr, cand_items), gt_ptr, gt_items, None, k_list,
                                  alpha_list, exclude_seen, item_mask)

    def evaluate_candidates_fold_in(self, hist_ptr, hist_items, cand_ptr, cand_items, gt_ptr,
                                    gt_items, k_list=EVAL_K_LIST, alpha_list=EVAL_ALPHA_LIST,
                                    exclude_seen: bool = True, item_mask=None):
        """The same for unseen users given by their histories: the fold-in
        projection, then the metrics of candidate list i for history row i
        (frecsys_model_evaluate_candidates_fold_in).  The projected rows stay
        in the EVAL side."""
        return self._eval_metrics("evaluate_candidates", *self._head(hist=(hist_ptr, hist_items)),
                                  (cand_ptr, cand_items), gt_ptr, gt_items, None, k_list,
                                  alpha_list, exclude_seen, item_mask)

    def evaluate_sampled(self, users, gt_ptr, gt_items, n_neg: int, seed: int = 0,
                         k_list=EVAL_K_LIST, alpha_list=EVAL_ALPHA_LIST,
                         exclude_seen: bool = True, item_mask=None):
        """evaluate()'s dict of sampled evaluation for trained users
        (frecsys_model_evaluate_sampled): each user's ground truth ranked
        against n_neg negatives drawn on the GPU (Context.sampled_metrics,
        sample_negatives).  Affordable per epoch where evaluate() is not --
        and not an estimate of evaluate()'s full-catalogue values."""
        return self._eval_metrics("evaluate_sampled", *self._head(users), None, gt_ptr, gt_items,
                                  (n_neg, seed), k_list, alpha_list, exclude_seen, item_mask)

    def evaluate_sampled_fold_in(self, hist_ptr, hist_items, gt_ptr, gt_items, n_neg: int,
                                 seed: int = 0, k_list=EVAL_K_LIST, alpha_list=EVAL_ALPHA_LIST,
                                 exclude_seen: bool = True, item_mask=None):
        """The same for unseen users given by their histories
        (frecsys_model_evaluate_sampled_fold_in); history row i has side row
        id i in the generator.  The projected rows stay in the EVAL side."""
        return self._eval_metrics("evaluate_sampled", *self._head(hist=(hist_ptr, hist_items)),
                                  None, gt_ptr, gt_items, (n_neg, seed), k_list, alpha_list,
                                  exclude_seen, item_mask)

    def close(self):
        if getattr(self, "h", None):
            self.lib.frecsys_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
