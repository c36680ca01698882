"""ctypes binding of the C ABI in include/gorse_hip.h (libgorse_hip.so).

This is plumbing: every entry point of the header is declared here with its exact
signature, plus thin numpy-friendly wrappers (`MF`, `TopK`, `Sparse`).  There is NO CPU fallback:
if the shared library is missing, or no gfx950 device is visible when a handle is
created, the call raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GORSE_HIP_LIB") or os.path.join(HERE, "lib", "libgorse_hip.so")  # the override serves probe builds

OK, ERR_INVALID, ERR_HIP, ERR_CANCELLED, ERR_NO_DEVICE, ERR_RANGE, ERR_NOMEM = 0, -1, -2, -3, -4, -5, -6
BPR_HOGWILD_ATOMIC, BPR_SEQUENTIAL, BPR_HOGWILD_RACY, BPR_HOGWILD_STORES = 0, 1, 2, 3
DTYPE_F32, DTYPE_BF16 = 0, 1
METRIC_NEG_DOT, METRIC_EUCLIDEAN, METRIC_COSINE, METRIC_EUCLIDEAN_BF16 = 0, 1, 2, 3
PROF_BPR_UPDATE, PROF_BPR_SAMPLE, PROF_ALS_SWEEP, PROF_ALS_GRAM, PROF_BPR_SORT, PROF_COMM = 0, 1, 2, 3, 4, 5
COMM_ID_BYTES = 128
MF_EVAL_MAX_TOPK = 128  # GORSE_MF_EVAL_MAX_TOPK
OPT_SGD, OPT_ADAM = 0, 1
PROF_TOPK_SCORE, PROF_TOPK_RESCORE, PROF_TOPK_SWEEP, PROF_TOPK_SELECT, PROF_TOPK_HIST, PROF_TOPK_REPLAY = 0, 1, 2, 3, 4, 5
# gorse_hip_test_set_topk_variant (include/gorse_hip_test.h, GORSE_TEST_TOPK_*)
TOPK_TILE64, TOPK_COARSE_OFF, TOPK_COARSE_ON, TOPK_REPLAY_COUNTERS = 1 << 0, 1 << 2, 1 << 3, 1 << 4
TOPK_WARM_OFF, TOPK_WARM_ALWAYS, TOPK_PILOT_KTH2, TOPK_COLD_SLICES = 1 << 8, 1 << 9, 1 << 10, 1 << 11
TOPK_SLICES8, TOPK_SLICE1, TOPK_SYM_OFF, TOPK_REPLAY_WAVE64 = 1 << 14, 1 << 15, 1 << 23, 1 << 28
TOPK_VARIANT_MASK = (TOPK_TILE64 | TOPK_COARSE_OFF | TOPK_COARSE_ON | TOPK_REPLAY_COUNTERS | TOPK_WARM_OFF | TOPK_WARM_ALWAYS | TOPK_PILOT_KTH2 |
                     TOPK_COLD_SLICES | TOPK_SLICES8 | TOPK_SLICE1 | TOPK_SYM_OFF | TOPK_REPLAY_WAVE64 | (3 << 29))


def TOPK_TRI_SLICES(n):
    """GORSE_TEST_TOPK_TRI_SLICES(n): n = 1 / 2 / 3 -> one / two / four row slices per query block of a triangle-sharded sweep"""
    return (n & 3) << 29

_f32p = C.POINTER(C.c_float)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)
_vp = C.c_void_p
_u8p = C.POINTER(C.c_uint8)

# name -> (restype, argtypes); mirrors include/gorse_hip.h (the boundary) and include/gorse_hip_test.h (test hooks) one to one
SIGNATURES = {
    "gorse_hip_abi_version": (C.c_int32, []),
    "gorse_hip_last_error": (C.c_char_p, []),
    "gorse_hip_device_count": (C.c_int32, [_i32p]),
    "gorse_mf_create": (C.c_int32, [C.POINTER(_vp), C.c_int32, C.c_int64, C.c_int64, C.c_int32, _i64p, _i32p, _i64p, _i32p]),
    "gorse_mf_destroy": (C.c_int32, [_vp]),
    "gorse_mf_set_factors": (C.c_int32, [_vp, _f32p, _f32p]),
    "gorse_mf_get_factors": (C.c_int32, [_vp, _f32p, _f32p]),
    "gorse_mf_score": (C.c_int32, [_vp, _i32p, _i32p, C.c_int64, _f32p]),
    "gorse_mf_rank": (C.c_int32, [_vp, C.c_int64, _i32p, _i64p, _i32p, C.c_int32, _i32p, _i32p]),
    "gorse_mf_recommend": (C.c_int32, [_vp, C.c_int64, _i32p, C.c_int32, C.POINTER(C.c_uint8), _i64p, _i32p, _i32p, _f32p, _i32p]),
    "gorse_mf_recommend_stats": (C.c_int32, [_vp, _i64p, _i64p, _f64p]),
    "gorse_mf_sample_user_negatives": (C.c_int32, [_vp, _i64p, _i32p, C.c_int32, C.c_uint64, _i32p, _i32p]),
    "gorse_mf_resident_candidates": (C.c_int32, [_vp, _i64p, _i64p]),
    "gorse_mf_resident_generation": (C.c_int32, [_vp, C.POINTER(C.c_uint64)]),
    "gorse_mf_rank_resident": (C.c_int32, [_vp, C.c_int32, _i32p, _i32p, _i32p]),
    "gorse_mf_evaluate_resident": (C.c_int32, [_vp, C.c_int32, _f32p, _f32p, _f32p, _i32p, _i32p]),
    "gorse_mf_evaluate": (C.c_int32, [_vp, C.c_int64, _i32p, _i64p, _i32p, _i64p, _i32p, C.c_int32, _f32p, _f32p, _f32p]),
    "gorse_mf_evaluate_stats": (C.c_int32, [_vp, _i64p, _i64p, _f64p]),
    "gorse_bpr_epoch": (C.c_int32, [_vp, C.c_int64, C.c_float, C.c_float, C.c_uint64, C.c_uint64, C.c_int64, C.c_int32,
                                    _i32p, _f64p]),
    "gorse_bpr_epoch_enqueue": (C.c_int32, [_vp, C.c_int64, C.c_float, C.c_float, C.c_uint64, C.c_uint64, C.c_int64,
                                            C.c_int32]),
    "gorse_bpr_sample_triplets": (C.c_int32, [_vp, C.c_int64, C.c_uint64, C.c_uint64, C.c_int64, _i32p, _i32p, _i32p]),
    "gorse_bpr_apply_triplets": (C.c_int32, [_vp, _i32p, _i32p, _i32p, C.c_int64, C.c_float, C.c_float, C.c_int32]),
    "gorse_mf_bpr_schedule": (C.c_int32, [_vp, _i32p]),
    "gorse_mf_set_bpr_cold_window": (C.c_int32, [_vp, C.c_int64, _i64p]),
    "gorse_als_epoch": (C.c_int32, [_vp, C.c_float, C.c_float, _i32p]),
    "gorse_als_set_ranges": (C.c_int32, [_vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "gorse_als_half_epoch": (C.c_int32, [_vp, C.c_int32, C.c_float, C.c_float]),
    "gorse_als_half_epoch_enqueue": (C.c_int32, [_vp, C.c_int32, C.c_float, C.c_float]),
    "gorse_mf_rows_export": (C.c_int32, [_vp, C.c_int32, C.c_int64, C.c_int64, _vp]),
    "gorse_mf_rows_import": (C.c_int32, [_vp, C.c_int32, C.c_int64, C.c_int64, _vp]),
    "gorse_mf_item_sync_mark": (C.c_int32, [_vp]),
    "gorse_mf_item_delta_export": (C.c_int32, [_vp, _vp]),
    "gorse_mf_item_delta_import": (C.c_int32, [_vp, _vp]),
    "gorse_mf_device_ptrs": (C.c_int32, [_vp, C.POINTER(_vp), C.POINTER(_vp)]),
    "gorse_comm_unique_id": (C.c_int32, [_vp]),
    "gorse_comm_create": (C.c_int32, [C.POINTER(_vp), _vp, C.c_int32, C.c_int32, C.c_int32]),
    "gorse_comm_create_local": (C.c_int32, [C.POINTER(_vp), _i32p, C.c_int32]),
    "gorse_comm_destroy": (C.c_int32, [_vp]),
    "gorse_comm_info": (C.c_int32, [_vp, _i32p, _i32p]),
    "gorse_mf_item_allreduce": (C.c_int32, [C.POINTER(_vp), C.POINTER(_vp), C.c_int32]),
    "gorse_mf_rows_allgather": (C.c_int32, [C.POINTER(_vp), C.POINTER(_vp), C.c_int32, C.c_int32, _i64p]),
    "gorse_comm_allreduce_f32": (C.c_int32, [_vp, _f32p, C.c_int64]),
    "gorse_comm_allreduce_f32_local": (C.c_int32, [C.POINTER(_vp), C.c_int32, C.POINTER(_f32p), C.c_int64]),
    "gorse_comm_available": (C.c_int32, []),
    "gorse_mf_synchronize": (C.c_int32, [_vp]),
    "gorse_mf_epoch_throttle": (C.c_int32, [_vp, C.c_int32, _i32p]),
    "gorse_mf_epoch_times": (C.c_int32, [_vp, _i64p, C.POINTER(C.c_double), _i64p, C.c_int32]),
    "gorse_mf_set_profiling": (C.c_int32, [_vp, C.c_int32]),
    "gorse_mf_get_profile": (C.c_int32, [_vp, C.c_int32, _i64p, _f64p]),
    "gorse_mf_reset_profile": (C.c_int32, [_vp]),
    "gorse_topk_create": (C.c_int32, [C.POINTER(_vp), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, _vp]),
    "gorse_topk_destroy": (C.c_int32, [_vp]),
    "gorse_topk_search_index": (C.c_int32, [_vp, _i64p, C.c_int64, C.c_int32, C.c_int32, _i32p, _f32p, _i32p]),
    "gorse_topk_search_vector": (C.c_int32, [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, _i32p, _f32p, _i32p]),
    "gorse_topk_all_pairs": (C.c_int32, [_vp, C.c_int64, C.c_int64, C.c_int32, _i32p, _f32p]),
    "gorse_topk_set_mask": (C.c_int32, [_vp, _vp]),
    "gorse_topk_synchronize": (C.c_int32, [_vp]),
    "gorse_topk_set_profiling": (C.c_int32, [_vp, C.c_int32]),
    "gorse_topk_get_profile": (C.c_int32, [_vp, C.c_int32, _i64p, _f64p]),
    "gorse_topk_last_stats": (C.c_int32, [_vp, _i64p, _i64p]),
    "gorse_sparse_create": (C.c_int32, [C.POINTER(_vp), C.c_int32, C.c_int64, _i64p, _vp, _f32p]),
    "gorse_sparse_destroy": (C.c_int32, [_vp]),
    "gorse_sparse_set_mask": (C.c_int32, [_vp, _vp]),
    "gorse_sparse_search": (C.c_int32, [_vp, C.c_int64, _i64p, _vp, _f32p, _i64p, C.c_int32, _i32p, _f32p, _i32p]),
    "gorse_sparse_all_pairs": (C.c_int32, [_vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, _i32p, _f32p, _i32p]),
    "gorse_sparse_synchronize": (C.c_int32, [_vp]),
    "gorse_sparse_set_profiling": (C.c_int32, [_vp, C.c_int32]),
    "gorse_sparse_get_profile": (C.c_int32, [_vp, _i64p, _f64p]),
    "gorse_sparse_last_stats": (C.c_int32, [_vp, _i64p, _i64p]),
    "gorse_hip_sgemm": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _f32p, C.c_int32,
                                    _f32p, C.c_int32, _f32p, C.c_int32]),
    "gorse_hip_sgemm_device": (C.c_int32, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32,
                                           _vp, C.c_int32, _vp, C.c_int32]),
    "gorse_fm_create": (C.c_int32, [C.POINTER(_vp), C.c_int32, C.c_int64, C.c_int32]),
    "gorse_fm_destroy": (C.c_int32, [_vp]),
    "gorse_fm_set_params": (C.c_int32, [_vp, C.c_float, _f32p, _f32p]),
    "gorse_fm_get_params": (C.c_int32, [_vp, _f32p, _f32p, _f32p]),
    "gorse_fm_set_train": (C.c_int32, [_vp, C.c_int64, C.c_int32, _i32p, _f32p, _f32p]),
    "gorse_fm_epoch": (C.c_int32, [_vp, C.c_int32, C.c_int32, C.c_float, C.c_float, _i32p, _f32p]),
    "gorse_fm_predict": (C.c_int32, [_vp, C.c_int64, C.c_int32, _i32p, _f32p, _f32p]),
    "gorse_fm_set_embedding_dims": (C.c_int32, [_vp, C.c_int32, _i32p]),
    "gorse_fm_set_embedding_params": (C.c_int32, [_vp, C.c_int32, _f32p, _f32p, _f32p, _f32p, _f32p]),
    "gorse_fm_get_embedding_params": (C.c_int32, [_vp, C.c_int32, _f32p, _f32p, _f32p, _f32p, _f32p]),
    "gorse_fm_set_train_embeddings": (C.c_int32, [_vp, C.c_int32, C.POINTER(C.c_uint16)]),
    "gorse_fm_predict_embeddings": (C.c_int32, [_vp, C.c_int64, C.c_int32, _i32p, _f32p, C.POINTER(C.POINTER(C.c_uint16)),
                                                C.c_int32, _f32p]),
    "gorse_fm_set_items": (C.c_int32, [_vp, C.c_int64, _i64p, _i32p, _f32p, _i32p, C.POINTER(C.POINTER(C.c_uint16))]),
    "gorse_fm_rank_users": (C.c_int32, [_vp, C.c_int64, _i64p, _i32p, _f32p, _i32p, _i64p, _i32p, C.c_int32, _i32p, _f32p,
                                        _i32p]),
    "gorse_fm_rank_stats": (C.c_int32, [_vp, _i64p, _i64p, _i64p, _i64p, _f64p]),
    "gorse_fm_set_test": (C.c_int32, [_vp, C.c_int64, C.c_int32, _i32p, _f32p, _f32p, C.POINTER(C.POINTER(C.c_uint16))]),
    "gorse_fm_evaluate": (C.c_int32, [_vp, C.c_int32, _i32p, _i64p, _f32p, _f32p]),
    "gorse_fm_evaluate_stats": (C.c_int32, [_vp, _i64p, _i64p, _i64p, _f64p]),
    "gorse_fm_set_train_samples": (C.c_int32, [_vp, C.c_int64, _i64p, _i32p, _f32p, _i32p, C.c_int64, _i32p, _i32p, _f32p]),
    "gorse_fm_set_test_samples": (C.c_int32, [_vp, C.c_int64, _i64p, _i32p, _f32p, _i32p, C.c_int64, _i32p, _i32p, _f32p]),
    "gorse_hip_test_set_exact_exp": (None, [C.c_int32]),
    "gorse_hip_test_set_variant": (None, [C.c_int32]),
    "gorse_hip_test_set_topk_path": (None, [C.c_int32]),
    "gorse_hip_test_set_topk_variant": (None, [C.c_int32]),
    "gorse_hip_test_get_sweep_profile": (C.c_int32, [_vp, C.POINTER(C.c_uint64)]),
    "gorse_topk_tri_begin": (C.c_int32, [_vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    "gorse_topk_tri_slice": (C.c_int32, [_vp, C.c_int32, _i64p, _i64p, _i64p]),
    "gorse_topk_tri_thresholds_get": (C.c_int32, [_vp, C.c_int64, C.c_int64, _vp]),
    "gorse_topk_tri_thresholds_put": (C.c_int32, [_vp, C.c_int64, C.c_int64, _vp]),
    "gorse_topk_tri_sweep": (C.c_int32, [_vp]),
    "gorse_topk_tri_pack": (C.c_int32, [_vp, C.c_int32, _i64p, _i64p]),
    "gorse_topk_tri_pack_read": (C.c_int32, [_vp, _vp, _vp]),
    "gorse_topk_tri_unpack": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int64, _vp, C.c_int64]),
    "gorse_topk_tri_finish": (C.c_int32, [_vp, _i32p, _f32p]),
    "gorse_topk_tri_all_pairs_local": (C.c_int32, [C.POINTER(_vp), C.c_int32, C.c_int64, C.c_int64, C.c_int32, _i32p, _f32p]),
    "gorse_hip_test_topk_resweeps": (C.c_int32, [_vp, _i64p]),
    "gorse_hip_test_topk_last_symmetric": (C.c_int32, [_vp, C.POINTER(C.c_int32)]),
    "gorse_hip_test_topk_sym_stats": (C.c_int32, [_vp, C.POINTER(C.c_uint64)]),
    "gorse_hip_test_topk_get_thresholds": (C.c_int32, [_vp, _f32p, C.c_int64]),
    "gorse_hip_test_topk_get_flags": (C.c_int32, [_vp, C.POINTER(C.c_uint8), C.c_int64]),
    "gorse_hip_test_topk_get_foreign_counts": (C.c_int32, [_vp, _i32p, C.c_int64]),
    "gorse_hip_test_set_sparse_slots": (None, [C.c_int64]),
    "gorse_hip_test_set_sparse_head": (None, [C.c_int32]),
    "gorse_hip_test_set_sparse_sym": (None, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "gorse_hip_test_set_sparse_front": (None, [C.c_int32]),
    "gorse_hip_test_sparse_sym_stats": (None, [C.c_void_p, C.POINTER(C.c_int64)]),
    "gorse_hip_test_sparse_path_stats": (None, [C.c_void_p, C.POINTER(C.c_int64)]),
    "gorse_hip_test_set_sparse_tile": (None, [C.c_int32]),
    "gorse_hip_test_set_scan_literal": (None, [C.c_int32]),
    "gorse_hip_test_topk_scan_flags": (C.c_int32, [_vp, _i32p, C.c_int64]),
    "gorse_hip_test_set_scan_block": (None, [C.c_int64]),
    "gorse_hip_test_set_sparse_split": (None, [C.c_int64]),
    "gorse_hip_test_set_sparse_heavy": (None, [C.c_int64]),
    "gorse_hip_test_set_sparse_atomic": (None, [C.c_int32]),
    "gorse_hip_test_set_als_path": (None, [C.c_int32]),
    "gorse_hip_test_set_als_plan": (None, [C.c_int32, C.c_int32]),
    "gorse_hip_test_set_bpr_chunk": (None, [C.c_int64]),
    "gorse_hip_test_bpr_prepare_chunk": (C.c_int32, [_vp, C.c_int64, C.c_uint64, C.c_uint64, C.c_int64, _i32p, _i32p, _i32p]),
    "gorse_hip_test_bpr_finish_capacities": (None, [_i32p, _i32p]),
    "gorse_hip_test_bpr_fail_count": (C.c_int32, [_vp, _i32p]),
    "gorse_hip_test_set_bpr_store_mode": (None, [C.c_int32]),
    "gorse_hip_test_set_sgemm_valu": (None, [C.c_int32]),
    "gorse_hip_test_sgemm_last_ms": (C.c_double, []),
    "gorse_hip_test_sgemm_last_form": (C.c_int32, []),
    "gorse_hip_test_set_bpr_cold_window": (None, [C.c_int64]),
    "gorse_hip_test_set_bpr_replica_unit": (None, [C.c_double]),
    "gorse_hip_test_set_bpr_fold_period": (None, [C.c_int32]),
    "gorse_hip_test_bpr_fold_stats": (C.c_int32, [_vp, _vp]),
    "gorse_hip_test_bpr_hot_state": (C.c_int32, [_vp, _vp, _vp, _vp]),
    "gorse_hip_test_set_bpr_acc_rows": (None, [C.c_int32]),
    "gorse_hip_test_set_bpr_acc_fold_every": (None, [C.c_int32]),
    "gorse_hip_test_bpr_acc_state": (C.c_int32, [_vp, _vp, _vp]),
    "gorse_hip_test_bpr_item_classes": (C.c_int32, [_vp, _vp, _vp]),
    "gorse_hip_test_bpr_fold_tier_stats": (C.c_int32, [_vp, _vp]),
    "gorse_hip_test_set_bpr_folder_timeout": (None, [C.c_int64]),
    "gorse_hip_test_set_recommend": (None, [C.c_int32, C.c_int32, C.c_int64]),
    "gorse_hip_test_set_fm_rank": (None, [C.c_int64, C.c_int32]),
    "gorse_hip_test_fm_rank_sort": (C.c_int32, [_vp, C.c_int64, _i64p, _f32p, _i32p]),
    "gorse_hip_test_set_fm_evaluate": (None, [C.c_int64, C.c_int32]),
    "gorse_hip_test_fm_auc": (C.c_int32, [_vp, _f32p, C.c_int64, _f32p, C.c_int64, _i64p, _f32p]),
    "gorse_hip_test_fm_evaluate_times": (C.c_int32, [_vp, _f64p]),
    "gorse_hip_test_mf_evaluate_times": (C.c_int32, [_vp, _f64p]),
    "gorse_hip_test_mf_evaluate_tables": (C.c_int32, [_f32p, _f32p, C.c_int32]),
    "gorse_nbr_create": (C.c_int32, [C.POINTER(_vp), C.c_int32, C.c_int64]),
    "gorse_nbr_destroy": (C.c_int32, [_vp]),
    "gorse_nbr_set_table": (C.c_int32, [_vp, C.c_int32, C.c_int64, _i64p, _i32p, _f32p, C.c_int32, C.c_double]),
    "gorse_nbr_recommend": (C.c_int32, [_vp, C.c_int64, _i32p, C.c_int32, _i64p, _i32p, _i32p, _f64p, _i32p]),
    "gorse_nbr_recommend_stats": (C.c_int32, [_vp, _i64p, _i64p, _f64p]),
    "gorse_nbr_set_table_from_topk": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int64, _i64p, C.c_int32, C.c_int32, C.c_int32, C.c_double]),
    "gorse_nbr_set_table_from_sparse": (C.c_int32, [_vp, C.c_int32, _vp, C.c_int64, _i64p, C.c_int32, C.c_int32, C.c_int32, C.c_double]),
    "gorse_nbr_table_info": (C.c_int32, [_vp, C.c_int32, _i64p, _i64p, _i32p]),
    "gorse_nbr_get_table": (C.c_int32, [_vp, C.c_int32, _i64p, _i32p, _f32p]),
    "gorse_hip_test_set_nbr": (None, [C.c_int32, C.c_int64]),
    "gorse_cand_create": (C.c_int32, [C.POINTER(_vp), C.c_int32, C.c_int64]),
    "gorse_cand_destroy": (C.c_int32, [_vp]),
    "gorse_cand_begin": (C.c_int32, [_vp, C.c_int64, _i64p, _i32p, C.c_int32]),
    "gorse_cand_add_mf": (C.c_int32, [_vp, _vp, _i32p, C.c_int32, _u8p, _u8p]),
    "gorse_cand_add_nbr": (C.c_int32, [_vp, _vp, _i32p, C.c_int32, _u8p]),
    "gorse_cand_add_shared": (C.c_int32, [_vp, C.c_int64, _i32p, _f64p, C.c_int32, _u8p]),
    "gorse_cand_add_lists": (C.c_int32, [_vp, _i64p, _i32p, _f64p, C.c_int32, _u8p]),
    "gorse_cand_finish": (C.c_int32, [_vp, _u8p]),
    "gorse_cand_info": (C.c_int32, [_vp, _i64p, _i32p, _i64p, _i64p]),
    "gorse_cand_get": (C.c_int32, [_vp, _i64p, _i32p, _f64p, _u8p]),
    "gorse_cand_get_exclusion": (C.c_int32, [_vp, _i64p, _i32p]),
    "gorse_cand_stats": (C.c_int32, [_vp, C.c_int32, _f64p, _f64p]),
    "gorse_fm_rank_cand": (C.c_int32, [_vp, _vp, _i64p, _i32p, _f32p, _i32p, C.c_int32, _i32p, _f32p, _i32p]),
    "gorse_cand_add_replacement": (C.c_int32, [_vp, _i64p, _i32p, _u8p, _u8p]),
    "gorse_cand_get_replacement": (C.c_int32, [_vp, _i64p, _i32p, _u8p]),
    "gorse_cand_replacement_stats": (C.c_int32, [_vp, _i64p, _i64p, _i64p, _f64p]),
    "gorse_fm_rank_cand_decayed": (C.c_int32, [_vp, _vp, _i64p, _i32p, _f32p, _i32p, C.c_int32, _i32p, C.c_double, C.c_double, _f32p, _f64p,
                                               _i32p]),
}


class GorseHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libgorse_hip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Load libgorse_hip.so (once). Raises if it has not been built -- there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the HIP extension is mandatory; there is no CPU path)" % LIB_PATH)
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != OK:
        raise GorseHipError(rc, lib().gorse_hip_last_error().decode("utf-8", "replace"))


def device_count():
    n = C.c_int32(0)
    rc = lib().gorse_hip_device_count(C.byref(n))
    return n.value if rc == OK else 0


def mf_evaluate_tables(n=MF_EVAL_MAX_TOPK):
    """the evaluation kernel's two tables as the library fills them: (1 / log2f(i + 2) for i < n, IDCG prefix sums for k <= n)"""
    inv_log, idcg = np.zeros(n, np.float32), np.zeros(n + 1, np.float32)
    check(lib().gorse_hip_test_mf_evaluate_tables(inv_log.ctypes.data_as(_f32p), idcg.ctypes.data_as(_f32p), n))
    return inv_log, idcg


def _arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


class MF:
    """One gorse_mf handle (one model resident on one GPU)."""

    def __init__(self, U, I, d, user_indptr, user_indices, item_indptr=None, item_indices=None, device=0):
        self.U, self.I, self.d = int(U), int(I), int(d)
        up, ui = _arr(user_indptr, np.int64), _arr(user_indices, np.int32)
        if up.size != self.U + 1:
            raise GorseHipError(ERR_INVALID, "user_indptr must have U+1 entries")
        ip = _arr(item_indptr, np.int64) if item_indptr is not None else None
        ii = _arr(item_indices, np.int32) if item_indices is not None else None
        self.h = _vp()
        check(lib().gorse_mf_create(C.byref(self.h), device, self.U, self.I, self.d, _p(up, _i64p), _p(ui, _i32p),
                                    _p(ip, _i64p), _p(ii, _i32p)))

    def close(self):
        if getattr(self, "h", None):
            lib().gorse_mf_destroy(self.h)
            self.h = None

    __del__ = close

    def set_factors(self, P=None, Q=None):
        P = _arr(P, np.float32) if P is not None else None
        Q = _arr(Q, np.float32) if Q is not None else None
        if P is not None and P.shape != (self.U, self.d):
            raise GorseHipError(ERR_INVALID, "P must be U x d")
        if Q is not None and Q.shape != (self.I, self.d):
            raise GorseHipError(ERR_INVALID, "Q must be I x d")
        check(lib().gorse_mf_set_factors(self.h, _p(P, _f32p), _p(Q, _f32p)))

    def get_factors(self):
        P = np.empty((self.U, self.d), np.float32)
        Q = np.empty((self.I, self.d), np.float32)
        check(lib().gorse_mf_get_factors(self.h, _p(P, _f32p), _p(Q, _f32p)))
        return P, Q

    def score(self, u, i):
        u, i = _arr(u, np.int32), _arr(i, np.int32)
        out = np.empty(u.size, np.float32)
        check(lib().gorse_mf_score(self.h, _p(u, _i32p), _p(i, _i32p), u.size, _p(out, _f32p)))
        return out

    def rank(self, users, cand_indptr, cand, topk):
        users, cand_indptr, cand = _arr(users, np.int32), _arr(cand_indptr, np.int64), _arr(cand, np.int32)
        rank = np.empty((users.size, topk), np.int32)
        rlen = np.empty(users.size, np.int32)
        check(lib().gorse_mf_rank(self.h, users.size, _p(users, _i32p), _p(cand_indptr, _i64p), _p(cand, _i32p), topk,
                                  _p(rank, _i32p), _p(rlen, _i32p)))
        return rank, rlen

    def recommend(self, users, k, item_ok=None, seen_indptr=None, seen_items=None):
        """every query's k best unseen items (gorse_mf_recommend): (items n x k padded with -1, scores n x k padded with 0, counts n).
        users = None: all users of the handle, or an int n: the first n; seen rows are per QUERY (seen_indptr has n + 1 entries)."""
        if users is None or isinstance(users, (int, np.integer)):
            n, up = (self.U if users is None else int(users)), None
        else:
            up = _arr(users, np.int32)
            n = up.size
        ok = _arr(item_ok, np.uint8) if item_ok is not None else None
        if ok is not None and ok.size != self.I:
            raise GorseHipError(ERR_INVALID, "item_ok must have I entries")
        sp = _arr(seen_indptr, np.int64) if seen_indptr is not None else None
        if sp is not None and sp.size != n + 1:
            raise GorseHipError(ERR_INVALID, "seen_indptr must have n_users + 1 entries")
        si = _arr(seen_items, np.int32) if seen_items is not None else None
        if si is not None and si.size == 0:
            si = np.zeros(1, np.int32)
        kk = max(int(k), 0)
        items = np.full((n, kk), -2, np.int32)
        scores = np.full((n, kk), np.nan, np.float32)
        counts = np.full(n, -2, np.int32)
        check(lib().gorse_mf_recommend(self.h, n, _p(up, _i32p), k, _p(ok, C.POINTER(C.c_uint8)), _p(sp, _i64p), _p(si, _i32p),
                                       _p(items, _i32p), _p(scores, _f32p), _p(counts, _i32p)))
        return items, scores, counts

    def recommend_stats(self):
        """the last recommend(): (queries answered by the threshold kernel, queries answered literally, device milliseconds)"""
        nf, nl, ms = C.c_int64(0), C.c_int64(0), C.c_double(0)
        check(lib().gorse_mf_recommend_stats(self.h, C.byref(nf), C.byref(nl), C.byref(ms)))
        return nf.value, nl.value, ms.value

    def sample_user_negatives(self, test_indptr, test_indices, num_candidates, seed=0, fetch=True):
        """dataset.SampleUserNegatives on the device: (neg U x n padded with -1, len U); the candidate lists of the users with
        test feedback stay resident for rank_resident"""
        tp, ti = _arr(test_indptr, np.int64), _arr(test_indices, np.int32)
        if ti.size == 0:
            ti = np.zeros(1, np.int32)
        neg = np.empty((self.U, num_candidates), np.int32) if fetch else None
        ln = np.empty(self.U, np.int32) if fetch else None
        check(lib().gorse_mf_sample_user_negatives(self.h, _p(tp, _i64p), _p(ti, _i32p), num_candidates, seed,
                                                   _p(neg, _i32p) if fetch else None, _p(ln, _i32p) if fetch else None))
        return neg, ln

    def rank_resident(self, topk):
        """Rank over the resident candidate lists: (users, rank n_users x topk padded with -1, lengths)"""
        nu, nc = C.c_int64(0), C.c_int64(0)
        check(lib().gorse_mf_resident_candidates(self.h, C.byref(nu), C.byref(nc)))
        users = np.empty(nu.value, np.int32)
        rank = np.empty((nu.value, topk), np.int32)
        rlen = np.empty(nu.value, np.int32)
        if nu.value:
            check(lib().gorse_mf_rank_resident(self.h, topk, _p(users, _i32p), _p(rank, _i32p), _p(rlen, _i32p)))
        return users, rank, rlen

    def evaluate_resident(self, topk, per_user=False, ranks=False):
        """cf.Evaluate's ranking and metrics over the resident lists (gorse_mf_evaluate_resident): (sums 6, count), the metrics
        in the order NDCG, Precision, Recall, HR, MAP, MRR; then per_user 6 x n_users when asked for, then (rank n_users x topk
        padded with -1, lengths) when asked for"""
        nu, nc = C.c_int64(0), C.c_int64(0)
        check(lib().gorse_mf_resident_candidates(self.h, C.byref(nu), C.byref(nc)))
        sums, count = np.full(6, np.nan, np.float32), C.c_float(0)
        pu = np.full((6, nu.value), np.nan, np.float32) if per_user else None
        rank = np.full((nu.value, max(int(topk), 0)), -2, np.int32) if ranks else None
        rlen = np.full(nu.value, -2, np.int32) if ranks else None
        check(lib().gorse_mf_evaluate_resident(self.h, topk, _p(sums, _f32p), C.byref(count), _p(pu, _f32p), _p(rank, _i32p),
                                               _p(rlen, _i32p)))
        return (sums, np.float32(count.value)) + ((pu,) if per_user else ()) + ((rank, rlen) if ranks else ())

    def evaluate(self, users, target_indptr, targets, cand_indptr, cand, topk, per_user=False):
        """the same over lists given here (gorse_mf_evaluate): targets and candidates as CSRs with one row per entry of users"""
        users, tp, cp = _arr(users, np.int32), _arr(target_indptr, np.int64), _arr(cand_indptr, np.int64)
        tg, cd = _arr(targets, np.int32), _arr(cand, np.int32)
        if tp.size != users.size + 1 or cp.size != users.size + 1:
            raise GorseHipError(ERR_INVALID, "target_indptr and cand_indptr must have n_users + 1 entries")
        tg = tg if tg.size else np.zeros(1, np.int32)
        cd = cd if cd.size else np.zeros(1, np.int32)
        sums, count = np.full(6, np.nan, np.float32), C.c_float(0)
        pu = np.full((6, users.size), np.nan, np.float32) if per_user else None
        check(lib().gorse_mf_evaluate(self.h, users.size, _p(users, _i32p), _p(tp, _i64p), _p(tg, _i32p), _p(cp, _i64p),
                                      _p(cd, _i32p), topk, _p(sums, _f32p), C.byref(count), _p(pu, _f32p)))
        return (sums, np.float32(count.value)) + ((pu,) if per_user else ())

    def evaluate_stats(self):
        """the last evaluate / evaluate_resident: (users counted, candidates scored, device milliseconds)"""
        nu, nc, ms = C.c_int64(0), C.c_int64(0), C.c_double(0)
        check(lib().gorse_mf_evaluate_stats(self.h, C.byref(nu), C.byref(nc), C.byref(ms)))
        return nu.value, nc.value, ms.value

    def evaluate_stage_times(self):
        """device milliseconds of the last evaluation by stage: (per-user kernel, sum chain)"""
        ms = np.zeros(2, np.float64)
        check(lib().gorse_hip_test_mf_evaluate_times(self.h, _p(ms, _f64p)))
        return float(ms[0]), float(ms[1])

    def set_bpr_cold_window(self, samples):
        """the cold window of THIS handle (GORSE_BPR_HOGWILD_STORES); returns the number of cold items"""
        n = C.c_int64(0)
        check(lib().gorse_mf_set_bpr_cold_window(self.h, samples, C.byref(n)))
        return n.value

    def bpr_epoch(self, n_samples, lr, reg, seed, epoch, sample_base=0, mode=BPR_HOGWILD_STORES, want_loss=False,
                  cancel=None):
        loss = C.c_double(0)
        cp = _p(cancel, _i32p) if cancel is not None else None
        check(lib().gorse_bpr_epoch(self.h, n_samples, lr, reg, seed, epoch, sample_base, mode, cp,
                                    C.byref(loss) if want_loss else None))
        return loss.value

    def bpr_epoch_enqueue(self, n_samples, lr, reg, seed, epoch, sample_base=0, mode=BPR_HOGWILD_STORES):
        check(lib().gorse_bpr_epoch_enqueue(self.h, n_samples, lr, reg, seed, epoch, sample_base, mode))

    def bpr_sample_triplets(self, n, seed, epoch, sample_base=0):
        u = np.empty(n, np.int32)
        i = np.empty(n, np.int32)
        j = np.empty(n, np.int32)
        check(lib().gorse_bpr_sample_triplets(self.h, n, seed, epoch, sample_base, _p(u, _i32p), _p(i, _i32p),
                                              _p(j, _i32p)))
        return u, i, j

    def bpr_prepare_chunk(self, n, seed, epoch, sample_base=0):
        """test hook: (run offsets U + 2, positives n, negatives n) of the user-run schedule's preparation of one chunk"""
        off = np.empty(self.U + 2, np.int32)
        si = np.empty(n, np.int32)
        sj = np.empty(n, np.int32)
        check(lib().gorse_hip_test_bpr_prepare_chunk(self.h, n, seed, epoch, sample_base, _p(off, _i32p), _p(si, _i32p),
                                                     _p(sj, _i32p)))
        return off, si, sj

    def bpr_fail_count(self):
        """test hook: samples the BPR samplers of this handle have given up on so far"""
        n = C.c_int32(0)
        check(lib().gorse_hip_test_bpr_fail_count(self.h, C.byref(n)))
        return n.value

    def bpr_apply_triplets(self, u, i, j, lr, reg, mode):
        u, i, j = _arr(u, np.int32), _arr(i, np.int32), _arr(j, np.int32)
        if not (u.size == i.size == j.size):
            raise GorseHipError(ERR_INVALID, "triplet arrays differ in length")
        check(lib().gorse_bpr_apply_triplets(self.h, _p(u, _i32p), _p(i, _i32p), _p(j, _i32p), u.size, lr, reg, mode))

    def als_epoch(self, weight, reg, cancel=None):
        cp = _p(cancel, _i32p) if cancel is not None else None
        check(lib().gorse_als_epoch(self.h, weight, reg, cp))

    def item_sync_mark(self):
        check(lib().gorse_mf_item_sync_mark(self.h))

    def bpr_user_runs(self):
        v = C.c_int32(0)
        check(lib().gorse_mf_bpr_schedule(self.h, C.byref(v)))
        return bool(v.value)

    def als_set_ranges(self, u_begin, u_end, i_begin, i_end):
        check(lib().gorse_als_set_ranges(self.h, u_begin, u_end, i_begin, i_end))

    def als_half_epoch(self, side, weight, reg):
        check(lib().gorse_als_half_epoch(self.h, side, weight, reg))

    def als_half_epoch_enqueue(self, side, weight, reg):
        check(lib().gorse_als_half_epoch_enqueue(self.h, side, weight, reg))

    def rows_export(self, side, begin, end, dev_ptr):
        check(lib().gorse_mf_rows_export(self.h, side, begin, end, _vp(dev_ptr)))

    def rows_import(self, side, begin, end, dev_ptr):
        check(lib().gorse_mf_rows_import(self.h, side, begin, end, _vp(dev_ptr)))

    def item_delta_export(self, dev_ptr):
        check(lib().gorse_mf_item_delta_export(self.h, _vp(dev_ptr)))

    def item_delta_import(self, dev_ptr):
        check(lib().gorse_mf_item_delta_import(self.h, _vp(dev_ptr)))

    def device_ptrs(self):
        P, Q = _vp(), _vp()
        check(lib().gorse_mf_device_ptrs(self.h, C.byref(P), C.byref(Q)))
        return P.value, Q.value

    def synchronize(self):
        check(lib().gorse_mf_synchronize(self.h))

    def epoch_throttle(self, max_in_flight, cancel=None):
        """blocks until at most max_in_flight enqueued epochs are unfinished; raises GorseHipError(ERR_CANCELLED) when *cancel is set"""
        check(lib().gorse_mf_epoch_throttle(self.h, max_in_flight, _p(cancel, _i32p) if cancel is not None else None))

    def epoch_times(self, reset=False):
        """(finished epochs, their device milliseconds, epochs still in flight) since the last reset"""
        n, ms, fl = C.c_int64(0), C.c_double(0), C.c_int64(0)
        check(lib().gorse_mf_epoch_times(self.h, C.byref(n), C.byref(ms), C.byref(fl), int(bool(reset))))
        return n.value, ms.value, fl.value

    def set_profiling(self, on):
        check(lib().gorse_mf_set_profiling(self.h, int(bool(on))))

    def reset_profile(self):
        check(lib().gorse_mf_reset_profile(self.h))

    def get_profile(self, cls):
        n, ms = C.c_int64(0), C.c_double(0)
        check(lib().gorse_mf_get_profile(self.h, cls, C.byref(n), C.byref(ms)))
        return n.value, ms.value


EVAL_COUNTS = ("n_pos", "n_neg", "pos_above", "neg_above", "neg_below", "nan", "pairs_less")


class FM:
    """One gorse_fm handle: a factorization machine (ctr.AFM) resident on one GPU, with its item-embedding attention branch when
    embedding_dims names fields.  Rows are n x width matrices of feature indices and values, padded with index 0 / value 0;
    embeddings are n x D matrices of bf16 bit patterns (uint16)."""

    def __init__(self, n_features, n_factors, device=0, embedding_dims=None):
        self.nf, self.d = int(n_features), int(n_factors)
        self.dims = ()
        self.h = _vp()
        check(lib().gorse_fm_create(C.byref(self.h), device, self.nf, self.d))
        if embedding_dims is not None:
            self.set_embedding_dims(embedding_dims)

    def set_embedding_dims(self, dims):
        """the item-embedding fields' dimensions (an empty list: the plain factorization machine)"""
        dims = _arr(list(dims), np.int32).reshape(-1)
        check(lib().gorse_fm_set_embedding_dims(self.h, dims.size, _p(dims, _i32p) if dims.size else None))
        self.dims = tuple(int(x) for x in dims)

    def _field_shapes(self, field):
        D = self.dims[field]
        return ((self.d, D), (D, self.d), (self.d,), (D, self.d), (self.d,))

    def set_embedding_params(self, field, H, Wa, ba, We, be):
        if not 0 <= field < len(self.dims):
            raise GorseHipError(ERR_INVALID, "embedding field out of range")
        arrs = [_arr(a, np.float32) for a in (H, Wa, ba, We, be)]
        for a, shp in zip(arrs, self._field_shapes(field)):
            if a.size != int(np.prod(shp)):
                raise GorseHipError(ERR_INVALID, "H is d x D, Wa and We are D x d, ba and be hold d values")
        check(lib().gorse_fm_set_embedding_params(self.h, field, *[_p(a, _f32p) for a in arrs]))

    def get_embedding_params(self, field):
        """(H, Wa, ba, We, be) of one field"""
        if not 0 <= field < len(self.dims):
            raise GorseHipError(ERR_INVALID, "embedding field out of range")
        arrs = [np.empty(shp, np.float32) for shp in self._field_shapes(field)]
        check(lib().gorse_fm_get_embedding_params(self.h, field, *[_p(a, _f32p) for a in arrs]))
        return tuple(arrs)

    def set_train_embeddings(self, field, emb):
        """the training rows' embeddings of one field: an n x D matrix of bf16 bit patterns (uint16)"""
        emb = _arr(emb, np.uint16)
        check(lib().gorse_fm_set_train_embeddings(self.h, field, _p(emb, C.POINTER(C.c_uint16))))

    def predict_embeddings(self, indices, values, embs, batch_size):
        """logits of the rows scored in slices of batch_size rows; embs: one n x D uint16 (bf16) matrix per field"""
        idx, val = self._rows(indices, values)
        embs = [_arr(e, np.uint16) for e in embs]
        if len(embs) != len(self.dims) or any(e.shape != (idx.shape[0], D) for e, D in zip(embs, self.dims)):
            raise GorseHipError(ERR_INVALID, "one n x D embedding matrix per field")
        ptrs = (C.POINTER(C.c_uint16) * max(1, len(embs)))(*[_p(e, C.POINTER(C.c_uint16)) for e in embs])
        out = np.empty(idx.shape[0], np.float32)
        check(lib().gorse_fm_predict_embeddings(self.h, idx.shape[0], idx.shape[1], _p(idx, _i32p), _p(val, _f32p), ptrs,
                                                int(batch_size), _p(out, _f32p)))
        return out

    def set_items(self, indptr, indices, values, lead=None, embs=()):
        """the resident item catalogue of rank_users: the items' feature rows as a CSR (item-id entry first when known, then the
        labels), lead[i] = leading entries that precede the user's labels (None: 0), embs = one n_items x D uint16 (bf16) table
        per field.  An empty catalogue (indptr of one entry) drops it."""
        ptr = _arr(indptr, np.int64).reshape(-1)
        n = ptr.size - 1
        idx, val = _arr(indices, np.int32).reshape(-1), _arr(values, np.float32).reshape(-1)
        if n < 0 or idx.size != val.size or (n > 0 and idx.size < ptr[-1]):
            raise GorseHipError(ERR_INVALID, "indptr holds n_items + 1 entries and indices / values indptr[-1] each")
        ld = _arr(lead, np.int32).reshape(-1) if lead is not None else None
        if ld is not None and ld.size != n:
            raise GorseHipError(ERR_INVALID, "one lead per item")
        embs = [_arr(e, np.uint16) for e in embs]
        if n > 0 and (len(embs) != len(self.dims) or any(e.shape != (n, D) for e, D in zip(embs, self.dims))):
            raise GorseHipError(ERR_INVALID, "one n_items x D embedding table per field")
        ptrs = (C.POINTER(C.c_uint16) * max(1, len(embs)))(*[_p(e, C.POINTER(C.c_uint16)) for e in embs])
        check(lib().gorse_fm_set_items(self.h, max(n, 0), _p(ptr, _i64p), _p(idx, _i32p), _p(val, _f32p), _p(ld, _i32p),
                                       ptrs if embs else None))

    def rank_users(self, user_indptr, user_indices, user_values, cand_indptr, cand, batch_size, user_lead=None, cancel=None,
                   scores=True, order=True):
        """(scores, order) of every user's candidates (catalogue rows), flat in cand's layout: scores[cand_indptr[t] + r] = the
        logit of user t's r-th candidate, order[cand_indptr[t] + r] = the position in t's list of its r-th ranked candidate.
        scores / order: True = return a new array, False / None = not wanted (None in its place), an array = filled in place."""
        uptr, cptr = _arr(user_indptr, np.int64).reshape(-1), _arr(cand_indptr, np.int64).reshape(-1)
        n = uptr.size - 1
        uidx, uval = _arr(user_indices, np.int32).reshape(-1), _arr(user_values, np.float32).reshape(-1)
        cd = _arr(cand, np.int32).reshape(-1)
        if n < 0 or cptr.size != n + 1 or uidx.size != uval.size:
            raise GorseHipError(ERR_INVALID, "user_indptr and cand_indptr hold n_users + 1 entries each")
        # the library reads indptr[-1] entries: only a well-formed pointer array may be trusted with that
        for ptr, arr in ((uptr, uidx), (cptr, cd)):
            if n > 0 and np.all(np.diff(ptr) >= 0) and ptr[0] == 0 and arr.size < ptr[-1]:
                raise GorseHipError(ERR_INVALID, "fewer entries than the pointer array names")
        ul = _arr(user_lead, np.int32).reshape(-1) if user_lead is not None else None
        if ul is not None and ul.size != n:
            raise GorseHipError(ERR_INVALID, "one lead per user")
        total = int(cptr[-1]) if n >= 0 and cptr.size else 0
        outs = []
        for want, dt in ((scores, np.float32), (order, np.int32)):
            if want is True:
                outs.append(np.zeros(max(total, 0), dt))
            elif want is None or want is False:
                outs.append(None)
            else:
                if want.dtype != dt or not want.flags.c_contiguous or want.size < total:
                    raise GorseHipError(ERR_INVALID, "an output array of the wrong type or size")
                outs.append(want)
        check(lib().gorse_fm_rank_users(self.h, max(n, 0), _p(uptr, _i64p), _p(uidx, _i32p), _p(uval, _f32p), _p(ul, _i32p),
                                        _p(cptr, _i64p), _p(cd, _i32p), int(batch_size),
                                        _p(cancel, _i32p) if cancel is not None else None, _p(outs[0], _f32p), _p(outs[1], _i32p)))
        return outs[0], outs[1]

    def rank_cand(self, chain, user_indptr, user_indices, user_values, batch_size, user_lead=None, cancel=None, scores=True,
                  order=True):
        """rank_users with every user's candidates taken on the device from a finished CandidateChain (gorse_fm_rank_cand):
        (scores, order) flat in the layout of chain.get()'s row pointer.  scores / order: True or False."""
        uptr = _arr(user_indptr, np.int64).reshape(-1)
        uidx, uval = _arr(user_indices, np.int32).reshape(-1), _arr(user_values, np.float32).reshape(-1)
        n, _, total, _ = chain.info()
        if uptr.size != n + 1 or uidx.size != uval.size:
            raise GorseHipError(ERR_INVALID, "user_indptr holds one entry per query of the chain and one more")
        if n > 0 and np.all(np.diff(uptr) >= 0) and uptr[0] == 0 and uidx.size < uptr[-1]:
            raise GorseHipError(ERR_INVALID, "fewer entries than the pointer array names")
        ul = _arr(user_lead, np.int32).reshape(-1) if user_lead is not None else None
        if ul is not None and ul.size != n:
            raise GorseHipError(ERR_INVALID, "one lead per user")
        sc = np.zeros(total, np.float32) if scores else None
        od = np.zeros(total, np.int32) if order else None
        check(lib().gorse_fm_rank_cand(self.h, chain.h, _p(uptr, _i64p), _p(uidx, _i32p), _p(uval, _f32p), _p(ul, _i32p), int(batch_size),
                                       _p(cancel, _i32p) if cancel is not None else None, _p(sc, _f32p), _p(od, _i32p)))
        return sc, od

    def rank_cand_decayed(self, chain, user_indptr, user_indices, user_values, batch_size, positive_decay, read_decay, user_lead=None,
                          cancel=None, scores=True, final=True, order=True):
        """rank_cand followed by the replacement decay and the sort of the decayed scores on the device
        (gorse_fm_rank_cand_decayed): (the ranker's float32 scores, the decayed float64 scores, the order), flat in the layout of
        chain.get()'s row pointer.  scores / final / order: True or False."""
        uptr = _arr(user_indptr, np.int64).reshape(-1)
        uidx, uval = _arr(user_indices, np.int32).reshape(-1), _arr(user_values, np.float32).reshape(-1)
        n, _, total, _ = chain.info()
        if uptr.size != n + 1 or uidx.size != uval.size:
            raise GorseHipError(ERR_INVALID, "user_indptr holds one entry per query of the chain and one more")
        if n > 0 and np.all(np.diff(uptr) >= 0) and uptr[0] == 0 and uidx.size < uptr[-1]:
            raise GorseHipError(ERR_INVALID, "fewer entries than the pointer array names")
        ul = _arr(user_lead, np.int32).reshape(-1) if user_lead is not None else None
        if ul is not None and ul.size != n:
            raise GorseHipError(ERR_INVALID, "one lead per user")
        sc = np.zeros(total, np.float32) if scores else None
        fn = np.zeros(total, np.float64) if final else None
        od = np.zeros(total, np.int32) if order else None
        check(lib().gorse_fm_rank_cand_decayed(self.h, chain.h, _p(uptr, _i64p), _p(uidx, _i32p), _p(uval, _f32p), _p(ul, _i32p),
                                               int(batch_size), _p(cancel, _i32p) if cancel is not None else None, float(positive_decay),
                                               float(read_decay), _p(sc, _f32p), _p(fn, _f64p), _p(od, _i32p)))
        return sc, fn, od

    def rank_stats(self):
        """the last rank_users / rank_cand / rank_cand_decayed: rows scored, slices, launch rounds, lists sorted by the host, device milliseconds"""
        v = [C.c_int64(0) for _ in range(4)]
        ms = C.c_double(0)
        check(lib().gorse_fm_rank_stats(self.h, *[C.byref(x) for x in v], C.byref(ms)))
        return dict(rows=v[0].value, slices=v[1].value, rounds=v[2].value, host_sorted=v[3].value, device_ms=ms.value)

    def set_test(self, indices, values, target, embs=()):
        """the resident test split of evaluate: n x width indices / values, one target per row (> 0: a positive) and one
        n x D uint16 (bf16) matrix per field.  No rows (n = 0) drops the split."""
        idx, val = self._rows(indices, values)
        tgt = _arr(target, np.float32).reshape(-1)
        n = idx.shape[0]
        if tgt.size != n:
            raise GorseHipError(ERR_INVALID, "one target per row")
        embs = [_arr(e, np.uint16) for e in embs]
        if n > 0 and (len(embs) != len(self.dims) or any(e.shape != (n, D) for e, D in zip(embs, self.dims))):
            raise GorseHipError(ERR_INVALID, "one n x D embedding matrix per field")
        ptrs = (C.POINTER(C.c_uint16) * max(1, len(embs)))(*[_p(e, C.POINTER(C.c_uint16)) for e in embs])
        check(lib().gorse_fm_set_test(self.h, n, max(1, idx.shape[1]), _p(idx, _i32p), _p(val, _f32p), _p(tgt, _f32p),
                                      ptrs if embs else None))
        self._n_test = n

    @staticmethod
    def _samples(user_indptr, user_indices, user_values, user_lead, user, item, target):
        uptr = _arr(user_indptr, np.int64).reshape(-1)
        nu = uptr.size - 1
        uidx, uval = _arr(user_indices, np.int32).reshape(-1), _arr(user_values, np.float32).reshape(-1)
        if nu < 0 or uidx.size != uval.size:
            raise GorseHipError(ERR_INVALID, "user_indptr holds n_users + 1 entries, user_indices and user_values one per entry")
        # the library reads indptr[-1] entries: only a well-formed pointer array may be trusted with that
        if nu > 0 and np.all(np.diff(uptr) >= 0) and uptr[0] == 0 and uidx.size < uptr[-1]:
            raise GorseHipError(ERR_INVALID, "fewer entries than the pointer array names")
        ul = _arr(user_lead, np.int32).reshape(-1) if user_lead is not None else None
        if ul is not None and ul.size != nu:
            raise GorseHipError(ERR_INVALID, "one lead per user")
        us, it = _arr(user, np.int32).reshape(-1), _arr(item, np.int32).reshape(-1)
        tgt = _arr(target, np.float32).reshape(-1)
        if us.size != it.size or us.size != tgt.size:
            raise GorseHipError(ERR_INVALID, "one user, one item and one target per sample")
        keep = (uptr, uidx, uval, ul, us, it, tgt)
        return keep, (max(nu, 0), _p(uptr, _i64p), _p(uidx, _i32p), _p(uval, _f32p), _p(ul, _i32p), us.size, _p(us, _i32p),
                      _p(it, _i32p), _p(tgt, _f32p))

    def set_train_samples(self, user_indptr, user_indices, user_values, user, item, target, user_lead=None):
        """the training set in sample form: the users' feature rows as a CSR (as rank_users takes them) and per sample
        (user, item, target); sample i is the row rank_users composes for user[i] and catalogue row item[i] (set_items), its
        embeddings are the catalogue's.  Replaces a set_train set, and the other way round."""
        keep, args = self._samples(user_indptr, user_indices, user_values, user_lead, user, item, target)
        check(lib().gorse_fm_set_train_samples(self.h, *args))

    def set_test_samples(self, user_indptr, user_indices, user_values, user, item, target, user_lead=None):
        """the resident test split of evaluate in sample form (see set_train_samples).  No samples drops the split."""
        keep, args = self._samples(user_indptr, user_indices, user_values, user_lead, user, item, target)
        check(lib().gorse_fm_set_test_samples(self.h, *args))
        self._n_test = args[5]

    def evaluate(self, batch_size, cancel=None, logits=False):
        """(counts, auc_sum) of the resident split, or (counts, auc_sum, logits) with the logits in the rows' given order.
        counts: dict of n_pos, n_neg, pos_above (positives with logit > 0), neg_above, neg_below, nan, pairs_less."""
        cnt = np.zeros(7, np.int64)
        s = np.zeros(1, np.float32)
        out = np.zeros(max(1, getattr(self, "_n_test", 0)), np.float32) if logits else None
        check(lib().gorse_fm_evaluate(self.h, int(batch_size), _p(cancel, _i32p) if cancel is not None else None, _p(cnt, _i64p),
                                      _p(s, _f32p), _p(out, _f32p)))
        counts = dict(zip(EVAL_COUNTS, (int(x) for x in cnt)))
        return (counts, s[0], out[:getattr(self, "_n_test", 0)]) if logits else (counts, s[0])

    def evaluate_stats(self):
        """the last evaluate: rows scored, slices, launch rounds, device milliseconds"""
        v = [C.c_int64(0) for _ in range(3)]
        ms = C.c_double(0)
        check(lib().gorse_fm_evaluate_stats(self.h, *[C.byref(x) for x in v], C.byref(ms)))
        return dict(rows=v[0].value, slices=v[1].value, rounds=v[2].value, device_ms=ms.value)

    def close(self):
        if getattr(self, "h", None):
            lib().gorse_fm_destroy(self.h)
            self.h = None

    __del__ = close

    def set_params(self, B, W, V):
        W = _arr(W, np.float32).reshape(-1)
        V = _arr(V, np.float32).reshape(-1)
        if W.size != self.nf or V.size != self.nf * self.d:
            raise GorseHipError(ERR_INVALID, "W must hold n_features and V n_features x d values")
        check(lib().gorse_fm_set_params(self.h, float(B), _p(W, _f32p), _p(V, _f32p)))

    def get_params(self):
        B = np.zeros(1, np.float32)
        W = np.empty(self.nf, np.float32)
        V = np.empty((self.nf, self.d), np.float32)
        check(lib().gorse_fm_get_params(self.h, _p(B, _f32p), _p(W, _f32p), _p(V, _f32p)))
        return B[0], W, V

    @staticmethod
    def _rows(indices, values):
        idx, val = _arr(indices, np.int32), _arr(values, np.float32)
        if idx.ndim != 2 or idx.shape != val.shape:
            raise GorseHipError(ERR_INVALID, "indices and values must be n x width matrices of one shape")
        return idx, val

    def set_train(self, indices, values, target):
        idx, val = self._rows(indices, values)
        tgt = _arr(target, np.float32)
        if tgt.size != idx.shape[0]:
            raise GorseHipError(ERR_INVALID, "one target per row")
        check(lib().gorse_fm_set_train(self.h, idx.shape[0], idx.shape[1], _p(idx, _i32p), _p(val, _f32p), _p(tgt, _f32p)))

    def epoch(self, batch_size, optimizer, lr, wd, cancel=None):
        """one epoch over the training set; returns the cost (sum of the batches' mean losses)"""
        cost = C.c_float(0)
        check(lib().gorse_fm_epoch(self.h, batch_size, optimizer, lr, wd, _p(cancel, _i32p) if cancel is not None else None,
                                   C.byref(cost)))
        return cost.value

    def predict(self, indices, values):
        idx, val = self._rows(indices, values)
        out = np.empty(idx.shape[0], np.float32)
        check(lib().gorse_fm_predict(self.h, idx.shape[0], idx.shape[1], _p(idx, _i32p), _p(val, _f32p), _p(out, _f32p)))
        return out


class TopK:
    """One gorse_topk handle (exact brute-force index resident on one GPU)."""

    def __init__(self, X, metric, dtype=DTYPE_F32, device=0):
        X = _arr(X, np.uint16 if dtype == DTYPE_BF16 else np.float32)
        if X.ndim != 2:
            raise GorseHipError(ERR_INVALID, "X must be N x d")
        self.N, self.d = X.shape
        self.dtype, self.metric = dtype, metric
        self.h = _vp()
        check(lib().gorse_topk_create(C.byref(self.h), device, self.N, self.d, dtype, metric, X.ctypes.data_as(_vp)))

    def close(self):
        if getattr(self, "h", None):
            lib().gorse_topk_destroy(self.h)
            self.h = None

    __del__ = close

    def _out(self, nq, k):
        return np.empty((nq, k), np.int32), np.empty((nq, k), np.float32), np.empty(nq, np.int32)

    def search_index(self, q, k, prune0=False):
        q = _arr(np.atleast_1d(q), np.int64)
        idx, dist, cnt = self._out(q.size, k)
        check(lib().gorse_topk_search_index(self.h, _p(q, _i64p), q.size, k, int(prune0), _p(idx, _i32p),
                                            _p(dist, _f32p), _p(cnt, _i32p)))
        return idx, dist, cnt

    def search_vector(self, qv, k, prune0=False):
        qv = _arr(np.atleast_2d(qv), np.uint16 if self.dtype == DTYPE_BF16 else np.float32)
        if qv.shape[1] != self.d:
            raise GorseHipError(ERR_INVALID, "query dimension mismatch")
        idx, dist, cnt = self._out(qv.shape[0], k)
        check(lib().gorse_topk_search_vector(self.h, qv.ctypes.data_as(_vp), qv.shape[0], k, int(prune0),
                                             _p(idx, _i32p), _p(dist, _f32p), _p(cnt, _i32p)))
        return idx, dist, cnt

    def all_pairs(self, k, q_begin=0, q_end=None, fetch=True):
        q_end = self.N if q_end is None else q_end
        nq = q_end - q_begin
        idx = np.empty((nq, k), np.int32) if fetch else None
        dist = np.empty((nq, k), np.float32) if fetch else None
        check(lib().gorse_topk_all_pairs(self.h, q_begin, q_end, k, _p(idx, _i32p), _p(dist, _f32p)))
        return idx, dist

    # ---- the triangle-sharded all-pairs search (include/gorse_hip.h, gorse_topk_tri_*): host-memory forms of the messages ----
    def tri_begin(self, k, rank, world, q_begin=0, q_end=None):
        q_end = self.N if q_end is None else q_end
        self._tri = (k, q_end - q_begin)
        check(lib().gorse_topk_tri_begin(self.h, q_begin, q_end, k, rank, world))

    def tri_slice(self, rank):
        """(lo, hi, owned): the queries whose pilots `rank` runs, and how many queries it owns"""
        lo, hi, ow = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(lib().gorse_topk_tri_slice(self.h, rank, C.byref(lo), C.byref(hi), C.byref(ow)))
        return lo.value, hi.value, ow.value

    def tri_thresholds_get(self, lo, hi):
        out = np.empty(hi - lo, np.float32)
        check(lib().gorse_topk_tri_thresholds_get(self.h, lo, hi, out.ctypes.data_as(_vp)))
        return out

    def tri_thresholds_put(self, lo, hi, thr):
        thr = _arr(thr, np.float32)
        assert thr.size == hi - lo
        check(lib().gorse_topk_tri_thresholds_put(self.h, lo, hi, thr.ctypes.data_as(_vp)))

    def tri_sweep(self):
        check(lib().gorse_topk_tri_sweep(self.h))

    def tri_pack_device(self, dest):
        """builds the message for `dest` in the handle's device buffers; returns (number of counts, number of entries)"""
        nc, ne = C.c_int64(0), C.c_int64(0)
        check(lib().gorse_topk_tri_pack(self.h, dest, C.byref(nc), C.byref(ne)))
        return nc.value, ne.value

    def tri_pack_fetch(self, nc, ne):
        counts, entries = np.empty(nc, np.int32), np.empty(ne, np.uint64)
        check(lib().gorse_topk_tri_pack_read(self.h, counts.ctypes.data_as(_vp), entries.ctypes.data_as(_vp)))
        return counts, entries

    def tri_pack(self, dest):
        """the message for `dest`: (counts int32 per query dest owns, entries uint64 = (key, row) pairs end to end)"""
        return self.tri_pack_fetch(*self.tri_pack_device(dest))

    def tri_unpack(self, src, counts, entries):
        counts, entries = _arr(counts, np.int32), _arr(entries, np.uint64)
        check(lib().gorse_topk_tri_unpack(self.h, src, counts.ctypes.data_as(_vp), counts.size, entries.ctypes.data_as(_vp), entries.size))

    # device-pointer forms (the messages stay on the GPU: torch tensors' data_ptr(); gorse_amd.dist.HipTriEngine(device="cuda"))
    def tri_thresholds_get_ptr(self, lo, hi, ptr):
        check(lib().gorse_topk_tri_thresholds_get(self.h, lo, hi, _vp(ptr)))

    def tri_thresholds_put_ptr(self, lo, hi, ptr):
        check(lib().gorse_topk_tri_thresholds_put(self.h, lo, hi, _vp(ptr)))

    def tri_pack_read_ptr(self, counts_ptr, entries_ptr):
        check(lib().gorse_topk_tri_pack_read(self.h, _vp(counts_ptr), _vp(entries_ptr)))

    def tri_unpack_ptr(self, src, counts_ptr, n_counts, entries_ptr, n_entries):
        check(lib().gorse_topk_tri_unpack(self.h, src, _vp(counts_ptr), n_counts, _vp(entries_ptr), n_entries))

    def tri_finish(self, idx=None, dist=None, fetch=True):
        """rescoring + tie path of the queries this rank owns; with fetch their rows are written into idx / dist (nq x k, allocated
        here when not given: the rows of other ranks' queries are then -1 / +inf)"""
        k, nq = self._tri
        if fetch and idx is None:
            idx, dist = np.full((nq, k), -1, np.int32), np.full((nq, k), np.inf, np.float32)
        check(lib().gorse_topk_tri_finish(self.h, _p(idx, _i32p) if fetch else None, _p(dist, _f32p) if fetch else None))
        return idx, dist

    def set_mask(self, admissible=None):
        m = None if admissible is None else _arr(admissible, np.uint8)
        if m is not None and m.size != self.N:
            raise GorseHipError(ERR_INVALID, "mask must have N entries")
        check(lib().gorse_topk_set_mask(self.h, None if m is None else m.ctypes.data_as(_vp)))

    def resweeps(self):
        n = C.c_int64(0)
        check(lib().gorse_hip_test_topk_resweeps(self.h, C.byref(n)))
        return n.value

    def warm_thresholds(self, n):
        out = np.empty(n, np.float32)
        check(lib().gorse_hip_test_topk_get_thresholds(self.h, out.ctypes.data_as(_f32p), n))
        return out

    def last_flags(self, n):
        """per-query flags of the last MFMA search's last chunk behind the rescoring (non-zero: the query took the tie path)"""
        f = np.empty(n, np.uint8)
        check(lib().gorse_hip_test_topk_get_flags(self.h, f.ctypes.data_as(C.POINTER(C.c_uint8)), n))
        return f

    def scan_flags(self, n):
        """flags of the last scan block of the last call (1: select_fast_kernel left the query to the literal kernel or the reroute)"""
        f = np.empty(n, np.int32)
        check(lib().gorse_hip_test_topk_scan_flags(self.h, _p(f, _i32p), n))
        return f

    def foreign_counts(self, n):
        """entries appended to each query's foreign list by the last symmetric sweep (> 512: the list overflowed)"""
        c = np.empty(n, np.int32)
        check(lib().gorse_hip_test_topk_get_foreign_counts(self.h, c.ctypes.data_as(_i32p), n))
        return c

    def sym_stats(self):
        out = (C.c_uint64 * 4)()
        check(lib().gorse_hip_test_topk_sym_stats(self.h, out))
        return [int(x) for x in out]

    def last_symmetric(self):
        s = C.c_int32(0)
        check(lib().gorse_hip_test_topk_last_symmetric(self.h, C.byref(s)))
        return bool(s.value)

    def synchronize(self):
        check(lib().gorse_topk_synchronize(self.h))

    def set_profiling(self, on):
        check(lib().gorse_topk_set_profiling(self.h, int(bool(on))))

    def get_profile(self, cls):
        n, ms = C.c_int64(0), C.c_double(0)
        check(lib().gorse_topk_get_profile(self.h, cls, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def sweep_profile(self):
        out = (C.c_uint64 * 16)()
        check(lib().gorse_hip_test_get_sweep_profile(self.h, out))
        return [int(x) for x in out]

    def last_stats(self):
        a, b = C.c_int64(0), C.c_int64(0)
        check(lib().gorse_topk_last_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value


def topk_tri_all_pairs_local(handles, k, q_begin=0, q_end=None, fetch=True):
    """gorse_topk_tri_all_pairs_local: the triangle-sharded all-pairs search over the TopK handles of ONE process (handles[r] = rank r)"""
    q_end = handles[0].N if q_end is None else q_end
    nq = q_end - q_begin
    hs = (_vp * len(handles))(*[h.h for h in handles])
    idx = np.empty((nq, k), np.int32) if fetch else None
    dist = np.empty((nq, k), np.float32) if fetch else None
    check(lib().gorse_topk_tri_all_pairs_local(hs, len(handles), q_begin, q_end, k, _p(idx, _i32p), _p(dist, _f32p)))
    return idx, dist


class Comm:
    """One rank of an RCCL communicator owned by the library (gorse_comm_*): Comm.unique_id() on rank 0, the bytes shipped
    to every rank by the caller, Comm(id, world, rank, device) everywhere; Comm.local(devices) = all ranks in this process."""

    def __init__(self, uid=None, world=1, rank=0, device=0, _handle=None):
        if _handle is not None:
            self.h = _handle
        else:
            buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(uid))
            self.h = _vp()
            check(lib().gorse_comm_create(C.byref(self.h), C.cast(buf, _vp), world, rank, device))
        w, r = C.c_int32(0), C.c_int32(0)
        check(lib().gorse_comm_info(self.h, C.byref(w), C.byref(r)))
        self.world, self.rank = w.value, r.value

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        check(lib().gorse_comm_unique_id(C.cast(buf, _vp)))
        return bytes(buf)

    @staticmethod
    def local(devices):
        devs = _arr(devices, np.int32)
        out = (_vp * devs.size)()
        check(lib().gorse_comm_create_local(out, _p(devs, _i32p), devs.size))
        return [Comm(_handle=_vp(out[i])) for i in range(devs.size)]

    def close(self):
        if getattr(self, "h", None):
            lib().gorse_comm_destroy(self.h)
            self.h = None

    __del__ = close

    def allreduce_f32(self, values):
        a = np.array(values, dtype=np.float32)
        check(lib().gorse_comm_allreduce_f32(self.h, _p(a, _f32p), a.size))
        return a


def comm_available():
    """None when RCCL can be opened in this process, else the reason"""
    if lib().gorse_comm_available() == 0:
        return None
    return lib().gorse_hip_last_error().decode()


def allreduce_f32_local(comms, arrays):
    """gorse_comm_allreduce_f32_local: one array of equal length per communicator of this process, summed in place"""
    arrs = [np.ascontiguousarray(a, np.float32) for a in arrays]
    cs = (_vp * len(comms))(*[c.h for c in comms])
    bs = (_f32p * len(arrs))(*[_p(a, _f32p) for a in arrs])
    check(lib().gorse_comm_allreduce_f32_local(cs, len(comms), bs, arrs[0].size))
    return arrs


def _pairs(mfs, comms):
    n = len(mfs)
    hs, cs = (_vp * n)(*[m.h for m in mfs]), (_vp * n)(*[c.h for c in comms])
    return hs, cs, n


def item_allreduce(mfs, comms):
    """gorse_mf_item_allreduce over this process's (handle, communicator) pairs"""
    hs, cs, n = _pairs(mfs, comms)
    check(lib().gorse_mf_item_allreduce(hs, cs, n))


def rows_allgather(mfs, comms, side, row_splits):
    hs, cs, n = _pairs(mfs, comms)
    sp = _arr(row_splits, np.int64)
    check(lib().gorse_mf_rows_allgather(hs, cs, n, side, _p(sp, _i64p)))


class Sparse:
    """One gorse_sparse handle: N sparse vectors (CSR, strictly ascending indices per row) resident on one GPU."""

    def __init__(self, indptr, indices, values, device=0):
        self.indptr = _arr(indptr, np.int64)
        self.indices = _arr(indices, np.uint32)
        self.values = _arr(values, np.float32)
        self.N = self.indptr.size - 1
        self.h = _vp()
        check(lib().gorse_sparse_create(C.byref(self.h), device, self.N, _p(self.indptr, _i64p),
                                        self.indices.ctypes.data_as(_vp), _p(self.values, _f32p)))

    def close(self):
        if getattr(self, "h", None):
            lib().gorse_sparse_destroy(self.h)
            self.h = None

    __del__ = close

    def set_mask(self, admissible=None):
        m = None if admissible is None else _arr(admissible, np.uint8)
        if m is not None and m.size != self.N:
            raise GorseHipError(ERR_INVALID, "mask must have N entries")
        check(lib().gorse_sparse_set_mask(self.h, None if m is None else m.ctypes.data_as(_vp)))

    def search(self, q_indptr, q_indices, q_values, k, exclude=None):
        qp = _arr(q_indptr, np.int64)
        qi = _arr(q_indices, np.uint32)
        qv = _arr(q_values, np.float32)
        nq = qp.size - 1
        ex = None if exclude is None else _arr(exclude, np.int64)
        idx, sc, cnt = np.empty((nq, k), np.int32), np.empty((nq, k), np.float32), np.empty(nq, np.int32)
        check(lib().gorse_sparse_search(self.h, nq, _p(qp, _i64p), qi.ctypes.data_as(_vp), _p(qv, _f32p), _p(ex, _i64p), k,
                                        _p(idx, _i32p), _p(sc, _f32p), _p(cnt, _i32p)))
        return idx, sc, cnt

    def all_pairs(self, k, q_begin=0, q_end=None, exclude_self=True, fetch=True):
        q_end = self.N if q_end is None else q_end
        nq = q_end - q_begin
        idx = np.empty((nq, k), np.int32) if fetch else None
        sc = np.empty((nq, k), np.float32) if fetch else None
        cnt = np.empty(nq, np.int32) if fetch else None
        check(lib().gorse_sparse_all_pairs(self.h, q_begin, q_end, k, int(bool(exclude_self)), _p(idx, _i32p),
                                           _p(sc, _f32p), _p(cnt, _i32p)))
        return idx, sc, cnt

    def synchronize(self):
        check(lib().gorse_sparse_synchronize(self.h))

    def set_profiling(self, on):
        check(lib().gorse_sparse_set_profiling(self.h, int(bool(on))))

    def get_profile(self):
        n, ms = C.c_int64(0), C.c_double(0)
        check(lib().gorse_sparse_get_profile(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def last_stats(self):
        a, b = C.c_int64(0), C.c_int64(0)
        check(lib().gorse_sparse_last_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def sym_stats(self):
        """the last call: (ran in symmetric form, rows redone after a foreign list overflowed, foreign entries ranked, longest foreign list)"""
        out = (C.c_int64 * 4)()
        lib().gorse_hip_test_sparse_sym_stats(self.h, out)
        return tuple(int(x) for x in out)

    def path_stats(self):
        """the last call: (launch rounds, heavy queries over the rounds); the handle: (row ranges of the heavy-query kernel, directory cells)"""
        out = (C.c_int64 * 4)()
        lib().gorse_hip_test_sparse_path_stats(self.h, out)
        return tuple(int(x) for x in out)


NBR_HOP1, NBR_HOP2 = 0, 1
NBR_RAW, NBR_RECIP = 0, 1
NBR_MAX_K = 256  # GORSE_NBR_MAX_K


def set_nbr(lds_slots=0, query_chunk=0):
    """gorse_hip_test_set_nbr: slots of the largest LDS table and queries per launch of the calls that follow (0 = the library's)"""
    lib().gorse_hip_test_set_nbr(int(lds_slots), int(query_chunk))


class NbrRecommender:
    """One gorse_nbr handle: the two neighbour tables of an item-to-item or user-to-user recommender resident on one GPU."""

    def __init__(self, n_items, device=0):
        self.n_items = int(n_items)
        self.h = _vp()
        check(lib().gorse_nbr_create(C.byref(self.h), device, self.n_items))

    def close(self):
        if getattr(self, "h", None):
            lib().gorse_nbr_destroy(self.h)
            self.h = None

    __del__ = close

    def set_table(self, which, indptr, indices, weights=None, transform=NBR_RAW, scale=1.0):
        """a CSR of len(indptr) - 1 rows; weights = None: every weight is 1.0"""
        ip, ix = _arr(indptr, np.int64), _arr(indices, np.int32)
        w = _arr(weights, np.float32) if weights is not None else None
        if ip.size < 1 or (w is not None and w.size != ix.size):
            raise GorseHipError(ERR_INVALID, "indptr must have n_rows + 1 entries and weights one per index")
        if ix.size == 0:
            ix = np.zeros(1, np.int32)
            w = np.zeros(1, np.float32) if w is not None else None
        check(lib().gorse_nbr_set_table(self.h, which, ip.size - 1, _p(ip, _i64p), _p(ix, _i32p), _p(w, _f32p), transform, scale))

    def _set_table_from(self, fn, which, index, sources, n_rows, n, positive_only, transform, scale):
        src = _arr(sources, np.int64) if sources is not None else None
        if src is not None:
            n_rows = src.size
            if src.size == 0:
                src = np.zeros(1, np.int64)
        check(fn(self.h, which, getattr(index, "h", index), int(n_rows), _p(src, _i64p), int(n), int(bool(positive_only)), transform, scale))

    def set_table_from_topk(self, which, index, n, sources=None, n_rows=None, positive_only=False, transform=NBR_RAW, scale=1.0):
        """the neighbour lists of a TopK index's rows, built on the device (gorse_nbr_set_table_from_topk): row r = the list of
        stored row sources[r] (None: the index's first n_rows rows, all of them by default)"""
        if sources is None and n_rows is None:
            n_rows = index.N
        self._set_table_from(lib().gorse_nbr_set_table_from_topk, which, index, sources, n_rows, n, positive_only, transform, scale)

    def set_table_from_sparse(self, which, index, n, sources=None, n_rows=None, positive_only=False, transform=NBR_RAW, scale=1.0):
        """the same from a Sparse index (gorse_nbr_set_table_from_sparse)"""
        if sources is None and n_rows is None:
            n_rows = index.N
        self._set_table_from(lib().gorse_nbr_set_table_from_sparse, which, index, sources, n_rows, n, positive_only, transform, scale)

    def table_info(self, which):
        """(rows, entries, weighted) of the table a slot holds (gorse_nbr_table_info)"""
        nr, nz, w = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        check(lib().gorse_nbr_table_info(self.h, which, C.byref(nr), C.byref(nz), C.byref(w)))
        return nr.value, nz.value, bool(w.value)

    def get_table(self, which):
        """(indptr, indices, weights or None) of the table a slot holds, host-built or device-built (gorse_nbr_get_table)"""
        nr, nz, weighted = self.table_info(which)
        ip, ix = np.zeros(nr + 1, np.int64), np.zeros(max(nz, 1), np.int32)
        w = np.zeros(max(nz, 1), np.float32) if weighted else None
        check(lib().gorse_nbr_get_table(self.h, which, _p(ip, _i64p), _p(ix, _i32p), _p(w, _f32p)))
        return ip, ix[:nz], (w[:nz] if weighted else None)

    def recommend(self, rows, k, seen_indptr=None, seen_items=None, out=None):
        """every query's k best candidates (gorse_nbr_recommend): (items n x k padded with -1, float64 sums n x k padded with 0,
        counts n).  rows = an int n: the first n hop-1 rows; seen rows are per QUERY.  out = the three arrays to fill."""
        if isinstance(rows, (int, np.integer)):
            n, rp = int(rows), None
        else:
            rp = _arr(rows, np.int32)
            n = rp.size
        sp = _arr(seen_indptr, np.int64) if seen_indptr is not None else None
        if sp is not None and sp.size != n + 1:
            raise GorseHipError(ERR_INVALID, "seen_indptr must have n_queries + 1 entries")
        si = _arr(seen_items, np.int32) if seen_items is not None else None
        if si is not None and si.size == 0:
            si = np.zeros(1, np.int32)
        kk = max(int(k), 0)
        if out is None:
            out = (np.full((n, kk), -2, np.int32), np.full((n, kk), np.nan, np.float64), np.full(n, -2, np.int32))
        items, sums, counts = out
        assert items.dtype == np.int32 and sums.dtype == np.float64 and counts.dtype == np.int32
        assert items.size >= n * kk and sums.size >= n * kk and counts.size >= n
        check(lib().gorse_nbr_recommend(self.h, n, _p(rp, _i32p), k, _p(sp, _i64p), _p(si, _i32p), _p(items, _i32p), _p(sums, _f64p),
                                        _p(counts, _i32p)))
        return items, sums, counts

    def recommend_stats(self):
        """the last recommend(): (queries answered over an LDS table, over a table in global scratch, device milliseconds)"""
        nl, ng, ms = C.c_int64(0), C.c_int64(0), C.c_double(0)
        check(lib().gorse_nbr_recommend_stats(self.h, C.byref(nl), C.byref(ng), C.byref(ms)))
        return nl.value, ng.value, ms.value


CAND_MAX_K, CAND_MAX_STAGES = 256, 255  # GORSE_CAND_MAX_K, GORSE_CAND_MAX_STAGES
CAND_STAGE_REPLACEMENT, CAND_KIND_POSITIVE, CAND_KIND_READ = 255, 1, 2  # GORSE_CAND_STAGE_REPLACEMENT, GORSE_CAND_KIND_*


class CandidateChain:
    """One gorse_cand handle: the exclusion rows and candidate rows of one offline pass (RecommendSequential for many users)
    resident on one GPU.  begin, then add_* in the recommenders' order, then finish; get / FM.rank_cand need a finished pass."""

    def __init__(self, n_items, device=0):
        self.n_items = int(n_items)
        self.h = _vp()
        check(lib().gorse_cand_create(C.byref(self.h), device, self.n_items))

    def close(self):
        if getattr(self, "h", None):
            lib().gorse_cand_destroy(self.h)
            self.h = None

    __del__ = close

    def _keep(self, keep):
        if keep is None:
            return None
        kp = _arr(keep, np.uint8).reshape(-1)
        if kp.size != self.n_items:
            raise GorseHipError(ERR_INVALID, "keep must have n_items entries")
        return kp

    @staticmethod
    def _csr(indptr, n, *arrays):
        """a host CSR the library may read to indptr[-1]: only a well-formed pointer array is trusted with that"""
        ip = _arr(indptr, np.int64).reshape(-1)
        if ip.size != n + 1:
            raise GorseHipError(ERR_INVALID, "a row pointer must have n_queries + 1 entries")
        if ip[0] == 0 and np.all(np.diff(ip) >= 0) and any(a.size < ip[-1] for a in arrays):
            raise GorseHipError(ERR_INVALID, "fewer entries than the pointer array names")
        return ip

    def begin(self, n_queries, capacity, excl_indptr=None, excl_items=None):
        """starts a pass of n_queries queries whose candidate rows hold `capacity` entries; the base exclusion rows as a CSR"""
        n = int(n_queries)
        it = _arr(excl_items if excl_items is not None else [], np.int32).reshape(-1)
        ip = self._csr(excl_indptr, n, it) if excl_indptr is not None and n >= 0 else None
        if it.size == 0:
            it = np.zeros(1, np.int32)
        check(lib().gorse_cand_begin(self.h, n, _p(ip, _i64p), _p(it, _i32p), int(capacity)))

    def _queries(self, ids):
        if ids is None:
            return None
        a = _arr(ids, np.int32).reshape(-1)
        if a.size != self.info()[0]:
            raise GorseHipError(ERR_INVALID, "one user / row per query of the pass")
        return a if a.size else np.zeros(1, np.int32)

    def add_mf(self, mf, users, k, item_ok=None, keep=None):
        """MF.recommend(users, k, item_ok, seen = the BASE rows) as a stage (users = None: query t is user t)"""
        ok = _arr(item_ok, np.uint8).reshape(-1) if item_ok is not None else None
        if ok is not None and ok.size != self.n_items:
            raise GorseHipError(ERR_INVALID, "item_ok must have n_items entries")
        check(lib().gorse_cand_add_mf(self.h, mf.h, _p(self._queries(users), _i32p), int(k), _p(ok, _u8p), _p(self._keep(keep), _u8p)))

    def add_nbr(self, nbr, rows, k, keep=None):
        """NbrRecommender.recommend(rows, k, seen = the CURRENT rows) as a stage (rows = None: query t walks hop-1 row t)"""
        check(lib().gorse_cand_add_nbr(self.h, nbr.h, _p(self._queries(rows), _i32p), int(k), _p(self._keep(keep), _u8p)))

    def add_shared(self, items, scores, k, keep=None):
        """one list for every query (latest, non-personalized)"""
        it, sc = _arr(items, np.int32).reshape(-1), _arr(scores, np.float64).reshape(-1)
        if it.size != sc.size:
            raise GorseHipError(ERR_INVALID, "one score per item")
        n = it.size
        if n == 0:
            it, sc = np.zeros(1, np.int32), np.zeros(1, np.float64)
        check(lib().gorse_cand_add_shared(self.h, n, _p(it, _i32p), _p(sc, _f64p), int(k), _p(self._keep(keep), _u8p)))

    def add_lists(self, indptr, items, scores, k, keep=None):
        """one list per query, as a CSR"""
        it, sc = _arr(items, np.int32).reshape(-1), _arr(scores, np.float64).reshape(-1)
        if it.size != sc.size:
            raise GorseHipError(ERR_INVALID, "one score per item")
        ip = self._csr(indptr, self.info()[0], it)
        if it.size == 0:
            it, sc = np.zeros(1, np.int32), np.zeros(1, np.float64)
        check(lib().gorse_cand_add_lists(self.h, _p(ip, _i64p), _p(it, _i32p), _p(sc, _f64p), int(k), _p(self._keep(keep), _u8p)))

    def finish(self, keep=None):
        """compacts the candidates (dropping items with keep == 0) and closes the pass"""
        check(lib().gorse_cand_finish(self.h, _p(self._keep(keep), _u8p)))

    def info(self):
        """(queries, stages so far, candidates, current exclusion entries)"""
        nq, ns, nc, nx = C.c_int64(0), C.c_int32(0), C.c_int64(0), C.c_int64(0)
        check(lib().gorse_cand_info(self.h, C.byref(nq), C.byref(ns), C.byref(nc), C.byref(nx)))
        return nq.value, ns.value, nc.value, nx.value

    def get(self):
        """the finished pass as a CSR: (indptr, items, float64 scores, uint8 stage numbers)"""
        nq, _, nc, _ = self.info()
        ip = np.zeros(nq + 1, np.int64)
        it, sc, sg = np.zeros(max(nc, 1), np.int32), np.zeros(max(nc, 1), np.float64), np.zeros(max(nc, 1), np.uint8)
        check(lib().gorse_cand_get(self.h, _p(ip, _i64p), _p(it, _i32p), _p(sc, _f64p), _p(sg, _u8p)))
        n = int(ip[-1])
        return ip, it[:n], sc[:n], sg[:n]

    def exclusion(self):
        """the current exclusion rows as a CSR with ascending rows: (indptr, items)"""
        nq, _, _, nx = self.info()
        ip, it = np.zeros(nq + 1, np.int64), np.zeros(max(nx, 1), np.int32)
        check(lib().gorse_cand_get_exclusion(self.h, _p(ip, _i64p), _p(it, _i32p)))
        return ip, it[:nx]

    def stats(self, stage):
        """(device milliseconds of the stage's own search, of the chain's filter / scan / append / merge)"""
        a, b = C.c_double(0), C.c_double(0)
        check(lib().gorse_cand_stats(self.h, int(stage), C.byref(a), C.byref(b)))
        return a.value, b.value

    def add_replacement(self, hist_indptr, hist_items, hist_kind, keep=None):
        """the users' historical items back among the finished candidates (gorse_cand_add_replacement): one history row per query as a
        CSR, a kind per entry (KIND_POSITIVE / KIND_READ); keep = the items that exist and are not hidden"""
        it, kd = _arr(hist_items, np.int32).reshape(-1), _arr(hist_kind, np.uint8).reshape(-1)
        if it.size != kd.size:
            raise GorseHipError(ERR_INVALID, "one kind per history entry")
        ip = self._csr(hist_indptr, self.info()[0], it)
        if it.size == 0:
            it, kd = np.zeros(1, np.int32), np.ones(1, np.uint8)
        check(lib().gorse_cand_add_replacement(self.h, _p(ip, _i64p), _p(it, _i32p), _p(kd, _u8p), _p(self._keep(keep), _u8p)))

    def replacement(self):
        """the pass's replacement rows as a CSR with ascending rows: (indptr, items, uint8 kinds)"""
        nq = self.info()[0]
        ip = np.zeros(nq + 1, np.int64)
        check(lib().gorse_cand_get_replacement(self.h, _p(ip, _i64p), None, None))
        n = int(ip[-1])
        it, kd = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
        check(lib().gorse_cand_get_replacement(self.h, None, _p(it, _i32p), _p(kd, _u8p)))
        return ip, it[:n], kd[:n]

    def replacement_stats(self):
        """(entries appended, positive entries and read entries of the replacement rows, device milliseconds)"""
        v = [C.c_int64(0) for _ in range(3)]
        ms = C.c_double(0)
        check(lib().gorse_cand_replacement_stats(self.h, *[C.byref(x) for x in v], C.byref(ms)))
        return v[0].value, v[1].value, v[2].value, ms.value


# gorse_hip_test_sgemm_last_form (include/gorse_hip_test.h, GORSE_TEST_SGEMM_*)
SGEMM_NONE, SGEMM_NT, SGEMM_VALU, SGEMM_MFMA64, SGEMM_MFMA128 = range(5)
SGEMM_IN_PLACE, SGEMM_NT_LONG = 0x100, 0x200


def sgemm(transA, transB, m, n, k, a, lda, b, ldb, c, ldc, device=0):
    a, b = _arr(a, np.float32), _arr(b, np.float32)
    c = np.array(c, dtype=np.float32, order="C")
    check(lib().gorse_hip_sgemm(device, int(transA), int(transB), m, n, k, _p(a, _f32p), lda, _p(b, _f32p), ldb,
                                _p(c, _f32p), ldc))
    return c


def sgemm_device(transA, transB, m, n, k, a_ptr, lda, b_ptr, ldb, c_ptr, ldc, device=0):
    """gorse_hip_sgemm_device: the operands are device addresses (e.g. torch tensors' data_ptr()); C is updated in place"""
    check(lib().gorse_hip_sgemm_device(device, int(transA), int(transB), m, n, k, C.c_void_p(a_ptr), lda, C.c_void_p(b_ptr), ldb,
                                       C.c_void_p(c_ptr), ldc))
