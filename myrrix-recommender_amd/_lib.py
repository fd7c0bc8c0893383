"""ctypes binding of libmyrrix_als.so (the C-ABI of include/myrrix_als.h).

There is deliberately no fallback: if the HIP library is missing or a call fails, this raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MALS_LIB") or os.path.join(_HERE, "csrc", "libmyrrix_als.so")  # MALS_LIB: A/B builds

OK, SINGULAR, INVALID_ARG, HIP_ERROR, COMM_ERROR, CANCELLED, OOM, ILL_CONDITIONED, IO_ERROR = range(9)
SIDE_X, SIDE_Y = 0, 1
FLAG_RECONSTRUCT_R, FLAG_LOSS_IGNORES_UNSPECIFIED = 1, 2
SIMILAR_FILTER_QUERY_ITEMS = 1   # MALS_SIMILAR_FILTER_QUERY_ITEMS
MEM_HOST, MEM_DEVICE = 0, 1
GRAMIAN_AUTO, GRAMIAN_FP32, GRAMIAN_SPLIT_F16, GRAMIAN_SPLIT3_F16 = 0, 1, 2, 3
SOLVE_AUTO, SOLVE_DIRECT, SOLVE_DUAL = 0, 1, 2
ABI_VERSION = 5
GROUP_RCCL, GROUP_PEER_COPY = 0, 1
INGEST_OPT_KNOWN_ITEMS, INGEST_OPT_TEXT_BLOCK_BYTES, INGEST_OPT_RESERVE_RECORDS, INGEST_OPT_PARTITION_RECORDS, INGEST_OPT_SHARE = 1, 2, 3, 4, 5
INGEST_OPT_TAB_DELIMITER = 6
INGEST_OPT_LIVE_TAGS = 7
ITEM_TAG_IDS, USER_TAG_IDS = 0, 1
INSTALL_COPY = 1

STATUS_NAMES = {OK: "OK", SINGULAR: "SINGULAR", INVALID_ARG: "INVALID_ARG", HIP_ERROR: "HIP_ERROR",
                COMM_ERROR: "COMM_ERROR", CANCELLED: "CANCELLED", OOM: "OOM",
                ILL_CONDITIONED: "ILL_CONDITIONED", IO_ERROR: "IO_ERROR"}


class Config(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("features", ctypes.c_int32),
                ("alpha", ctypes.c_double), ("lam", ctypes.c_double),
                ("singularity_threshold", ctypes.c_double), ("flags", ctypes.c_int32),
                ("device", ctypes.c_int32), ("segment_nnz", ctypes.c_int32),
                ("chunk_rows", ctypes.c_int32), ("gramian_mode", ctypes.c_int32),
                ("solve_mode", ctypes.c_int32)]


class Stats(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("rows_ms", ctypes.c_double), ("segments_ms", ctypes.c_double),
                ("finish_ms", ctypes.c_double), ("gramian_ms", ctypes.c_double),
                ("rows_launches", ctypes.c_int64), ("segments_launches", ctypes.c_int64),
                ("finish_launches", ctypes.c_int64), ("gramian_launches", ctypes.c_int64),
                ("rows_bytes", ctypes.c_double), ("segments_bytes", ctypes.c_double),
                ("finish_bytes", ctypes.c_double), ("gramian_bytes", ctypes.c_double),
                ("rows_solved", ctypes.c_int64), ("nnz_gathered", ctypes.c_int64),
                ("dual_ms", ctypes.c_double), ("rotate_ms", ctypes.c_double),
                ("dual_launches", ctypes.c_int64), ("rotate_launches", ctypes.c_int64),
                ("dual_bytes", ctypes.c_double), ("rotate_bytes", ctypes.c_double),
                ("rows_dual", ctypes.c_int64), ("eigen_host_ms", ctypes.c_double), ("rows_refined", ctypes.c_int64)]


class ModelView(ctypes.Structure):
    """mals_model_view"""
    _fields_ = [("struct_size", ctypes.c_int32), ("features", ctypes.c_int32),
                ("n_users", ctypes.c_int64), ("user_ids", ctypes.c_void_p), ("X", ctypes.c_void_p),
                ("n_items", ctypes.c_int64), ("item_ids", ctypes.c_void_p), ("Y", ctypes.c_void_p),
                ("n_known", ctypes.c_int64), ("known_user_ids", ctypes.c_void_p),
                ("known_ptr", ctypes.c_void_p), ("known_item_ids", ctypes.c_void_p),
                ("n_item_tags", ctypes.c_int64), ("item_tag_ids", ctypes.c_void_p),
                ("n_user_tags", ctypes.c_int64), ("user_tag_ids", ctypes.c_void_p),
                ("n_user_clusters", ctypes.c_int64), ("user_cluster_member_ptr", ctypes.c_void_p),
                ("user_cluster_members", ctypes.c_void_p), ("user_cluster_centroid_ptr", ctypes.c_void_p),
                ("user_cluster_centroids", ctypes.c_void_p),
                ("n_item_clusters", ctypes.c_int64), ("item_cluster_member_ptr", ctypes.c_void_p),
                ("item_cluster_members", ctypes.c_void_p), ("item_cluster_centroid_ptr", ctypes.c_void_p),
                ("item_cluster_centroids", ctypes.c_void_p)]


class IterationInfo(ctypes.Structure):   # mals_iteration_info
    _fields_ = [("struct_size", ctypes.c_int32), ("iteration", ctypes.c_int32), ("avg_abs_difference", ctypes.c_double),
                ("seconds", ctypes.c_double), ("x_rows", ctypes.c_int64), ("y_rows", ctypes.c_int64),
                ("entries_gathered", ctypes.c_int64), ("algorithmic_bytes", ctypes.c_double), ("devices", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class IngestTextInfo(ctypes.Structure):   # mals_ingest_text_info_t
    _fields_ = [("struct_size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("lines", ctypes.c_int64), ("bad_lines", ctypes.c_int64),
                ("header_lines", ctypes.c_int64), ("skipped_lines", ctypes.c_int64), ("full_parser_lines", ctypes.c_int64),
                ("text_bytes", ctypes.c_int64), ("records", ctypes.c_int64), ("parse_ms", ctypes.c_double), ("stage_ms", ctypes.c_double),
                ("n_item_tag_ids", ctypes.c_int64), ("n_user_tag_ids", ctypes.c_int64), ("n_known_items", ctypes.c_int64)]


GENERATION_KEEP_NOT_UPDATED, GENERATION_RECOMPUTE_SOLVERS = 1, 2


class GenerationLoad(ctypes.Structure):   # mals_generation_load
    _fields_ = [("struct_size", ctypes.c_int32), ("flags", ctypes.c_int32), ("features", ctypes.c_int32), ("cur_mem_kind", ctypes.c_int32),
                ("new_mem_kind", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("cur_ids", ctypes.c_void_p * 2), ("n_cur", ctypes.c_int64 * 2),
                ("new_ids", ctypes.c_void_p * 2), ("n_new", ctypes.c_int64 * 2), ("new_rows", ctypes.c_void_p * 2),
                ("new_known_ptr", ctypes.c_void_p), ("new_known_idx", ctypes.c_void_p),
                ("item_tag_ids", ctypes.c_void_p), ("n_item_tag_ids", ctypes.c_int64),
                ("user_tag_ids", ctypes.c_void_p), ("n_user_tag_ids", ctypes.c_int64)]


class GenerationResult(ctypes.Structure):   # mals_generation_result
    _fields_ = [("struct_size", ctypes.c_int32), ("solver_status", ctypes.c_int32),
                ("n_merged", ctypes.c_int64 * 2), ("n_updated", ctypes.c_int64 * 2), ("n_kept", ctypes.c_int64 * 2), ("n_pruned", ctypes.c_int64 * 2),
                ("n_known_dropped", ctypes.c_int64), ("n_tag_ids_without_row", ctypes.c_int64),
                ("join_ms", ctypes.c_double * 2), ("scan_ms", ctypes.c_double * 2), ("gather_ms", ctypes.c_double * 2),
                ("sides_ms", ctypes.c_double), ("known_ms", ctypes.c_double), ("tags_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


ITERATION_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.POINTER(IterationInfo))


def create_error():
    """mals_create_error: why the last mals_create / mals_group_create* on this thread failed ("" after a success)."""
    buf = ctypes.create_string_buffer(1024)
    load().mals_create_error(buf, len(buf))
    return buf.value.decode("utf-8", "replace")


# every symbol include/myrrix_als.h declares: name -> (restype, argtypes)
_H = ctypes.c_void_p
_I64 = ctypes.c_int64
_I32 = ctypes.c_int32
_P = ctypes.c_void_p
SYMBOLS = {
    "mals_abi_version": (ctypes.c_int, []),
    "mals_default_config": (ctypes.c_int, [ctypes.POINTER(Config)]),
    "mals_create": (ctypes.c_int, [ctypes.POINTER(Config), ctypes.POINTER(_H)]),
    "mals_destroy": (ctypes.c_int, [_H]),
    "mals_last_error": (ctypes.c_char_p, [_H]),
    "mals_create_error": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t]),
    "mals_group_create_error": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t]),
    "mals_set_iteration_callback": (ctypes.c_int, [_H, _P, _P]),
    "mals_group_set_iteration_callback": (ctypes.c_int, [_H, _P, _P]),
    "mals_set_stream": (ctypes.c_int, [_H, _P]),
    "mals_set_factor_rows": (ctypes.c_int, [_H, ctypes.c_int, _I64]),
    "mals_bind_factors": (ctypes.c_int, [_H, ctypes.c_int, _P, _I64]),
    "mals_factor_device_ptr": (ctypes.c_int, [_H, ctypes.c_int, ctypes.POINTER(_P), ctypes.POINTER(_I64)]),
    "mals_set_matrix": (ctypes.c_int, [_H, ctypes.c_int, _I64, _I64, _I64, _P, _P, _P, ctypes.c_int]),
    "mals_begin_matrix": (ctypes.c_int, [_H, ctypes.c_int, _I64, _I64, _I64]),
    "mals_append_rows": (ctypes.c_int, [_H, ctypes.c_int, _I64, _P, _P, _P]),
    "mals_end_matrix": (ctypes.c_int, [_H, ctypes.c_int]),
    "mals_get_value_bound": (ctypes.c_int, [_H, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "mals_set_value_bound": (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_float]),
    "mals_get_value_stats": (ctypes.c_int, [_H, ctypes.c_int, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_int64)]),
    "mals_set_value_stats": (ctypes.c_int, [_H, ctypes.c_int, ctypes.c_float, ctypes.c_double]),
    "mals_set_factors": (ctypes.c_int, [_H, ctypes.c_int, _I64, _I64, _P]),
    "mals_get_factors": (ctypes.c_int, [_H, ctypes.c_int, _I64, _I64, _P]),
    "mals_get_rows": (ctypes.c_int, [_H, ctypes.c_int, _P, _I32, _P]),
    "mals_gramian": (ctypes.c_int, [_H, ctypes.c_int, _P]),
    "mals_gramian_partial": (ctypes.c_int, [_H, ctypes.c_int, _I64, _I64, _P]),
    "mals_set_gramian": (ctypes.c_int, [_H, ctypes.c_int, _P, ctypes.c_int]),
    "mals_solve_side": (ctypes.c_int, [_H, ctypes.c_int]),
    "mals_solve_chunk": (ctypes.c_int, [_H, ctypes.c_int, _I32]),
    "mals_num_chunks": (ctypes.c_int, [_H, ctypes.c_int, ctypes.POINTER(_I32)]),
    "mals_set_chunk_rows": (ctypes.c_int, [_H, ctypes.c_int, _I64]),
    "mals_set_refine_limit": (ctypes.c_int, [_H, ctypes.c_double]),
    "mals_check": (ctypes.c_int, [_H]),
    "mals_singular_info": (ctypes.c_int, [_H, ctypes.POINTER(_I32), ctypes.POINTER(_I64), ctypes.POINTER(_I32)]),
    "mals_half_iteration": (ctypes.c_int, [_H, ctypes.c_int]),
    "mals_factorize": (ctypes.c_int, [_H, ctypes.c_double, _I32, _I32, _I32, _P, _I32, _P, _I32,
                                      ctypes.POINTER(_I32), ctypes.POINTER(ctypes.c_double)]),
    "mals_sample_dots": (ctypes.c_int, [_H, _P, _I32, _P, _I32, _P]),
    "mals_symmetric_eigen": (ctypes.c_int, [_P, _I32, _P, _P]),
    "mals_cancel": (ctypes.c_int, [_H]),
    "mals_recompute_solver": (ctypes.c_int, [_H, ctypes.c_int, ctypes.POINTER(_H), ctypes.POINTER(ctypes.c_double)]),
    "mals_solver_create": (ctypes.c_int, [_P, _I32, ctypes.c_double, ctypes.POINTER(_H), ctypes.POINTER(_I32)]),
    "mals_solver_dim": (ctypes.c_int, [_H]),
    "mals_solver_solve_dtof": (ctypes.c_int, [_H, _P, _P]),
    "mals_solver_solve_ftod": (ctypes.c_int, [_H, _P, _P]),
    "mals_solver_destroy": (ctypes.c_int, [_H]),
    "mals_reconstruction_error": (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_I64)]),
    "mals_recommend": (ctypes.c_int, [_H, _P, _I32, _I32, _I32, _P, _P, _P]),
    "mals_recommend_vectors": (ctypes.c_int, [_H, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    "mals_set_known_items": (ctypes.c_int, [_H, _I64, _P, _P, ctypes.c_int]),
    "mals_recommend_to_many": (ctypes.c_int, [_H, _P, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    "mals_features": (ctypes.c_int, [_H]),
    "mals_recommend_front_stats": (ctypes.c_int, [_H, _P]),
    "mals_recommend_set_depth": (ctypes.c_int, [_H, _I32]),
    "mals_recommend_set_spin_us": (ctypes.c_int, [_H, _I32]),
    "mals_most_similar_items": (ctypes.c_int, [_H, _P, _P, _I32, _I32, _P, _P, _P]),
    "mals_most_similar_items_rescored": (ctypes.c_int, [_H, _H, _I32, _P, _P, _I32, _I32, _P, _P, _P]),
    "mals_similar_stats": (ctypes.c_int, [_H, _P]),
    "mals_similarity_to_item": (ctypes.c_int, [_H, ctypes.c_int64, _P, _I32, _P]),
    "mals_recommended_because": (ctypes.c_int, [_H, _P, _P, _I32, _I32, _P, _P, _P]),
    "mals_set_foldin_solver": (ctypes.c_int, [_H, ctypes.c_int, _H]),
    "mals_set_foldin_learn_rate": (ctypes.c_int, [_H, ctypes.c_double]),
    "mals_foldin_stats": (ctypes.c_int, [_H, _P]),
    "mals_foldin_solve": (ctypes.c_int, [_H, ctypes.c_int, _P, _I32, _P]),
    "mals_set_preferences": (ctypes.c_int, [_H, _I64, _P, _P, _P, _P]),
    "mals_set_user_tags": (ctypes.c_int, [_H, _I64, _P, _P, _P, _P]),
    "mals_set_item_tags": (ctypes.c_int, [_H, _I64, _P, _P, _P, _P]),
    "mals_get_tag_rows": (ctypes.c_int, [_H, ctypes.c_int, _P, _I64, ctypes.POINTER(_I64)]),
    "mals_tag_id_host": (ctypes.c_int, [_P, _I64, ctypes.POINTER(_I64)]),
    "mals_remove_preferences": (ctypes.c_int, [_H, _I64, _P, _P, _P, ctypes.POINTER(_I64)]),
    "mals_grow_factor_rows": (ctypes.c_int, [_H, ctypes.c_int, _I64]),
    "mals_estimate_preferences": (ctypes.c_int, [_H, _I64, _P, _P, _P]),
    "mals_anonymous_features": (ctypes.c_int, [_H, _I32, _P, _P, _P, _P, _P]),
    "mals_recommend_to_anonymous": (ctypes.c_int, [_H, _I32, _P, _P, _P, _I32, _P, _P, _P, _P]),
    "mals_rescorer_create": (ctypes.c_int, [_H, ctypes.POINTER(_H)]),
    "mals_rescorer_destroy": (ctypes.c_int, [_H]),
    "mals_rescorer_set_filter": (ctypes.c_int, [_H, _I64, _P, ctypes.c_int]),
    "mals_rescorer_set_weights": (ctypes.c_int, [_H, _P, _P, _I64, ctypes.c_int]),
    "mals_rescorer_set_uniform": (ctypes.c_int, [_H, ctypes.c_double, ctypes.c_double]),
    "mals_recommend_rescored": (ctypes.c_int, [_H, _H, _P, _I32, _I32, _I32, _P, _P, _P]),
    "mals_recommend_to_many_rescored": (ctypes.c_int, [_H, _H, _P, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    "mals_recommend_to_anonymous_rescored": (ctypes.c_int, [_H, _H, _I32, _P, _P, _P, _I32, _P, _P, _P, _P]),
    "mals_lsh_max_bits_differing": (ctypes.c_int, [ctypes.c_double, _I32, ctypes.POINTER(_I32)]),
    "mals_lsh_build": (ctypes.c_int, [_H, _I32, _I32, _P, _P]),
    "mals_lsh_clear": (ctypes.c_int, [_H]),
    "mals_lsh_info": (ctypes.c_int, [_H, _P]),
    "mals_lsh_get": (ctypes.c_int, [_H, _P, _I64, _I64, _P]),
    "mals_lsh_signatures": (ctypes.c_int, [_H, _P, _I32, _P]),
    "mals_estimate_for_anonymous": (ctypes.c_int, [_H, _I32, _P, _P, _P, _P, _P, _P]),
    "mals_set_tag_items": (ctypes.c_int, [_H, _I64, _P, ctypes.c_int]),
    "mals_get_tag_item_count": (ctypes.c_int, [_H, ctypes.POINTER(_I64)]),
    "mals_set_tag_users": (ctypes.c_int, [_H, _I64, _P, ctypes.c_int]),
    "mals_get_tag_user_count": (ctypes.c_int, [_H, ctypes.POINTER(_I64)]),
    "mals_most_popular_items": (ctypes.c_int, [_H, _H, _I32, _P, _P, ctypes.POINTER(_I32)]),
    "mals_most_popular_stats": (ctypes.c_int, [_H, _P]),
    "mals_group_set_tag_users": (ctypes.c_int, [_H, _I64, _P]),
    "mals_group_most_popular_items": (ctypes.c_int, [_H, _I32, _P, _P, ctypes.POINTER(_I32)]),
    "mals_ingest_device": (ctypes.c_int, [_H, ctypes.POINTER(_I32)]),
    "mals_ingest_device_tag_items": (ctypes.c_int, [_H, ctypes.POINTER(_P), ctypes.POINTER(_I64)]),
    "mals_ingest_get_tag_items": (ctypes.c_int, [_H, _P]),
    "mals_ingest_install_group": (ctypes.c_int, [_H, _H, _I32]),
    "mals_ingest_create": (ctypes.c_int, [_I32, ctypes.c_float, ctypes.POINTER(_H)]),
    "mals_ingest_destroy": (ctypes.c_int, [_H]),
    "mals_ingest_last_error": (ctypes.c_char_p, [_H]),
    "mals_ingest_append": (ctypes.c_int, [_H, _I64, _P, _P, _P, ctypes.c_int]),
    "mals_ingest_finish": (ctypes.c_int, [_H]),
    "mals_ingest_counts": (ctypes.c_int, [_H, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "mals_ingest_get_ids": (ctypes.c_int, [_H, ctypes.c_int, _P]),
    "mals_ingest_get_csr": (ctypes.c_int, [_H, ctypes.c_int, _P, _P, _P]),
    "mals_ingest_device_csr": (ctypes.c_int, [_H, ctypes.c_int, ctypes.POINTER(_P), ctypes.POINTER(_P), ctypes.POINTER(_P)]),
    "mals_ingest_install": (ctypes.c_int, [_H, _H]),
    "mals_ingest_stats": (ctypes.c_int, [_H, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                         ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_I32)]),
    "mals_ingest_set_option": (ctypes.c_int, [_H, _I32, _I64]),
    "mals_ingest_partitions": (ctypes.c_int, [_H, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
    "mals_ingest_append_text": (ctypes.c_int, [_H, _P, _I64, ctypes.c_int, _I32]),
    "mals_ingest_read_file": (ctypes.c_int, [_H, ctypes.c_char_p]),
    "mals_ingest_read_dir": (ctypes.c_int, [_H, ctypes.c_char_p, ctypes.POINTER(_I32)]),
    "mals_ingest_read_dir_share": (ctypes.c_int, [_H, ctypes.c_char_p, _I32, _I32, ctypes.POINTER(_I32)]),
    "mals_group_ingest_finish": (ctypes.c_int, [_H, _P, _I32, _I32]),
    "mals_ingest_slice": (ctypes.c_int, [_H, ctypes.c_int, ctypes.POINTER(_I64), ctypes.POINTER(_I64)]),
    "mals_ingest_memory": (ctypes.c_int, [_H, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(ctypes.c_double),
                                          ctypes.POINTER(ctypes.c_double)]),
    "mals_ingest_text_info": (ctypes.c_int, [_H, ctypes.POINTER(IngestTextInfo)]),
    "mals_ingest_get_tag_ids": (ctypes.c_int, [_H, _I32, _P]),
    "mals_ingest_get_known_items": (ctypes.c_int, [_H, _P, _P]),
    "mals_ingest_device_known_items": (ctypes.c_int, [_H, ctypes.POINTER(_P), ctypes.POINTER(_P), ctypes.POINTER(_I64)]),
    "mals_plan_shards": (ctypes.c_int, [_P, _I64, _I32, ctypes.c_double, _I32, _P]),
    "mals_group_set_alternate_streams": (ctypes.c_int, [_H, _I32]),
    "mals_group_create": (ctypes.c_int, [ctypes.POINTER(Config), _P, _I32, _I32, ctypes.POINTER(_H)]),
    "mals_group_unique_id": (ctypes.c_int, [_P]),
    "mals_group_create_rank": (ctypes.c_int, [ctypes.POINTER(Config), _I32, _I32, _P, ctypes.POINTER(_H)]),
    "mals_group_destroy": (ctypes.c_int, [_H]),
    "mals_group_last_error": (ctypes.c_char_p, [_H]),
    "mals_group_world": (ctypes.c_int, [_H]),
    "mals_group_features": (ctypes.c_int, [_H]),
    "mals_group_pending_entries": (ctypes.c_int, [_H, ctypes.c_int, _I64, ctypes.POINTER(_I64)]),
    "mals_group_local": (ctypes.c_int, [_H, _I32, ctypes.POINTER(_H), ctypes.POINTER(_I32)]),
    "mals_group_set_exchange_chunks": (ctypes.c_int, [_H, _I32]),
    "mals_group_use_transport": (ctypes.c_int, [ctypes.c_char_p]),
    "mals_group_comm_info": (ctypes.c_int, [_H, _I32, ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.POINTER(_I32), ctypes.c_char_p, _I32]),
    "mals_get_timeline": (ctypes.c_int, [_H, _P]),
    "mals_get_gather_scale": (ctypes.c_int, [_H, _P]),
    "mals_group_set_refine_limit": (ctypes.c_int, [_H, ctypes.c_double]),
    "mals_group_set_factor_rows": (ctypes.c_int, [_H, ctypes.c_int, _I64]),
    "mals_group_set_factors": (ctypes.c_int, [_H, ctypes.c_int, _I64, _I64, _P]),
    "mals_group_get_factors": (ctypes.c_int, [_H, ctypes.c_int, _I64, _I64, _P]),
    "mals_group_get_rows": (ctypes.c_int, [_H, ctypes.c_int, _P, _I32, _P]),
    "mals_group_set_matrix": (ctypes.c_int, [_H, ctypes.c_int, _I64, _I64, _P, _P, _P, ctypes.c_int]),
    "mals_group_begin_matrix": (ctypes.c_int, [_H, ctypes.c_int, _I64, _P]),
    "mals_group_append_rows": (ctypes.c_int, [_H, ctypes.c_int, _I64, _P, _P]),
    "mals_group_end_matrix": (ctypes.c_int, [_H, ctypes.c_int]),
    "mals_group_bounds": (ctypes.c_int, [_H, ctypes.c_int, _P]),
    "mals_group_recommend": (ctypes.c_int, [_H, _P, _I32, _I32, _I32, _P, _P, _P]),
    "mals_group_most_similar_items": (ctypes.c_int, [_H, _P, _P, _I32, _I32, _P, _P, _P]),
    "mals_group_similarity_to_item": (ctypes.c_int, [_H, ctypes.c_int64, _P, _I32, _P]),
    "mals_group_recommended_because": (ctypes.c_int, [_H, _P, _P, _I32, _I32, _P, _P, _P]),
    "mals_group_set_foldin_solver": (ctypes.c_int, [_H, ctypes.c_int, _H]),
    "mals_group_set_foldin_learn_rate": (ctypes.c_int, [_H, ctypes.c_double]),
    "mals_group_foldin_stats": (ctypes.c_int, [_H, _P]),
    "mals_group_set_preferences": (ctypes.c_int, [_H, _I64, _P, _P, _P, _P]),
    "mals_group_set_user_tags": (ctypes.c_int, [_H, _I64, _P, _P, _P, _P]),
    "mals_group_set_item_tags": (ctypes.c_int, [_H, _I64, _P, _P, _P, _P]),
    "mals_group_remove_preferences": (ctypes.c_int, [_H, _I64, _P, _P, _P, ctypes.POINTER(_I64)]),
    "mals_group_grow_factor_rows": (ctypes.c_int, [_H, ctypes.c_int, _I64]),
    "mals_group_estimate_preferences": (ctypes.c_int, [_H, _I64, _P, _P, _P]),
    "mals_group_anonymous_features": (ctypes.c_int, [_H, _I32, _P, _P, _P, _P, _P]),
    "mals_group_recommend_to_anonymous": (ctypes.c_int, [_H, _I32, _P, _P, _P, _I32, _P, _P, _P, _P]),
    "mals_group_estimate_for_anonymous": (ctypes.c_int, [_H, _I32, _P, _P, _P, _P, _P, _P]),
    "mals_ids_set": (ctypes.c_int, [_H, ctypes.c_int, _I64, _P, ctypes.c_int]),
    "mals_ids_lookup": (ctypes.c_int, [_H, ctypes.c_int, _I64, _P, _P]),
    "mals_ids_resolve": (ctypes.c_int, [_H, ctypes.c_int, _I64, _P, _P, ctypes.POINTER(_I64)]),
    "mals_ids_get": (ctypes.c_int, [_H, ctypes.c_int, _I64, _I64, _P]),
    "mals_ids_count": (ctypes.c_int, [_H, ctypes.c_int, ctypes.POINTER(_I64)]),
    "mals_ingest_apply": (ctypes.c_int, [_H, _H, _P, _P, _I64, ctypes.POINTER(_I64)]),
    "mals_ingest_apply_times": (ctypes.c_int, [_H, _P]),
    "mals_ingest_apply_tag_stats": (ctypes.c_int, [_H, _P]),
    "mals_factor_digest": (ctypes.c_int, [_H, ctypes.c_int, _I64, _I64, ctypes.POINTER(ctypes.c_uint64)]),
    "mals_group_replica_digest": (ctypes.c_int, [_H, ctypes.c_int, _I64, _I64, _P, ctypes.POINTER(_I32)]),
    "mals_factor_digest_host": (ctypes.c_int, [_P, _I32, _I64, _I64, ctypes.POINTER(ctypes.c_uint64)]),
    "mals_load_generation": (ctypes.c_int, [_H, ctypes.POINTER(GenerationLoad), ctypes.POINTER(GenerationResult)]),
    "mals_generation_get_ids": (ctypes.c_int, [_H, ctypes.c_int, _P]),
    "mals_generation_get_map": (ctypes.c_int, [_H, ctypes.c_int, _P]),
    "mals_mark_recent": (ctypes.c_int, [_H, ctypes.c_int, _I64, _P]),
    "mals_get_recent": (ctypes.c_int, [_H, ctypes.c_int, _P, ctypes.POINTER(_I64)]),
    "mals_group_load_generation": (ctypes.c_int, [_H, ctypes.POINTER(GenerationLoad), ctypes.POINTER(GenerationResult)]),
    "mals_group_generation_get_ids": (ctypes.c_int, [_H, ctypes.c_int, _P]),
    "mals_group_generation_get_map": (ctypes.c_int, [_H, ctypes.c_int, _P]),
    "mals_group_mark_recent": (ctypes.c_int, [_H, ctypes.c_int, _I64, _P]),
    "mals_group_get_recent": (ctypes.c_int, [_H, ctypes.c_int, _P, ctypes.POINTER(_I64)]),
    "mals_group_generation_plan_host": (ctypes.c_int, [_I32, _I32, _I64, _P, _I64, _P, _P, _P, _P, _P]),
    "mals_generation_hash_host": (ctypes.c_uint64, [_I64]),
    "mals_generation_join_host": (ctypes.c_int, [_P, _I64, _P, _I64, _P, _I64, _I32, _P, _P]),
    "mals_group_half_iteration": (ctypes.c_int, [_H, ctypes.c_int]),
    "mals_group_factorize": (ctypes.c_int, [_H, ctypes.c_double, _I32, _I32, _I32, _P, _I32, _P, _I32,
                                            ctypes.POINTER(_I32), ctypes.POINTER(ctypes.c_double)]),
    "mals_group_singular_info": (ctypes.c_int, [_H, ctypes.POINTER(_I32), ctypes.POINTER(_I64), ctypes.POINTER(_I32)]),
    "mals_group_exchange_only": (ctypes.c_int, [_H, ctypes.c_int]),
    "mals_group_cancel": (ctypes.c_int, [_H]),
    "mals_group_synchronize": (ctypes.c_int, [_H]),
    "mals_enable_timing": (ctypes.c_int, [_H, _I32]),
    "mals_model_write": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ModelView)]),
    "mals_model_read": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(_H)]),
    "mals_model_get": (ctypes.c_int, [_H, ctypes.POINTER(ModelView)]),
    "mals_model_destroy": (ctypes.c_int, [_H]),
    "mals_model_last_error": (ctypes.c_char_p, []),
    "mals_reset_stats": (ctypes.c_int, [_H]),
    "mals_get_stats": (ctypes.c_int, [_H, ctypes.POINTER(Stats)]),
}

_lib = None


def load():
    """Load libmyrrix_als.so and declare every prototype.  Raises if the library is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libmyrrix_als.so not found at %s -- build it with __graft_entry__.build() or "
                "`make -C myrrix-recommender_amd/csrc` (hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
        # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64/libhsa, and
        # a process that first binds /opt/rocm's copy (through this library) and then imports torch
        # ends up with two runtimes, the second of which sees no device.  Importing torch first
        # makes this library resolve libamdhip64.so.7 to the copy torch already mapped.  Without
        # torch (the JVM deployment) the system runtime is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the library does not export it
            fn.restype = res
            fn.argtypes = args
        if L.mals_abi_version() != ABI_VERSION:
            raise ImportError("libmyrrix_als.so ABI version mismatch")
        _lib = L
    return _lib
