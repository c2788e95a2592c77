"""ctypes binding of libnmz_gpu.so (the C ABI declared in include/nmz_gpu.h).

The HIP library is the only compute path: if it is missing this module raises
NmzLibraryError instead of falling back to anything on the CPU.
"""
import ctypes
import os
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# NMZ_LIB_PATH: an alternative in-tree build of the same library (tuning variants)
DEFAULT_LIB_PATH = os.path.join(HERE, "libnmz_gpu.so")
LIB_PATH = os.environ.get("NMZ_LIB_PATH") or DEFAULT_LIB_PATH

NMZ_OK = 0
NMZ_EINVAL = -1
NMZ_EHIP = -2
NMZ_ENOMEM = -3
NMZ_ERANGE = -4
NMZ_EAGAIN = -5

NMZ_EV_PRIORITIZED = 0x01
NMZ_EV_FAULTABLE = 0x02
NMZ_STAT_RNG_OVERFLOW = 0x01
NMZ_NONE = 0xFFFFFFFF
NMZ_ED_NCOUNTERS = 6
NMZ_ED_OPT_SINGLE_KERNEL, NMZ_ED_OPT_NO_QGRAM, NMZ_ED_OPT_COMPACT, NMZ_ED_OPT_HOST_BUILD = 1, 2, 4, 8
NMZ_ED_FP_WORDS = 8
NMZ_PROC_MILD, NMZ_PROC_EXTREME, NMZ_PROC_DIRICHLET = 0, 1, 2
NMZ_PROCSET_MAX_PROCS, NMZ_PROCSET_MAX_PRIORITIZED = 512, 256

SCHED_STATS_DTYPE = np.dtype([
    ("sum_delay_ns", "<u8"), ("max_delay_ns", "<i8"), ("argmax_event", "<u4"),
    ("n_fault", "<u4"), ("first_fault", "<u4"), ("flags", "<u4")])
assert SCHED_STATS_DTYPE.itemsize == 32
TOPK_DTYPE = np.dtype([("seed", "<u8"), ("sum_delay_ns", "<i8"), ("n_fault", "<u4"),
                       ("first_fault", "<u4")])
assert TOPK_DTYPE.itemsize == 24
# ProcSetEvent decisions (nmz_proc_attr, nmz_procset_stats, nmz_procset_topk_entry)
PROC_ATTR_DTYPE = np.dtype([("policy", "<u4"), ("nice", "<i4"), ("priority", "<u4"), ("flags", "<u4")])
assert PROC_ATTR_DTYPE.itemsize == 16
PROCSET_STATS_DTYPE = np.dtype([("sum_delay_ns", "<u8"), ("score_sum", "<i8"), ("target_score", "<i8"),
                                ("n_special", "<u4"), ("flags", "<u4")])
assert PROCSET_STATS_DTYPE.itemsize == 32
PROCSET_TOPK_DTYPE = np.dtype([("seed", "<u8"), ("target_score", "<i8")])
assert PROCSET_TOPK_DTYPE.itemsize == 16
# event-order constraints of the replayable policy (nmz_order_constraint, nmz_order_stats)
ORDER_CONSTRAINT_DTYPE = np.dtype([("before", "<u4"), ("after", "<u4"), ("margin_ns", "<i8")])
assert ORDER_CONSTRAINT_DTYPE.itemsize == 16
ORDER_STATS_DTYPE = np.dtype([("sat_mask", "<u8"), ("min_slack_ns", "<i8"), ("n_satisfied", "<u4"),
                              ("argmin_constraint", "<u4")])
assert ORDER_STATS_DTYPE.itemsize == 24


# per-seed result of a delivery sweep (nmz_delivery_stats)
DELIVERY_STATS_DTYPE = np.dtype([("sig_lo", "<u8"), ("sig_hi", "<u8"), ("min_gap_ns", "<i8"), ("gap_event", "<u4"),
                                 ("n_counted", "<u4")])
NMZ_DELIVERY_MAX_EVENTS = 4096
# per-seed result of a nearest-order sweep (nmz_target_stats) and its rank modes
TARGET_STATS_DTYPE = np.dtype([("n_discordant", "<u4"), ("prefix_len", "<u4"), ("min_gap_ns", "<i8"),
                               ("gap_event", "<u4"), ("n_in_place", "<u4")])
assert TARGET_STATS_DTYPE.itemsize == 24
NMZ_TARGET_RANK_PAIRS, NMZ_TARGET_RANK_PREFIX = 0, 1
TARGET_RANK_MODES = {"pairs": NMZ_TARGET_RANK_PAIRS, "prefix": NMZ_TARGET_RANK_PREFIX}
# order contrast: one listed pair (nmz_order_pair), one ordered pair's counts (nmz_pair_counts), nmz_contrast_info
ORDER_PAIR_DTYPE = np.dtype([("before", "<u4"), ("after", "<u4"), ("score", "<i8"), ("n_fail_with", "<u4"),
                             ("n_pass_with", "<u4"), ("n_fail_against", "<u4"), ("n_pass_against", "<u4")])
assert ORDER_PAIR_DTYPE.itemsize == 32
PAIR_COUNTS_DTYPE = np.dtype([("n_fail_with", "<u4"), ("n_pass_with", "<u4")])
CONTRAST_INFO_DTYPE = np.dtype([("n_fail", "<u4"), ("n_pass", "<u4"), ("n_positive", "<u8")])
NMZ_CONTRAST_MAX_RUNS = 65535
# one op of an edit script (nmz_edit_op) and its kinds
EDIT_OP_DTYPE = np.dtype([("a_pos", "<u4"), ("b_pos", "<u4"), ("kind", "<u4")])
assert EDIT_OP_DTYPE.itemsize == 12
NMZ_EDIT_SUB, NMZ_EDIT_DEL, NMZ_EDIT_INS = 0, 1, 2
NMZ_ALIGN_MAX_BAND = 64
NMZ_ALIGN_WIDE_MAX_BAND = 1024  # the nmz_ed_align_wide_* entry points
NMZ_PO_MAX_ENTITIES = 1024  # global entity ids of the per-entity (partial-order) edit scripts
# the PO k-NN search (nmz_po_knn_*): its band and k limits, its option bit, its work counters
NMZ_PO_KNN_MAX_BAND, NMZ_PO_KNN_MAX_K, NMZ_PO_KNN_NCOUNTERS = 64, 64, 4
NMZ_PO_KNN_OPT_NO_FILTER, NMZ_PO_KNN_OPT_WHOLE_BLOCKS = 1, 2
# the same over bands up to 1,024 (nmz_po_knn_wide_*): its band limit, its nine counters, its own option bit
NMZ_PO_KNN_WIDE_MAX_BAND, NMZ_PO_KNN_WIDE_NCOUNTERS, NMZ_PO_KNN_OPT_FULL_BAND = 1024, 9, 4
# move profiles: one table symbol's counters (nmz_move_counts) and the call's totals (nmz_move_info)
MOVE_COUNTS_DTYPE = np.dtype([("later", "<u4"), ("earlier", "<u4"), ("dropped", "<u4"), ("extra", "<u4"),
                              ("sub_from", "<u4"), ("sub_to", "<u4"), ("n_pairs", "<u4"), ("reserved", "<u4"),
                              ("span_later", "<u8"), ("span_earlier", "<u8")])
assert MOVE_COUNTS_DTYPE.itemsize == 48
MOVE_INFO_DTYPE = np.dtype([("n_scripts", "<u8"), ("n_beyond", "<u8"), ("n_ops", "<u8"), ("n_unknown", "<u8")])
assert MOVE_INFO_DTYPE.itemsize == 32


class NmzLibraryError(RuntimeError):
    """libnmz_gpu.so is missing or failed to load (no CPU fallback exists)."""


class NmzError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"nmz error {code}: {msg}")
        self.code = code


class NmzInvalidArgument(NmzError, ValueError):
    pass


class RandomParams(ctypes.Structure):
    _fields_ = [("min_ns", ctypes.c_int64 * 2), ("max_ns", ctypes.c_int64 * 2),
                ("fault_threshold", ctypes.c_int32), ("reserved", ctypes.c_uint32)]


class ProcSetParams(ctypes.Structure):
    _fields_ = [("policy", ctypes.c_int32), ("use_batch", ctypes.c_int32), ("prioritized", ctypes.c_int32),
                ("reset_threshold", ctypes.c_int32)]


# every entry point declared in include/nmz_gpu.h: name -> (restype, argtypes)
_P = ctypes.c_void_p
_u64, _i64, _u32, _i32 = ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int32
_int = ctypes.c_int
SIGNATURES = {
    "nmz_open": (_int, [_int, ctypes.POINTER(_P)]),
    "nmz_close": (_int, [_P]),
    "nmz_last_error": (ctypes.c_char_p, []),
    "nmz_abi_version": (_int, []),
    "nmz_device_count": (_int, [ctypes.POINTER(_int)]),
    "nmz_ctx_stream": (_int, [_P, ctypes.POINTER(_P)]),
    "nmz_random_params_resolve": (_int, [_i64, _i64, ctypes.c_double, _P]),
    "nmz_fnv1a64_batch": (_int, [_P, _P, _P, _u64, _P]),
    "nmz_replayable_sweep": (_int, [_P, _P, _P, _u64, _P, _P, _u32, _i64, _P, _P, _u64, _u32, _P]),
    "nmz_replayable_plan_create": (_int, [_P, _P, _P, _u32, _i64, _u64, ctypes.POINTER(_P)]),
    "nmz_replayable_plan_create_async": (_int, [_P, _P, _P, _u32, _i64, _u64, ctypes.POINTER(_P)]),
    "nmz_replayable_seeds_create": (_int, [_P, _P, _P, _u64, _u64, ctypes.POINTER(_P)]),
    "nmz_replayable_seeds_destroy": (_int, [_P]),
    "nmz_replayable_sweep_seeds_topk_dev": (_int, [_P, _P, _u64, _u32, _P, _P, _P]),
    "nmz_replayable_sweep_traces": (_int, [_P, _u32, _P, _P, _P, _i64, _u64, _u64, _u32, _P]),
    "nmz_replayable_plan_destroy": (_int, [_P]),
    "nmz_replayable_plan_kernel": (_int, [_P]),
    "nmz_replayable_plan_wt_info": (_int, [_P, ctypes.POINTER(_u32), ctypes.POINTER(_u32), ctypes.POINTER(_u64)]),
    "nmz_replayable_sweep_dev": (_int, [_P, _P, _P, _u64, _P, _P]),
    "nmz_replayable_sweep_topk_dev": (_int, [_P, _P, _P, _u64, _u64, _u32, _P, _P, _P]),
    "nmz_replayable_order_host": (_int, [_P, _u32, _P, _P, _u32, _i64, _P, _P, _u32, _P, _P]),
    "nmz_replayable_order_plan_create": (_int, [_P, _P, _P, _u32, _i64, _P, _P, _u32, _u64, ctypes.POINTER(_P)]),
    "nmz_replayable_order_plan_destroy": (_int, [_P]),
    "nmz_replayable_order_sweep_decimal_dev": (_int, [_P, _u64, _u64, _u32, _P, _P, _P]),
    "nmz_replayable_order_sweep_dev": (_int, [_P, _P, _P, _u64, _u64, _u32, _P, _P, _P]),
    "nmz_replayable_order_sweep": (_int, [_P, _P, _P, _u64, _P, _P, _u32, _i64, _P, _P, _u32, _u32, _P, _P]),
    "nmz_replayable_order_sweep_decimal": (_int, [_P, _u64, _u64, _P, _P, _u32, _i64, _P, _P, _u32, _u32, _P, _P]),
    "nmz_replayable_decide": (_int, [_P, _P, _u32, _P, _P, _u32, _i64, _P]),
    "nmz_random_decide": (_int, [_P, _u64, _P, _P, _u32, _P, _P, _P]),
    "nmz_random_sweep": (_int, [_P, _u64, _u64, _P, _P, _u32, _P, _P, _P, _P, _u64, _u32, _P]),
    "nmz_procset_params_resolve": (_int, [ctypes.c_char_p, _int, _int, ctypes.c_double, _P]),
    "nmz_procset_decide_host": (_int, [_u64, _P, _P, _P, _u32, _P, _P, _P, _P]),
    "nmz_procset_decide": (_int, [_P, _u64, _P, _P, _P, _u32, _P, _P, _P, _P]),
    "nmz_procset_sweep": (_int, [_P, _u64, _u64, _P, _P, _P, _P, _u32, _P, _P, _P, _P, _P, _u64, _u32, _int, _P]),
    "nmz_random_plan_create": (_int, [_P, _P, _P, _u32, _P, _u64, ctypes.POINTER(_P)]),
    "nmz_random_plan_destroy": (_int, [_P]),
    "nmz_random_sweep_dev": (_int, [_P, _u64, _u64, _P, _P]),
    "nmz_ed_pairs": (_int, [_P, _P, _P, _u32, _P, _u64, _u32, _P]),
    "nmz_ed_allpairs_knn": (_int, [_P, _P, _P, _u32, _u32, _u32, _P, _P]),
    "nmz_ed_plan_create": (_int, [_P, _P, _P, _u32, _u32, ctypes.POINTER(_P)]),
    "nmz_ed_plan_destroy": (_int, [_P]),
    "nmz_ed_plan_create_dev": (_int, [_P, _P, _P, _u32, _u32, ctypes.POINTER(_P)]),
    "nmz_ed_plan_create_opts": (_int, [_P, _P, _P, _P, _u32, _u32, _u32, ctypes.POINTER(_P)]),
    "nmz_ed_plan_fingerprint": (_int, [_P, _P]),
    "nmz_ed_plan_is_fast": (_int, [_P]),
    "nmz_ed_block_shard": (_u32, [_u32, _u32]),
    "nmz_ed_allpairs_knn_dev": (_int, [_P, _u32, _P, _P]),
    "nmz_ed_allpairs_knn_shard_dev": (_int, [_P, _u32, _u32, _u32, _P, _P]),
    "nmz_knn_merge_dev": (_int, [_P, _P, _u32, _u32, _u32, _P, _P]),
    "nmz_ed_knn_fill_dev": (_int, [_P, _u32, _P, _P]),
    "nmz_ed_plan_counters": (_int, [_P, _P, _P]),
    "nmz_debug_tp_offsets": (_int, [_P, _P, _u32, _u32, _P, _P, _P, _P]),
    "nmz_ed_plan_query_knn": (_int, [_P, _P, _P, _u32, _u32, _P, _P]),
    "nmz_ed_align_host": (_int, [_P, _u64, _P, _u64, _u32, _P, _P]),
    "nmz_ed_align_plan_create": (_int, [_P, _u32, _u64, ctypes.POINTER(_P)]),
    "nmz_ed_align_plan_destroy": (_int, [_P]),
    "nmz_ed_align_plan_info": (_int, [_P, ctypes.POINTER(_u32), ctypes.POINTER(_u64)]),
    "nmz_ed_align_pairs_dev": (_int, [_P, _P, _P, _P, _u64, _P, _P, _P]),
    "nmz_ed_align_pairs": (_int, [_P, _P, _P, _u32, _P, _u64, _u32, _P, _P]),
    "nmz_ed_align_wide_host": (_int, [_P, _u64, _P, _u64, _u32, _P, _P]),
    "nmz_ed_align_wide_plan_create": (_int, [_P, _u32, _u64, ctypes.POINTER(_P)]),
    "nmz_ed_align_wide_plan_destroy": (_int, [_P]),
    "nmz_ed_align_wide_plan_info": (_int, [_P, ctypes.POINTER(_u32), ctypes.POINTER(_u64)]),
    "nmz_ed_align_wide_pairs_dev": (_int, [_P, _P, _P, _P, _u64, _P, _P, _P]),
    "nmz_ed_align_wide_pairs": (_int, [_P, _P, _P, _u32, _P, _u64, _u32, _P, _P]),
    "nmz_script_moves_host": (_int, [_P, _u64, _P, _u64, _P, _u32, _P]),
    "nmz_move_profile_host": (_int, [_P, _P, _u32, _P, _u64, _u32, _P, _P, _P, _u64, _P, _P, _P]),
    "nmz_move_profile_dev": (_int, [_P, _P, _P, _P, _u64, _u32, _P, _P, _P, _u64, _P, _P, _P, _int, _P]),
    "nmz_move_profile": (_int, [_P, _P, _P, _u32, _P, _u64, _u32, _P, _P, _P, _u64, _P, _P, _P]),
    "nmz_ed_diff_profile": (_int, [_P, _P, _P, _u32, _P, _u64, _u32, _P, _u64, _P, _P, _P]),
    "nmz_move_profile_wide_host": (_int, [_P, _P, _u32, _P, _u64, _u32, _P, _P, _P, _u64, _P, _P, _P]),
    "nmz_move_profile_wide_dev": (_int, [_P, _P, _P, _P, _u64, _u32, _P, _P, _P, _u64, _P, _P, _P, _int, _P]),
    "nmz_move_profile_wide": (_int, [_P, _P, _P, _u32, _P, _u64, _u32, _P, _P, _P, _u64, _P, _P, _P]),
    "nmz_ed_diff_profile_wide": (_int, [_P, _P, _P, _u32, _P, _u64, _u32, _P, _u64, _P, _P, _P]),
    "nmz_po_project_dev": (_int, [_P, _P, _P, _P, _u32, _u32, _P, _P, _P, _P]),
    "nmz_po_project": (_int, [_P, _P, _P, _P, _u32, _u32, _P, _P, _P]),
    "nmz_ed_align_po_host": (_int, [_P, _P, _u64, _P, _P, _u64, _u32, _u32, _P, _P]),
    "nmz_ed_align_po_plan_create": (_int, [_P, _u32, _u32, _u64, _u64, ctypes.POINTER(_P)]),
    "nmz_ed_align_po_plan_destroy": (_int, [_P]),
    "nmz_ed_align_po_plan_info": (_int, [_P, ctypes.POINTER(_u32), ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    "nmz_ed_align_po_pairs_dev": (_int, [_P, _P, _P, _P, _P, _P, _u64, _P, _P, _P]),
    "nmz_ed_align_po_pairs": (_int, [_P, _P, _P, _P, _u32, _u32, _P, _u64, _u32, _P, _P]),
    "nmz_ed_diff_profile_po": (_int, [_P, _P, _P, _P, _u32, _u32, _P, _u64, _u32, _P, _u64, _P, _P, _P]),
    "nmz_po_knn_plan_create": (_int, [_P, _P, _P, _P, _u32, _u32, _u32, _u64, _u64, _u32, ctypes.POINTER(_P)]),
    "nmz_po_knn_plan_destroy": (_int, [_P]),
    "nmz_po_knn_plan_info": (_int, [_P, ctypes.POINTER(_u64), ctypes.POINTER(_u32), ctypes.POINTER(_u32)]),
    "nmz_po_knn_query_dev": (_int, [_P, _P, _P, _P, _P, _u32, _u32, _P, _P]),
    "nmz_po_knn_query": (_int, [_P, _P, _P, _P, _P, _u32, _u32, _P, _P]),
    "nmz_po_knn": (_int, [_P, _P, _P, _P, _u32, _u32, _P, _P, _P, _P, _u32, _u32, _u32, _P, _P]),
    "nmz_po_knn_counters": (_int, [_P, _P, _P]),
    "nmz_po_knn_wide_plan_create": (_int, [_P, _P, _P, _P, _u32, _u32, _u32, _u64, _u64, _u32, ctypes.POINTER(_P)]),
    "nmz_po_knn_wide": (_int, [_P, _P, _P, _P, _u32, _u32, _P, _P, _P, _P, _u32, _u32, _u32, _P, _P]),
    "nmz_po_knn_wide_counters": (_int, [_P, _P, _P]),
    "nmz_po_knn_bound_host": (_int, [_P, _P, _u64, _P, _P, _u64, _u32, ctypes.POINTER(_u32), ctypes.POINTER(_u32)]),
    "nmz_replayable_delivery_host": (_int, [_P, _u32, _P, _P, _u32, _i64, _P, _P, _P, _P, _P, _P]),
    "nmz_replayable_delivery_plan_create": (_int, [_P, _P, _P, _u32, _i64, _P, _P, _P, _u64, ctypes.POINTER(_P)]),
    "nmz_replayable_delivery_plan_destroy": (_int, [_P]),
    "nmz_replayable_delivery_sweep_decimal_dev": (_int, [_P, _u64, _u64, _P, _P]),
    "nmz_replayable_delivery_sweep_dev": (_int, [_P, _P, _P, _u64, _P, _P]),
    "nmz_delivery_classes_dev": (_int, [_P, _P, _u32, _P, _P, _P, _P]),
    "nmz_sig_classes_dev": (_int, [_P, _P, _u32, _P, _P]),
    "nmz_replayable_delivery_sweep": (_int, [_P, _P, _P, _u64, _P, _P, _u32, _i64, _P, _P, _P, _P, _P, _P, _P]),
    "nmz_replayable_delivery_sweep_decimal": (_int, [_P, _u64, _u64, _P, _P, _u32, _i64, _P, _P, _P, _P, _P, _P,
                                                     _P]),
    "nmz_replayable_target_host": (_int, [_P, _u32, _P, _P, _u32, _i64, _P, _P, _P, _P, _P, _P]),
    "nmz_replayable_target_plan_create": (_int, [_P, _P, _P, _u32, _i64, _P, _P, _P, _u64, ctypes.POINTER(_P)]),
    "nmz_replayable_target_plan_destroy": (_int, [_P]),
    "nmz_replayable_target_plan_info": (_int, [_P, _P, _P]),
    "nmz_replayable_target_sweep_decimal_dev": (_int, [_P, _u64, _u64, _int, _u32, _P, _P, _P]),
    "nmz_replayable_target_sweep_dev": (_int, [_P, _P, _P, _u64, _u64, _int, _u32, _P, _P, _P]),
    "nmz_replayable_target_sweep": (_int, [_P, _P, _P, _u64, _P, _P, _u32, _i64, _P, _P, _P, _int, _u32, _P, _P, _P,
                                           _P]),
    "nmz_order_contrast_host": (_int, [_P, _P, _u32, _u32, _u32, _u32, _P, _P]),
    "nmz_order_contrast_dev": (_int, [_P, _P, _P, _u32, _u32, _u32, _P, _P, _P, _P]),
    "nmz_order_contrast": (_int, [_P, _P, _P, _u32, _u32, _u32, _P, _P, _P]),
    "nmz_replayable_target_sweep_decimal": (_int, [_P, _u64, _u64, _P, _P, _u32, _i64, _P, _P, _P, _int, _u32, _P,
                                                   _P, _P, _P]),
    "nmz_match_run_host": (_int, [_P, _P, _u32, _P, _u64, _P]),
    "nmz_match_plan_create": (_int, [_P, _P, _P, _u32, ctypes.POINTER(_P)]),
    "nmz_match_plan_destroy": (_int, [_P]),
    "nmz_match_plan_info": (_int, [_P, ctypes.POINTER(_u32), ctypes.POINTER(_u32)]),
    "nmz_match_runs_dev": (_int, [_P, _P, _P, _u64, _P, _P]),
    "nmz_match_runs": (_int, [_P, _P, _P, _u32, _P, _P, _u64, _P]),
    "nmz_order_contrast_runs": (_int, [_P, _P, _P, _u32, _P, _P, _P, _u32, _u32, _P, _P, _P]),
    "nmz_trace_signatures": (_int, [_P, _P, _P, _P, _u32, _P]),
    "nmz_unique_traces": (_int, [_P, _P, _P, _P, _u32, _P]),
    "nmz_unique_traces_dev": (_int, [_P, _P, _P, _P, _u32, _u32, _P, _P, _P]),
    "nmz_topk_select_dev": (_int, [_P, _P, _u64, _u64, _u32, _P, _P]),
    "nmz_replayable_sweep_decimal_topk_dev": (_int, [_P, _u64, _u64, _u32, _P, _P, _P]),
    "nmz_random_decide_host": (_int, [_u64, _P, _P, _u32, _P, _P, _P]),
    "nmz_replayable_decide_host": (_int, [_P, _u32, _P, _P, _u32, _i64, _P]),
    "nmz_fnv1a64_batch_host": (_int, [_P, _P, _u64, _P]),
    "nmz_tbqueue_create": (_int, [ctypes.POINTER(_P)]),
    "nmz_tbqueue_close": (_int, [_P]),
    "nmz_tbqueue_destroy": (_int, [_P]),
    "nmz_monotonic_ns": (_i64, []),
    "nmz_tbqueue_enqueue": (_int, [_P, _u64, _i64]),
    "nmz_tbqueue_enqueue_fixed": (_int, [_P, _u64, _i64, _i64]),
    "nmz_tbqueue_dequeue": (_int, [_P, _i64, ctypes.POINTER(_u64), ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
    "nmz_tbqueue_stats": (_int, [_P, ctypes.POINTER(_u64), ctypes.POINTER(_u64), ctypes.POINTER(_u64)]),
    # device groups (multi-GPU inside the C ABI, csrc/group.hip)
    "nmz_open_group": (_int, [_u32, _u32, ctypes.POINTER(_P)]),
    "nmz_group_unique_id": (_int, [_P]),
    "nmz_open_group_rank": (_int, [_P, _int, _int, _int, _u32, ctypes.POINTER(_P)]),
    "nmz_close_group": (_int, [_P]),
    "nmz_group_info": (_int, [_P, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_u32)]),
    "nmz_group_collectives": (_int, [_P, ctypes.POINTER(_u64)]),
    "nmz_topk_merge_dev": (_int, [_P, _P, _u64, _u32, _P, _P, _P]),
    "nmz_replayable_group_plan_create": (_int, [_P, _P, _P, _u32, _i64, _u64, ctypes.POINTER(_P)]),
    "nmz_replayable_group_plan_destroy": (_int, [_P]),
    "nmz_replayable_group_sweep": (_int, [_P, _P, _P, _u64, _u32, _P, _P]),
    "nmz_replayable_group_sweep_decimal": (_int, [_P, _u64, _u64, _u32, _P, _P]),
    "nmz_replayable_sweep_topk_group": (_int, [_P, _P, _P, _u64, _P, _P, _u32, _i64, _u32, _P, _P]),
    "nmz_random_group_plan_create": (_int, [_P, _P, _P, _u32, _P, _u64, ctypes.POINTER(_P)]),
    "nmz_random_group_plan_destroy": (_int, [_P]),
    "nmz_random_group_sweep": (_int, [_P, _u64, _u64, _u32, _P, _P]),
    "nmz_random_sweep_topk_group": (_int, [_P, _u64, _u64, _P, _P, _u32, _P, _u32, _P, _P]),
    "nmz_ed_group_plan_create": (_int, [_P, _P, _P, _u32, _u32, ctypes.POINTER(_P)]),
    "nmz_ed_group_plan_create_opts": (_int, [_P, _P, _P, _u32, _u32, _u32, ctypes.POINTER(_P)]),
    "nmz_ed_group_plan_destroy": (_int, [_P]),
    "nmz_ed_group_plan_timing": (_int, [_P, _P, _P, _P]),
    "nmz_ed_group_allpairs_knn": (_int, [_P, _u32, _P, _P]),
    "nmz_ed_allpairs_knn_group": (_int, [_P, _P, _P, _u32, _u32, _u32, _P, _P]),
    "nmz_timing_enable": (_int, [_P, _int]),
    "nmz_timing_read": (_int, [_P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                ctypes.POINTER(_u64), _int]),
    "nmz_timing_read_span": (_int, [_P, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                ctypes.POINTER(_u64), _int]),
}

_lib = None
_lock = threading.Lock()


def load():
    """Load libnmz_gpu.so (fails loudly; there is no CPU fallback)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NmzLibraryError(
                f"{LIB_PATH} not found: build it with `make -C namazu_amd/csrc` "
                "(or __graft_entry__.build()); the engine has no CPU fallback")
        try:
            import torch  # noqa: F401  (pin one HIP runtime per process when torch is present)
        except Exception:
            pass
        try:
            L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        except OSError as e:
            raise NmzLibraryError(f"failed to load {LIB_PATH}: {e}") from e
        variant = LIB_PATH != DEFAULT_LIB_PATH  # an A/B build (NMZ_LIB_PATH) may predate newer entry points
        for name, (res, args) in SIGNATURES.items():
            if variant and not hasattr(L, name):
                continue
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
        return L


def last_error():
    return load().nmz_last_error().decode(errors="replace")


def check(rc):
    if rc != NMZ_OK:
        msg = last_error()
        if rc == NMZ_EINVAL:
            raise NmzInvalidArgument(rc, msg)
        raise NmzError(rc, msg)


def ptr(a):
    """Data pointer of a numpy array (None for None)."""
    if a is None:
        return None
    return ctypes.c_void_p(a.ctypes.data)


def resolve_random_params(min_ns, max_ns, probability):
    p = RandomParams()
    check(load().nmz_random_params_resolve(int(min_ns), int(max_ns), float(probability),
                                           ctypes.byref(p)))
    return p


def resolve_procset_params(proc_policy="mild", use_batch=True, prioritized=3, reset_probability=0.1):
    """nmz_procset_params_resolve: loadProcConfig's checks (randompolicy.go:230-270) and the kernels' integers."""
    p = ProcSetParams()
    name = None if proc_policy is None else str(proc_policy).encode()
    check(load().nmz_procset_params_resolve(name, int(bool(use_batch)), int(prioritized), float(reset_probability),
                                            ctypes.byref(p)))
    return p


class Context:
    """One device context (libnmz_gpu nmz_ctx). Use as a context manager."""

    def __init__(self, device=0):
        self._lib = load()
        h = ctypes.c_void_p()
        check(self._lib.nmz_open(int(device), ctypes.byref(h)))
        self.handle = h
        self.device = device

    def stream(self):
        """The context's own HIP stream handle (int): what a NULL stream argument means."""
        s = ctypes.c_void_p()
        check(self._lib.nmz_ctx_stream(self.handle, ctypes.byref(s)))
        return s.value

    def close(self):
        if self.handle:
            self._lib.nmz_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count():
    n = ctypes.c_int()
    check(load().nmz_device_count(ctypes.byref(n)))
    return n.value


_default_ctx = {}


def default_context(device=0):
    ctx = _default_ctx.get(device)
    if ctx is None:
        ctx = _default_ctx[device] = Context(device)
    return ctx
