"""ctypes binding of libspiral_gpu.so (the C ABI declared in include/spiral_gpu.h).

The library is the product; this module only loads it and declares prototypes.  It fails loudly when
the shared object is missing -- there is no CPU fallback anywhere in this package.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SPIRAL_LIB=<path>: load another build of the library (tuning A/B runs, tools/build_variants.sh: -DSPIRAL_TUNING builds of the same sources);
# every process of a multi-rank run inherits it.  Whatever is loaded must export every declared entry point.
LIB_PATH = os.environ.get("SPIRAL_LIB") or os.path.join(HERE, "libspiral_gpu.so")
CSRC = os.path.join(HERE, "csrc")


class Params(C.Structure):
    """spiral_gpu_params: the reference's -D scheme parameters (include/values.h:78-93) + argv[1..2]"""

    _fields_ = [
        ("nu1", C.c_uint32),
        ("nu2", C.c_uint32),
        ("t_gsw", C.c_uint32),
        ("t_conv", C.c_uint32),
        ("t_exp", C.c_uint32),
        ("t_exp_right", C.c_uint32),
        ("qprime_bits", C.c_uint32),
        ("direct_upload", C.c_uint32),
        ("p_db", C.c_uint64),
    ]


class Shape(C.Structure):
    _fields_ = [
        ("dim0", C.c_uint32),
        ("num_per", C.c_uint32),
        ("ell", C.c_uint32),
        ("m2", C.c_uint32),
        ("g", C.c_uint32),
        ("stopround", C.c_uint32),
        ("n_left", C.c_uint32),
        ("n_right", C.c_uint32),
        ("n_query_cts", C.c_uint32),
        ("n_bits", C.c_uint32),
        ("qprime", C.c_uint64),
    ]


class PackShape(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("dim0", "num_per", "ell", "g", "stopround", "n_left", "n_right", "n_query_cts", "trials")] + [
        ("qprime", C.c_uint64)
    ]


class RecordLayout(C.Structure):
    """spiral_gpu_record_layout: how records of one byte size lie in the plaintexts of a base or a SpiralPack parameter set (include/spiral_gpu.h
    "Records")"""

    _fields_ = [("coeff_bits", C.c_uint32), ("instances", C.c_uint32), ("per_item", C.c_uint64), ("item_bytes", C.c_uint64), ("capacity", C.c_uint64)]


class KvLayout(C.Structure):
    """spiral_gpu_kv_layout: how keyed records of one value size lie in the buckets (items) of a base parameter set (include/spiral_gpu.h "Keyed
    records")"""

    _fields_ = [("coeff_bits", C.c_uint32), ("slots", C.c_uint32), ("value_bytes", C.c_uint64), ("item_bytes", C.c_uint64), ("buckets", C.c_uint64),
                ("capacity", C.c_uint64)]


class KvStatsStruct(C.Structure):
    """spiral_gpu_kv_stats (include/spiral_gpu.h, spiral_gpu_server_kv_stats)"""

    _fields_ = [("buckets", C.c_uint64), ("used", C.c_uint64), ("full_buckets", C.c_uint64), ("max_used", C.c_uint32), ("slots", C.c_uint32),
                ("hist", C.c_uint64 * 257)]


class KvEntry(C.Structure):
    """spiral_gpu_kv_entry (include/spiral_gpu.h "Listing"): a slot whose tag is not 0, 16 bytes"""

    _fields_ = [("tag", C.c_uint64), ("bucket", C.c_uint32), ("slot", C.c_uint32)]


KV_ENTRY_DTYPE = np.dtype([("tag", "<u8"), ("bucket", "<u4"), ("slot", "<u4")])  # the same 16 bytes as a numpy record


class KvReconcileCounts(C.Structure):
    """spiral_gpu_kv_reconcile_counts"""

    _fields_ = [(n, C.c_uint64) for n in ("held", "missing", "shadowed", "misplaced", "orphans")]


U64P = C.POINTER(C.c_uint64)

# name -> (restype, argtypes); every symbol include/spiral_gpu.h declares
PROTOTYPES = {
    "spiral_gpu_abi_version": (C.c_int, []),
    "spiral_gpu_last_error": (C.c_char_p, []),
    "spiral_gpu_device_count": (C.c_int, []),
    "spiral_gpu_get_shape": (C.c_int, [C.POINTER(Params), C.POINTER(Shape)]),
    "spiral_gpu_has_limb_form": (C.c_int, [C.POINTER(Params), C.c_uint32, C.c_uint32]),
    "spiral_gpu_column_shard_has_limb_form": (C.c_int, [C.POINTER(Params), C.c_uint32]),
    "spiral_gpu_set_option": (C.c_int, [C.c_char_p, C.c_int64]),
    "spiral_gpu_get_option": (C.c_int, [C.c_char_p, C.POINTER(C.c_int64)]),
    "spiral_gpu_get_tables": (C.c_int, [U64P]),
    "spiral_gpu_ntt_forward": (C.c_int, [U64P, C.c_size_t]),
    "spiral_gpu_ntt_inverse": (C.c_int, [U64P, C.c_size_t]),
    "spiral_gpu_to_ntt": (C.c_int, [U64P, U64P, C.c_size_t, C.c_int]),
    "spiral_gpu_from_ntt": (C.c_int, [U64P, U64P, C.c_size_t]),
    "spiral_gpu_time_ntt": (C.c_int, [C.c_size_t, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "spiral_gpu_time_ntt_digits": (C.c_int, [C.c_size_t, C.c_uint32, C.c_int, C.POINTER(C.c_float)]),
    "spiral_gpu_multiply": (C.c_int, [U64P, U64P, U64P, C.c_size_t, C.c_size_t, C.c_size_t]),
    "spiral_gpu_add": (C.c_int, [U64P, U64P, U64P, C.c_size_t]),
    "spiral_gpu_mul_by_const": (C.c_int, [U64P, U64P, U64P, C.c_size_t]),
    "spiral_gpu_automorph": (C.c_int, [U64P, U64P, C.c_size_t, C.c_uint64]),
    "spiral_gpu_invert": (C.c_int, [U64P, U64P, C.c_size_t]),
    "spiral_gpu_gadget_invert": (C.c_int, [U64P, U64P, C.c_size_t, C.c_size_t, C.c_size_t]),
    "spiral_gpu_get_rescaled": (C.c_int, [U64P, U64P, C.c_size_t, C.c_uint64, C.c_uint64]),
    "spiral_gpu_multiply_query_by_database": (C.c_int, [U64P, U64P, U64P, C.c_size_t, C.c_size_t]),
    "spiral_gpu_multiply_queries_by_database": (C.c_int, [U64P, U64P, C.c_size_t, U64P, C.c_size_t, C.c_size_t]),
    "spiral_gpu_split_and_crt": (C.c_int, [U64P, U64P, C.c_size_t, C.c_uint32]),
    "spiral_gpu_fold_one_further_dimension": (C.c_int, [U64P, C.c_size_t, U64P, U64P, C.c_uint32]),
    "spiral_gpu_expand_improved": (C.c_int, [U64P, C.c_uint32, C.c_uint32, U64P, C.c_uint32, U64P, C.c_uint32, C.c_uint32, C.c_uint32]),
    "spiral_gpu_scal_to_mat": (C.c_int, [U64P, U64P, U64P, C.c_uint32]),
    "spiral_gpu_regev_to_gsw": (C.c_int, [U64P, U64P, U64P, U64P, C.c_uint32, C.c_uint32]),
    "spiral_gpu_server_create": (C.c_int, [C.POINTER(Params), C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "spiral_gpu_server_create_column_shard": (C.c_int, [C.POINTER(Params), C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "spiral_gpu_server_destroy": (None, [C.c_void_p]),
    "spiral_gpu_server_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_get_stream": (C.c_void_p, [C.c_void_p]),
    "spiral_gpu_server_load_db": (C.c_int, [C.c_void_p, U64P]),
    "spiral_gpu_server_gen_db": (C.c_int, [C.c_void_p, C.c_uint64]),
    "spiral_gpu_server_fill_db_random": (C.c_int, [C.c_void_p, C.c_uint64]),
    "spiral_gpu_server_set_db_format": (C.c_int, [C.c_void_p, C.c_int]),
    "spiral_gpu_server_db_format": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_db_device_bytes": (C.c_uint64, [C.c_void_p]),
    "spiral_gpu_server_share_db": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_create_lane": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "spiral_gpu_server_first_dim_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32]),
    "spiral_gpu_server_run_query_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32]),
    "spiral_gpu_server_run_query_instances": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_answer_instances": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, U64P, U64P, U64P, C.POINTER(C.c_double)]),
    "spiral_gpu_server_run_query_batch_instances": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p), C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_answer_batch_instances": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(U64P), U64P, C.c_void_p, C.POINTER(C.c_double)]),
    "spiral_gpu_response_wire_bytes": (C.c_size_t, [C.POINTER(Params), C.c_uint32]),
    "spiral_gpu_response_from_wire": (C.c_int, [C.POINTER(Params), C.c_uint32, C.c_void_p, U64P]),
    "spiral_gpu_server_read_response_wire": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "spiral_gpu_pack_server_read_response_wire": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "spiral_gpu_server_load_db_items": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]),
    "spiral_gpu_server_update_db_items": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, U64P, C.c_uint64]),
    "spiral_gpu_db_items_bytes": (C.c_size_t, [C.POINTER(Params), C.c_uint32, C.c_uint32, C.c_uint64]),
    "spiral_gpu_server_read_db_items": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]),
    "spiral_gpu_server_read_db_items_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, U64P, C.c_uint64]),
    "spiral_gpu_server_fingerprint_items": (C.c_int, [C.c_void_p, U64P, C.c_uint64, C.c_uint64, U64P, U64P]),
    "spiral_gpu_server_fingerprint_items_at": (C.c_int, [C.c_void_p, U64P, U64P, C.c_uint64, U64P, U64P]),
    "spiral_gpu_fingerprint_host": (C.c_int, [U64P, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, U64P, U64P]),
    "spiral_gpu_fingerprint_add": (C.c_uint64, [C.c_uint64, C.c_uint64]),
    "spiral_gpu_server_fingerprint_track": (C.c_int, [C.c_void_p, U64P, U64P]),
    "spiral_gpu_server_fingerprint_untrack": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_fingerprint_tracked": (C.c_int, [C.c_void_p, U64P, U64P, U64P]),
    "spiral_gpu_server_fingerprint_tracked_polys": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, U64P]),
    "spiral_gpu_server_fingerprint_scrub": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, U64P, U64P, C.POINTER(C.c_uint32)]),
    "spiral_gpu_fingerprint_of_polys": (C.c_int, [U64P, U64P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, U64P, U64P]),
    "spiral_gpu_record_layout_of": (C.c_int, [C.POINTER(Params), C.c_uint64, C.POINTER(RecordLayout)]),
    "spiral_gpu_pack_record_layout_of": (C.c_int, [C.POINTER(Params), C.c_uint32, C.c_uint64, C.POINTER(RecordLayout)]),
    "spiral_gpu_pack_server_load_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64]),
    "spiral_gpu_pack_server_update_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, U64P, C.c_uint64]),
    "spiral_gpu_pack_server_read_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64]),
    "spiral_gpu_pack_server_read_records_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, U64P, C.c_uint64]),
    "spiral_gpu_server_load_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64]),
    "spiral_gpu_server_update_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, U64P, C.c_uint64]),
    "spiral_gpu_server_read_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64]),
    "spiral_gpu_server_read_records_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, U64P, C.c_uint64]),
    "spiral_gpu_server_read_db_item": (C.c_int, [C.c_void_p, C.c_uint64, U64P]),
    "spiral_gpu_server_read_db_slots": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, U64P]),
    "spiral_gpu_server_read_db_columns": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, U64P]),
    "spiral_gpu_server_set_pub_params": (C.c_int, [C.c_void_p, U64P, U64P, U64P, U64P]),
    "spiral_gpu_server_set_query": (C.c_int, [C.c_void_p, U64P]),
    "spiral_gpu_server_expand": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_convert": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_first_dim": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_lift": (C.c_int, [C.c_void_p, C.c_int]),
    "spiral_gpu_server_fold": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_finish": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_sync": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_use_graphs": (C.c_int, [C.c_void_p, C.c_int]),
    "spiral_gpu_server_set_overlap": (C.c_int, [C.c_void_p, C.c_int]),
    "spiral_gpu_server_run_query": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_run_pre_sweep": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_run_pre": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_run_post": (C.c_int, [C.c_void_p, C.c_int]),
    "spiral_gpu_server_set_fold_ranks": (C.c_int, [C.c_void_p, C.c_uint32]),
    "spiral_gpu_server_fold_local": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_fold_root": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_set_expand_shard": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "spiral_gpu_server_gsw_bits_words": (C.c_size_t, [C.c_void_p]),
    "spiral_gpu_server_gsw_bits_pack": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_gsw_bits_unpack": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_run_expand_pack": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_run_unpack_convert_sweep": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_run_pre_sweep_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p]),
    "spiral_gpu_server_run_expand_pack_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p]),
    "spiral_gpu_server_run_unpack_convert_sweep_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_fold_local_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_fold_root_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    # (the list of servers as an opaque pointer, as for the trial-shard calls below: tests/test_lanes_cpu.py keeps a closed table of the calls declared
    # with POINTER(c_void_p) first; this one goes through the same list check, and tests/test_column_shard_cpu.py runs that table's cases on it)
    "spiral_gpu_server_run_column_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "spiral_gpu_server_run_scal2mat_sweep": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_run_unpack_gsw": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_set_sweep_stages": (C.c_int, [C.c_void_p, C.c_uint32]),
    "spiral_gpu_server_max_sweep_stages": (C.c_uint32, [C.c_void_p]),
    "spiral_gpu_server_first_dim_stage": (C.c_int, [C.c_void_p, C.c_uint32]),
    "spiral_gpu_server_run_scal2mat": (C.c_int, [C.c_void_p]),
    "spiral_gpu_server_acc": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_size_t)]),
    "spiral_gpu_server_set_acc": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spiral_gpu_server_answer": (C.c_int, [C.c_void_p, U64P, U64P, U64P, C.POINTER(C.c_double)]),
    "spiral_gpu_server_answer_resident": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "spiral_gpu_server_keep_cts": (C.c_int, [C.c_void_p, C.c_int]),
    "spiral_gpu_server_buffer_words": (C.c_size_t, [C.c_void_p, C.c_int]),
    "spiral_gpu_server_read": (C.c_int, [C.c_void_p, C.c_int, U64P]),
    "spiral_gpu_server_write_raw": (C.c_int, [C.c_void_p, U64P]),
    "spiral_gpu_server_write_acc": (C.c_int, [C.c_void_p, U64P]),
    "spiral_gpu_server_time_sweep": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float)]),
    "spiral_gpu_server_time_sweep_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_int, C.POINTER(C.c_float)]),
    "spiral_gpu_server_sweep_bytes": (C.c_uint64, [C.c_void_p]),
    "spiral_gpu_server_sweep_device_bytes": (C.c_uint64, [C.c_void_p]),
    "spiral_gpu_pack_get_shape": (C.c_int, [C.POINTER(Params), C.c_uint32, C.POINTER(PackShape)]),
    "spiral_gpu_pack": (C.c_int, [U64P, C.c_uint32, C.c_uint32, U64P, U64P]),
    "spiral_gpu_fast_multiply_query_by_database_dim1": (C.c_int, [U64P, U64P, U64P, C.c_size_t, C.c_size_t]),
    "spiral_gpu_fast_multiply_queries_by_database_dim1": (C.c_int, [U64P, U64P, U64P, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t]),
    "spiral_gpu_pack_server_create": (C.c_int, [C.POINTER(Params), C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "spiral_gpu_pack_server_create_sharded": (C.c_int, [C.POINTER(Params), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "spiral_gpu_pack_server_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spiral_gpu_pack_server_stage_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "spiral_gpu_pack_server_fold_trials": (C.c_int, [C.c_void_p, U64P, C.c_void_p]),
    "spiral_gpu_pack_server_pack_gathered": (C.c_int, [C.c_void_p, C.c_void_p, U64P, U64P]),
    "spiral_gpu_pack_server_destroy": (None, [C.c_void_p]),
    "spiral_gpu_pack_server_gen_db": (C.c_int, [C.c_void_p, C.c_uint64]),
    "spiral_gpu_pack_server_load_db": (C.c_int, [C.c_void_p, C.c_uint32, U64P]),
    "spiral_gpu_pack_server_fill_db_random": (C.c_int, [C.c_void_p, C.c_uint64]),
    "spiral_gpu_pack_server_load_db_items": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]),
    "spiral_gpu_pack_server_update_db_items": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, U64P, C.c_uint64]),
    "spiral_gpu_pack_server_read_db_items": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]),
    "spiral_gpu_pack_server_read_db_items_at": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, U64P, C.c_uint64]),
    "spiral_gpu_pack_server_fingerprint_items": (C.c_int, [C.c_void_p, U64P, C.c_uint64, C.c_uint64, U64P, U64P]),
    "spiral_gpu_pack_server_fingerprint_items_at": (C.c_int, [C.c_void_p, U64P, U64P, C.c_uint64, U64P, U64P]),
    "spiral_gpu_pack_server_fingerprint_track": (C.c_int, [C.c_void_p, U64P, U64P]),
    "spiral_gpu_pack_server_fingerprint_untrack": (C.c_int, [C.c_void_p]),
    "spiral_gpu_pack_server_fingerprint_tracked": (C.c_int, [C.c_void_p, U64P, U64P, U64P]),
    "spiral_gpu_pack_server_fingerprint_tracked_polys": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, U64P]),
    "spiral_gpu_pack_server_fingerprint_scrub": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, U64P, U64P, C.POINTER(C.c_uint32)]),
    "spiral_gpu_pack_server_set_pub_params": (C.c_int, [C.c_void_p, U64P, U64P, U64P, U64P]),
    "spiral_gpu_pack_server_answer": (C.c_int, [C.c_void_p, U64P, U64P, U64P, C.POINTER(C.c_double)]),
    "spiral_gpu_pack_server_read_acc": (C.c_int, [C.c_void_p, C.c_uint32, U64P]),
    "spiral_gpu_pack_server_sweep_bytes": (C.c_uint64, [C.c_void_p]),
    "spiral_gpu_pack_has_limb_form": (C.c_int, [C.POINTER(Params), C.c_uint32]),
    "spiral_gpu_pack_server_create_lane": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "spiral_gpu_pack_server_answer_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(U64P), C.POINTER(U64P), C.POINTER(U64P), C.POINTER(C.c_double)]),
    "spiral_gpu_pack_server_create_shard_lane": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    # (the list of servers as an opaque pointer: tests/test_lanes_cpu.py keeps a closed table of the calls declared with POINTER(c_void_p) first; these
    # two go through the same list check, lanes.h check_lane_list, and tests/test_pack_shard_batch_cpu.py runs that table's cases on them)
    "spiral_gpu_pack_server_fold_trials_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p]),
    "spiral_gpu_pack_server_pack_gathered_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint64,
                                                             C.POINTER(U64P), C.POINTER(U64P), C.c_void_p]),
    "spiral_gpu_pack_server_set_db_format": (C.c_int, [C.c_void_p, C.c_int]),
    "spiral_gpu_pack_server_db_format": (C.c_int, [C.c_void_p]),
    "spiral_gpu_pack_server_db_device_bytes": (C.c_uint64, [C.c_void_p]),
    "spiral_gpu_pack_server_time_sweep_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_int, C.POINTER(C.c_float)]),
    "spiral_gpu_query_wire_bytes": (C.c_size_t, [C.POINTER(Params)]),
    "spiral_gpu_pub_params_wire_bytes": (C.c_size_t, [C.POINTER(Params)]),
    "spiral_gpu_pack_query_wire_bytes": (C.c_size_t, [C.POINTER(Params), C.c_uint32]),
    "spiral_gpu_pack_pub_params_wire_bytes": (C.c_size_t, [C.POINTER(Params), C.c_uint32]),
    "spiral_gpu_raw_to_wire": (C.c_int, [U64P, C.c_size_t, C.c_void_p]),
    "spiral_gpu_raw_from_wire": (C.c_int, [C.c_void_p, C.c_size_t, U64P]),
    "spiral_gpu_server_set_query_wire": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "spiral_gpu_server_set_pub_params_wire": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "spiral_gpu_pack_server_set_pub_params_wire": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "spiral_gpu_pack_server_answer_wire": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, U64P, U64P, C.POINTER(C.c_double)]),
    "spiral_gpu_pack_server_answer_batch_wire": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(U64P), C.POINTER(U64P), C.POINTER(C.c_double)]),
    "spiral_gpu_pack_server_answer_batch_instances": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(U64P), U64P, C.c_void_p, C.POINTER(C.c_double)]),
    "spiral_gpu_pack_server_answer_batch_instances_wire": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p), C.c_size_t, U64P, C.c_void_p, C.POINTER(C.c_double)]),
    "spiral_gpu_query_seeded_bytes": (C.c_size_t, [C.POINTER(Params)]),
    "spiral_gpu_pub_params_seeded_bytes": (C.c_size_t, [C.POINTER(Params)]),
    "spiral_gpu_pack_query_seeded_bytes": (C.c_size_t, [C.POINTER(Params), C.c_uint32]),
    "spiral_gpu_pack_pub_params_seeded_bytes": (C.c_size_t, [C.POINTER(Params), C.c_uint32]),
    "spiral_gpu_seed_expand": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t, U64P]),
    "spiral_gpu_server_set_query_seeded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "spiral_gpu_server_set_pub_params_seeded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "spiral_gpu_pack_server_set_pub_params_seeded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "spiral_gpu_pack_server_answer_seeded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, U64P, U64P, C.POINTER(C.c_double)]),
    "spiral_gpu_pack_server_answer_batch_seeded": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(U64P), C.POINTER(U64P), C.POINTER(C.c_double)]),
    "spiral_gpu_pack_server_answer_batch_instances_seeded": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p), C.c_size_t, U64P, C.c_void_p, C.POINTER(C.c_double)]),
    "spiral_gpu_key_store_create": (C.c_int, [C.POINTER(Params), C.c_uint32, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_void_p)]),
    "spiral_gpu_key_store_destroy": (None, [C.c_void_p]),
    "spiral_gpu_key_store_slot_bytes": (C.c_size_t, [C.POINTER(Params), C.c_uint32, C.c_int]),
    "spiral_gpu_key_store_put": (C.c_int, [C.c_void_p, C.c_uint32, U64P, U64P, U64P, U64P]),
    "spiral_gpu_key_store_put_wire": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "spiral_gpu_key_store_put_seeded": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "spiral_gpu_key_store_drop": (C.c_int, [C.c_void_p, C.c_uint32]),
    "spiral_gpu_key_store_has": (C.c_int, [C.c_void_p, C.c_uint32]),
    "spiral_gpu_server_bind_keys": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    "spiral_gpu_pack_server_bind_keys": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    "spiral_gpu_server_set_query_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_int, C.POINTER(C.c_void_p), C.c_size_t]),
    "spiral_gpu_server_read_response_wire_batch": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_size_t]),
    "spiral_gpu_client_noise_table": (C.c_int, [U64P]),
    "spiral_gpu_client_create": (C.c_int, [C.POINTER(Params), C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "spiral_gpu_client_destroy": (None, [C.c_void_p]),
    "spiral_gpu_client_get_secret": (C.c_int, [C.c_void_p, U64P, U64P]),
    "spiral_gpu_client_set_secret": (C.c_int, [C.c_void_p, U64P, U64P]),
    "spiral_gpu_client_get_counter": (C.c_int, [C.c_void_p, U64P]),
    "spiral_gpu_client_set_counter": (C.c_int, [C.c_void_p, C.c_uint64]),
    "spiral_gpu_client_pub_params": (C.c_int, [C.c_void_p, U64P, U64P, U64P, U64P]),
    "spiral_gpu_client_pub_params_msg": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "spiral_gpu_client_queries": (C.c_int, [C.c_void_p, U64P, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]),
    "spiral_gpu_client_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, U64P]),
    "spiral_gpu_kv_layout_of": (C.c_int, [C.POINTER(Params), C.c_uint64, C.POINTER(KvLayout)]),
    "spiral_gpu_kv_hash": (C.c_int, [C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_uint64, U64P, U64P, U64P]),
    "spiral_gpu_server_kv_load": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]),
    "spiral_gpu_server_kv_put": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]),
    "spiral_gpu_server_kv_delete": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, U64P]),
    "spiral_gpu_server_kv_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "spiral_gpu_server_kv_stats": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(KvStatsStruct)]),
    "spiral_gpu_pack_kv_layout_of": (C.c_int, [C.POINTER(Params), C.c_uint32, C.c_uint64, C.POINTER(KvLayout)]),
    "spiral_gpu_pack_kv_hash": (C.c_int, [C.POINTER(Params), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, U64P, U64P, U64P]),
    "spiral_gpu_pack_server_kv_load": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]),
    "spiral_gpu_pack_server_kv_put": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]),
    "spiral_gpu_pack_server_kv_delete": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, U64P]),
    "spiral_gpu_pack_server_kv_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "spiral_gpu_pack_server_kv_stats": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(KvStatsStruct)]),
    "spiral_gpu_server_kv_scan": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, U64P]),
    "spiral_gpu_server_kv_scan_at": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, U64P]),
    "spiral_gpu_pack_server_kv_scan": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, U64P]),
    "spiral_gpu_pack_server_kv_scan_at": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, U64P]),
    "spiral_gpu_kv_reconcile": (C.c_int, [C.POINTER(Params), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                          C.POINTER(KvReconcileCounts)]),
    "spiral_gpu_client_kv_queries": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]),
    "spiral_gpu_client_kv_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p]),
    "spiral_gpu_client_record_queries": (C.c_int, [C.c_void_p, C.c_uint64, U64P, C.c_uint32, C.c_int, C.c_void_p, C.c_size_t]),
    "spiral_gpu_client_decode_records": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint64, U64P, C.c_void_p]),
    "spiral_gpu_client_response_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, U64P, U64P, C.POINTER(C.c_int64)]),
}


def build(force: bool = False) -> str:
    """hipcc-compile the HIP extension for gfx950 (works without a GPU)."""
    args = ["make", "-C", CSRC, "-s", "-j4"]
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(args)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the HIP extension must be built (python -c 'import __graft_entry__ as g; g.build()'); "
                "there is no CPU fallback"
            )
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            fn.restype = res
            fn.argtypes = args
        if L.spiral_gpu_abi_version() != 1:
            raise RuntimeError("libspiral_gpu.so ABI version mismatch")
        _lib = L
    return _lib


class SpiralGpuError(RuntimeError):
    pass


def check(rc: int) -> None:
    if rc != 0:
        raise SpiralGpuError(lib().spiral_gpu_last_error().decode() or f"error {rc}")


WIRE_POLY_BYTES = 7 * 2048  # one polynomial of a query / public-parameter message in its wire form (include/spiral_gpu.h)
SEED_BYTES = 32  # the seed that opens a message in its seeded form
FORM_NTT, FORM_WIRE, FORM_SEEDED = 0, 1, 2  # spiral_gpu_message_form (the NTT form is no message: the batch ingest refuses it by name)
SEED_QUERY, SEED_PUB_PARAMS, SEED_PACK_QUERY, SEED_PACK_PUB_PARAMS = 1, 2, 3, 4  # the seeded form's domain tags


def wire_bytes(wire) -> np.ndarray:
    """a wire message (bytes, bytearray, memoryview or an array) as one contiguous uint8 array"""
    if isinstance(wire, (bytes, bytearray, memoryview)):
        return np.frombuffer(wire, dtype=np.uint8)
    wire = np.ascontiguousarray(wire)
    if wire.dtype != np.uint8:
        raise TypeError(f"a wire message is bytes or a uint8 array, not {wire.dtype}")
    return wire.reshape(-1)


def db_items_bytes(params: Params, coeff_bits: int, n_items: int, out_n: int = 0) -> int:
    """bytes of n_items plaintexts in the item stream of load_db_items / read_db_items: 4 polynomials per item of a base server (out_n = 0), one per
    item of a SpiralPack trial (out_n >= 1); raises for a coefficient width outside 1..64 or too narrow for p_db"""
    if not isinstance(coeff_bits, (int, np.integer)) or isinstance(coeff_bits, bool) or not 0 <= coeff_bits < 2**32:
        raise ValueError(f"coeff_bits = {coeff_bits!r} is not in 1..64")
    n = lib().spiral_gpu_db_items_bytes(C.byref(params), out_n, int(coeff_bits), n_items)
    if n == 0 and n_items:
        raise SpiralGpuError(lib().spiral_gpu_last_error().decode())
    return n


def record_layout(params: Params, record_bytes: int, out_n: int = 0) -> RecordLayout:
    """the layout of records of record_bytes bytes in the plaintexts of `params` (out_n = 0: a base server's; out_n >= 1: the out_n^2 trial images of a
    SpiralPack server's), host only; raises for a size of 0 or one that takes more than 16 instances"""
    if not isinstance(record_bytes, (int, np.integer)) or isinstance(record_bytes, bool) or not 0 <= record_bytes < 2**64:
        raise ValueError(f"record_bytes = {record_bytes!r} is no byte count")
    if not isinstance(out_n, (int, np.integer)) or isinstance(out_n, bool) or not 0 <= out_n < 2**32:
        raise ValueError(f"out_n = {out_n!r} is no SpiralPack dimension")
    out = RecordLayout()
    if out_n:
        check(lib().spiral_gpu_pack_record_layout_of(C.byref(params), int(out_n), int(record_bytes), C.byref(out)))
    else:
        check(lib().spiral_gpu_record_layout_of(C.byref(params), int(record_bytes), C.byref(out)))
    return out


# ---- keyed records (include/spiral_gpu.h "Keyed records") ----
def kv_layout(params: Params, value_bytes: int, out_n: int = 0) -> KvLayout:
    """the layout of keyed records with values of value_bytes bytes in the buckets of `params`, host only; raises for a value size the definition
    refuses (slots = 0, slots > 256, a header beyond polynomial 0) and for fewer than 2 buckets.  This is the layout of a BASE parameter set (buckets
    of 4 polynomials), as spiral_gpu_kv_layout_of: out_n >= 1 is refused by name -- a SpiralPack set has pack_kv_layout, as the C ABI has
    spiral_gpu_pack_kv_layout_of"""
    if not isinstance(value_bytes, (int, np.integer)) or isinstance(value_bytes, bool) or not 0 <= value_bytes < 2**64:
        raise ValueError(f"value_bytes = {value_bytes!r} is no byte count")
    if out_n:
        raise SpiralGpuError(f"kv_layout is the layout of base parameter sets only (out_n = 0); for a SpiralPack set with out_n = {out_n} call "
                             f"pack_kv_layout(params, out_n, value_bytes)")
    out = KvLayout()
    check(lib().spiral_gpu_kv_layout_of(C.byref(params), int(value_bytes), C.byref(out)))
    return out


def pack_kv_layout(params: Params, out_n: int, value_bytes: int) -> KvLayout:
    """kv_layout for a SpiralPack parameter set with out_n in 1 .. 16: a bucket is an item of out_n^2 polynomials, one per trial image (include/spiral_gpu.h
    "Keyed records", SpiralPack), host only; the same refusals"""
    if not isinstance(value_bytes, (int, np.integer)) or isinstance(value_bytes, bool) or not 0 <= value_bytes < 2**64:
        raise ValueError(f"value_bytes = {value_bytes!r} is no byte count")
    if not isinstance(out_n, (int, np.integer)) or isinstance(out_n, bool) or not 0 <= out_n < 2**32:
        raise ValueError(f"out_n = {out_n!r} is no SpiralPack dimension")
    out = KvLayout()
    check(lib().spiral_gpu_pack_kv_layout_of(C.byref(params), int(out_n), int(value_bytes), C.byref(out)))
    return out


def kv_layout_for(params: Params, value_bytes: int, out_n: int) -> KvLayout:
    """the layout a server or session with this out_n uses (0: base)"""
    return pack_kv_layout(params, out_n, value_bytes) if out_n else kv_layout(params, value_bytes)


def kv_table_key(table_key) -> np.ndarray:
    """the 16-byte table key as a uint8 array"""
    key = np.frombuffer(bytes(table_key), dtype=np.uint8) if isinstance(table_key, (bytes, bytearray, memoryview)) else np.ascontiguousarray(table_key)
    if key.dtype != np.uint8 or key.size != 16:
        raise ValueError("the table key is 16 bytes (bytes or a uint8 array)")
    return np.ascontiguousarray(key.reshape(16))


def kv_keys(keys) -> np.ndarray:
    """the keys of a call as one contiguous uint8 array [n][key_bytes]: a 2-D uint8 array, or a list of bytes of equal length"""
    if isinstance(keys, np.ndarray):
        if keys.dtype != np.uint8 or keys.ndim != 2:
            raise TypeError("keys are a 2-D uint8 array [n][key_bytes] or a list of bytes of equal length")
        return np.ascontiguousarray(keys)
    keys = [bytes(k) for k in keys]
    if len({len(k) for k in keys}) > 1:
        raise ValueError("the keys of one call have one length")
    width = len(keys[0]) if keys else 0
    return np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), width).copy()


def kv_hash(params: Params, table_key, key, out_n: int = 0) -> tuple[int, int, int]:
    """(tag, b1, b2) of one key under the 16-byte table key: the definition's SipHash-2-4 values, host only (out_n >= 1: a SpiralPack set, spiral_gpu_pack_kv_hash; the values depend
    on nu1 + nu2 alone)"""
    tk = kv_table_key(table_key)
    kb = np.frombuffer(bytes(key), dtype=np.uint8)
    tag, b1, b2 = C.c_uint64(), C.c_uint64(), C.c_uint64()
    args = (tk.ctypes.data_as(C.c_void_p), kb.ctypes.data_as(C.c_void_p) if kb.size else None, kb.size, C.byref(tag), C.byref(b1), C.byref(b2))
    if out_n:
        check(lib().spiral_gpu_pack_kv_hash(C.byref(params), int(out_n), *args))
    else:
        check(lib().spiral_gpu_kv_hash(C.byref(params), *args))
    return tag.value, b1.value, b2.value


@dataclass(frozen=True)
class KvStats:
    """the occupancy of a range of buckets of a keyed table (include/spiral_gpu.h, spiral_gpu_server_kv_stats): hist[u] = buckets with exactly u used
    slots, u = 0 .. slots"""

    buckets: int
    used: int
    full_buckets: int
    max_used: int
    slots: int
    hist: tuple

    def load(self) -> float:
        """used / (buckets * slots); 0.0 for an empty range"""
        return self.used / (self.buckets * self.slots) if self.buckets else 0.0


class KvScanOverflow(SpiralGpuError):
    """a listing that holds more entries than max_entries: .count is the number of entries in the buckets named; nothing was written"""

    def __init__(self, message: str, count: int, max_entries: int):
        super().__init__(message)
        self.count, self.max_entries = count, max_entries


@dataclass(frozen=True)
class KvScan:
    """a listing (include/spiral_gpu.h "Listing"): the entries -- slots whose tag is not 0 -- of a set of buckets, in the order of the buckets and within
    a bucket by ascending slot; values[k] (where asked for) is the value of entry k.  first_bucket / n_buckets: the range of a kv_scan, None for a
    kv_scan_at; table_buckets: nb of the table listed"""

    tags: np.ndarray  # uint64 [n]
    buckets: np.ndarray  # uint32 [n]
    slots: np.ndarray  # uint32 [n]
    values: np.ndarray | None  # uint8 [n][V]
    first_bucket: int | None
    n_buckets: int | None
    table_buckets: int

    def __len__(self) -> int:
        return len(self.tags)

    def entries(self) -> np.ndarray:
        """the entries as the structured array (tag u64, bucket u32, slot u32) that spiral_gpu_kv_reconcile takes"""
        out = np.empty(len(self.tags), dtype=KV_ENTRY_DTYPE)
        out["tag"], out["bucket"], out["slot"] = self.tags, self.buckets, self.slots
        return out


class KeyedRecords:
    """the keyed-record calls of Server and PackServer (include/spiral_gpu.h "Keyed records"): a bucket is an item, a key hashes to two candidate
    buckets.  The class says which library calls are its own (_kv_prefix); out_n (PackServer) selects the SpiralPack layout"""

    def _kv(self, name: str):
        return getattr(lib(), f"{self._kv_prefix}_kv_{name}")

    def _kv_args(self, table_key, keys, values=None, value_bytes=None):
        tk, keys = kv_table_key(table_key), kv_keys(keys)
        if values is not None:
            values = np.ascontiguousarray(values)
            if values.dtype != np.uint8 or values.ndim != 2 or values.shape[0] != keys.shape[0]:
                raise ValueError(f"values are a uint8 array [n][value_bytes] with one row per key ({keys.shape[0]})")
            value_bytes = values.shape[1]
        kv_layout_for(self.params, value_bytes, getattr(self, "out_n", 0))
        kp = keys.ctypes.data_as(C.c_void_p) if keys.size else None
        return tk, keys, kp, values, int(value_bytes)

    def kv_load(self, table_key, keys, values):
        """a fresh keyed table from keys [n][key_bytes] and values [n][value_bytes]: placed from empty on the host, loaded through load_db_items (a
        SpiralPack server: every trial image)"""
        tk, keys, kp, values, vb = self._kv_args(table_key, keys, values)
        check(self._kv("load")(self.h, tk.ctypes.data_as(C.c_void_p), kp, keys.shape[1], values.ctypes.data_as(C.c_void_p), vb, keys.shape[0]))
        return self

    def kv_put(self, table_key, keys, values):
        """insert or overwrite keys in place, in the image's current form: one probe launch, the placement rule on the host, update_records' write;
        fails with nothing written where a key's two buckets are full; see include/spiral_gpu.h spiral_gpu_server_kv_put"""
        tk, keys, kp, values, vb = self._kv_args(table_key, keys, values)
        check(self._kv("put")(self.h, tk.ctypes.data_as(C.c_void_p), kp, keys.shape[1], values.ctypes.data_as(C.c_void_p), vb, keys.shape[0]))

    def kv_delete(self, table_key, keys, value_bytes: int) -> int:
        """zero tag and value of every key that is present; returns how many were (an absent key is not an error)"""
        tk, keys, kp, _, vb = self._kv_args(table_key, keys, None, value_bytes)
        n = C.c_uint64()
        check(self._kv("delete")(self.h, tk.ctypes.data_as(C.c_void_p), kp, keys.shape[1], vb, keys.shape[0], C.byref(n)))
        return n.value

    def kv_get(self, table_key, keys, value_bytes: int, out: np.ndarray | None = None):
        """(values uint8 [n][value_bytes], found uint8 [n]): found[k] is 0 (absent), 1 or 2 (the candidate bucket that holds the key); the bytes of an
        absent key are left as they are in `out` (zero in a fresh array).  Any server that references the image, lanes included"""
        tk, keys, kp, _, vb = self._kv_args(table_key, keys, None, value_bytes)
        out = record_out(vb, keys.shape[0], out)
        found = np.zeros(keys.shape[0], dtype=np.uint8)
        check(self._kv("get")(self.h, tk.ctypes.data_as(C.c_void_p), kp, keys.shape[1], out.ctypes.data_as(C.c_void_p), vb, keys.shape[0],
                              found.ctypes.data_as(C.c_void_p)))
        return out.reshape(keys.shape[0], vb), found

    def kv_stats(self, value_bytes: int, first_bucket: int = 0, n_buckets: int | None = None) -> KvStats:
        """how full buckets [first_bucket, first_bucket + n_buckets) are (n_buckets None: to the table's end): one launch, a histogram of used slots
        per bucket comes back, not the headers.  Any server that references the image, lanes included"""
        lay = kv_layout_for(self.params, value_bytes, getattr(self, "out_n", 0))
        if n_buckets is None:
            n_buckets = max(lay.buckets - first_bucket, 0)
        out = KvStatsStruct()
        check(self._kv("stats")(self.h, int(value_bytes), int(first_bucket), int(n_buckets), C.byref(out)))
        return KvStats(int(out.buckets), int(out.used), int(out.full_buckets), int(out.max_used), int(out.slots), tuple(int(x) for x in out.hist))

    def _kv_scan(self, name, value_bytes, head, values, max_entries, out_entries, out_values, about):
        """the shared body of kv_scan and kv_scan_at; head: the call's arguments between value_bytes and entries"""
        lay = kv_layout_for(self.params, value_bytes, getattr(self, "out_n", 0))
        vb, fn, n = int(value_bytes), self._kv(name), C.c_uint64()
        if max_entries is None:  # a count-only call first, then exactly that many entries
            check(fn(self.h, vb, *head, None, None, 0, C.byref(n)))
            max_entries = n.value
        max_entries = int(max_entries)
        ent = np.zeros(max_entries, dtype=KV_ENTRY_DTYPE) if out_entries is None else out_entries
        if ent.dtype != KV_ENTRY_DTYPE or ent.ndim != 1 or len(ent) < max_entries or not ent.flags.c_contiguous:
            raise ValueError(f"out_entries is a contiguous array of at least max_entries = {max_entries} records of {KV_ENTRY_DTYPE}")
        val = None
        if values:
            val = np.zeros((max_entries, vb), dtype=np.uint8) if out_values is None else out_values
            if val.dtype != np.uint8 or val.shape[1:] != (vb,) or len(val) < max_entries or not val.flags.c_contiguous:
                raise ValueError(f"out_values is a contiguous uint8 array [at least max_entries = {max_entries}][{vb}]")
        rc = fn(self.h, vb, *head, ent.ctypes.data_as(C.c_void_p) if max_entries else None, val.ctypes.data_as(C.c_void_p) if values and max_entries else None,
                max_entries, C.byref(n))
        if rc != 0:
            message = lib().spiral_gpu_last_error().decode()
            if n.value > max_entries:
                raise KvScanOverflow(message, n.value, max_entries)
            raise SpiralGpuError(message)
        if n.value > max_entries:  # (max_entries = 0 is the C call's count-only form: it succeeds)
            raise KvScanOverflow(f"{name}: the buckets named hold {n.value} entries, max_entries is {max_entries}; nothing was written", n.value, max_entries)
        ent = ent[:n.value]
        return KvScan(ent["tag"].copy(), ent["bucket"].copy(), ent["slot"].copy(), val[:n.value] if values else None, *about, int(lay.buckets))

    def kv_scan(self, value_bytes: int, first_bucket: int = 0, n_buckets: int | None = None, values: bool = True, max_entries: int | None = None, *,
                out_entries: np.ndarray | None = None, out_values: np.ndarray | None = None) -> KvScan:
        """the listing of buckets [first_bucket, first_bucket + n_buckets) (n_buckets None: to the table's end), compacted on the device: only live
        entries come back, with their values unless values=False.  max_entries None: a count-only call first, then exactly that many; an explicit
        max_entries is passed through, and a listing that holds more raises KvScanOverflow (.count) with nothing written.  out_entries / out_values: the
        caller's buffers (KV_ENTRY_DTYPE [max_entries], uint8 [max_entries][V]) in place of fresh ones.  Any server that references the image, lanes
        included"""
        lay = kv_layout_for(self.params, value_bytes, getattr(self, "out_n", 0))
        if n_buckets is None:
            n_buckets = max(lay.buckets - first_bucket, 0)
        head = (int(first_bucket), int(n_buckets))
        return self._kv_scan("scan", value_bytes, head, values, max_entries, out_entries, out_values, head)

    def kv_scan_at(self, value_bytes: int, buckets, values: bool = True, max_entries: int | None = None, *, out_entries: np.ndarray | None = None,
                   out_values: np.ndarray | None = None) -> KvScan:
        """the listing of the buckets of a list, in the order of the list (a bucket named twice is listed twice; .buckets are bucket ids); otherwise as
        kv_scan"""
        ids = np.ascontiguousarray(buckets, dtype=np.uint64).reshape(-1)
        head = (ids.ctypes.data_as(C.c_void_p) if ids.size else None, ids.size)
        return self._kv_scan("scan_at", value_bytes, head, values, max_entries, out_entries, out_values, (None, None))


@dataclass(frozen=True)
class KvReconcile:
    """spiral_gpu_kv_reconcile's result: where[k] = the entry a lookup of key k finds, or -1; entry_class[e] = 0 held, 1 shadowed, 2 misplaced, 3 orphan;
    and the totals"""

    where: np.ndarray  # int64 [n_keys]
    entry_class: np.ndarray  # uint8 [n_entries]
    held: int
    missing: int
    shadowed: int
    misplaced: int
    orphans: int

    def missing_keys(self) -> np.ndarray:
        """positions of the keys no lookup finds"""
        return np.flatnonzero(self.where < 0)

    def orphan_entries(self) -> np.ndarray:
        """positions of the entries whose tag belongs to no key given"""
        return np.flatnonzero(self.entry_class == 3)

    def misplaced_entries(self) -> np.ndarray:
        """positions of the entries that carry a key's tag in a bucket that is neither of its candidates"""
        return np.flatnonzero(self.entry_class == 2)


def kv_reconcile(params: Params, table_key, keys, scan: KvScan) -> KvReconcile:
    """a listing of the WHOLE table against a key set (spiral_gpu_kv_reconcile; host only, base and SpiralPack parameter sets alike): which keys are
    missing, which entries are held, shadowed, misplaced or orphans.  A KvScan that does not cover [0, table_buckets) is refused"""
    if scan.first_bucket != 0 or scan.n_buckets != scan.table_buckets:
        what = "a kv_scan_at listing" if scan.first_bucket is None else f"buckets [{scan.first_bucket}, +{scan.n_buckets})"
        raise SpiralGpuError(f"kv_reconcile takes a listing of the whole table, buckets [0, {scan.table_buckets}): this one is {what}")
    tk, keys, ent = kv_table_key(table_key), kv_keys(keys), scan.entries()
    where, cls, counts = np.empty(keys.shape[0], dtype=np.int64), np.empty(len(ent), dtype=np.uint8), KvReconcileCounts()
    check(lib().spiral_gpu_kv_reconcile(C.byref(params), tk.ctypes.data_as(C.c_void_p), keys.ctypes.data_as(C.c_void_p) if keys.size else None, keys.shape[1],
                                        keys.shape[0], ent.ctypes.data_as(C.c_void_p) if len(ent) else None, len(ent), where.ctypes.data_as(C.c_void_p),
                                        cls.ctypes.data_as(C.c_void_p), C.byref(counts)))
    return KvReconcile(where, cls, int(counts.held), int(counts.missing), int(counts.shadowed), int(counts.misplaced), int(counts.orphans))


def record_array(records, record_bytes: int, n: int | None = None) -> np.ndarray:
    """the records of a load_records / update_records call as one contiguous uint8 array of whole records (n of them, where n is given)"""
    if isinstance(records, (bytes, bytearray, memoryview)):
        records = np.frombuffer(records, dtype=np.uint8)
    records = np.ascontiguousarray(records)
    if records.dtype != np.uint8:
        raise TypeError(f"records are bytes or a uint8 array, not {records.dtype}")
    if records.size % record_bytes or (n is not None and records.size != n * record_bytes):
        raise ValueError(f"records holds {records.size} bytes: not {'whole' if n is None else n} records of {record_bytes} bytes")
    return records.reshape(-1)


def record_out(record_bytes: int, n: int, out) -> np.ndarray:
    """the output buffer of a read_records call: a fresh zeroed uint8 array [n][record_bytes], or the caller's `out` of exactly that size (shards and
    instance servers fill one buffer)"""
    if out is None:
        return np.zeros((n, record_bytes), dtype=np.uint8)
    if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable and out.size == n * record_bytes):
        raise ValueError(f"out must be a writable contiguous uint8 array of {n * record_bytes} bytes")
    return out


def read_args(params: Params, coeff_bits: int, n_items: int, out_n: int, out):
    """the output buffer of a read_db_items call: a fresh zeroed uint8 array of n_items plaintexts, or the caller's `out` (a contiguous uint8 array of
    exactly that size: the shards of a database fill one buffer, each its own items)"""
    nbytes = db_items_bytes(params, coeff_bits, n_items, out_n)
    if out is None:
        return np.zeros(nbytes, dtype=np.uint8)
    if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.flags.writeable and out.size == nbytes):
        raise ValueError(f"out must be a writable contiguous uint8 array of {nbytes} bytes")
    return out


def read_ids(item_ids) -> np.ndarray:
    """the id list of a read_db_items_at call (duplicates and any order are fine) -> uint64"""
    ids = np.asarray(item_ids)
    if ids.ndim != 1:
        raise ValueError("item_ids must be a flat list of item indices")
    if ids.size and ids.dtype.kind not in "iu":
        raise TypeError(f"item_ids must be integers, not {ids.dtype}")
    if ids.size and ids.dtype.kind == "i" and (ids < 0).any():
        raise ValueError("item_ids must be non-negative")
    return np.ascontiguousarray(ids, dtype=np.uint64)


# ---- fingerprints (include/spiral_gpu.h "Fingerprints") ----
FINGERPRINT_MODULUS = 2**61 - 1


def _is_int(v, lo: int, hi: int) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= int(v) < hi


def fingerprint_key(key):
    """a fingerprint key, a pair of ints in [0, 2^64), as the uint64[2] the library takes"""
    if isinstance(key, (str, bytes)) or not hasattr(key, "__len__") or len(key) != 2 or not all(_is_int(k, 0, 2**64) for k in key):
        raise ValueError(f"a fingerprint key is a pair of ints in [0, 2^64), not {key!r}")
    return (C.c_uint64 * 2)(int(key[0]), int(key[1]))


def fingerprint_call(fn, head: tuple, n: int, per_item: bool):
    """one fingerprint call of the library: fn(*head, per_item[n] or NULL, &combined) -> F, or (F, per-item uint64 array)"""
    items = np.zeros(n, dtype=np.uint64) if per_item else None
    combined = C.c_uint64(0)
    check(fn(*head, items.ctypes.data_as(U64P) if per_item else None, C.byref(combined)))
    return (int(combined.value), items) if per_item else int(combined.value)


def fingerprint_range(first_item, n_items, total: int):
    """the item range of a fingerprint_items call (n_items None: to the end of the database of `total` items)"""
    if not _is_int(first_item, 0, 2**64):
        raise ValueError(f"first_item = {first_item!r} is no item index")
    if n_items is None:
        n_items = max(total - int(first_item), 0)
    if not _is_int(n_items, 0, 2**64):
        raise ValueError(f"n_items = {n_items!r} is no item count")
    if int(first_item) + int(n_items) > total:  # (the library's own refusal, before an output of that many words is allocated)
        raise SpiralGpuError(f"items [{int(first_item)}, +{int(n_items)}) outside the database of {total}")
    return int(first_item), int(n_items)


def fingerprint_host(key, p_db: int, items, coeff_bits: int, polys_per_item: int = 4, poly0: int = 0, n_polys=None, first_item: int = 0, per_item: bool = False):
    """the fingerprint of a bit-packed item stream, computed on the host (no GPU): `items` holds, for consecutive items from database index first_item,
    the polynomials poly0 .. poly0 + n_polys - 1 (default: to the last) of an item of polys_per_item, coeff_bits wide as load_db_items takes them.
    Returns F, or (F, the per-item values as a uint64 array) with per_item; see include/spiral_gpu.h "Fingerprints" """
    k = fingerprint_key(key)
    for name, v, lo, hi in (("p_db", p_db, 0, 2**64), ("coeff_bits", coeff_bits, 0, 2**32), ("polys_per_item", polys_per_item, 0, 2**32),
                            ("poly0", poly0, 0, 2**32), ("first_item", first_item, 0, 2**64)):
        if not _is_int(v, lo, hi):
            raise ValueError(f"{name} = {v!r} is out of range")
    if n_polys is None:
        n_polys = max(int(polys_per_item) - int(poly0), 0)
    if not _is_int(n_polys, 0, 2**32):
        raise ValueError(f"n_polys = {n_polys!r} is out of range")
    if isinstance(items, (bytes, bytearray, memoryview)):
        items = np.frombuffer(items, dtype=np.uint8)
    items = np.ascontiguousarray(items)
    if items.dtype == np.uint64 and coeff_bits != 64:
        raise TypeError("a uint64 item array holds 64-bit coefficients: pass coeff_bits = 64, or the bit-packed stream as uint8")
    if items.dtype not in (np.uint8, np.uint64):
        raise TypeError(f"items are bytes, a uint8 array or (coeff_bits = 64) a uint64 array, not {items.dtype}")
    if not 1 <= int(coeff_bits) <= 64:
        raise ValueError(f"coeff_bits = {coeff_bits!r} is not in 1..64")
    item_bytes = int(n_polys) * 256 * int(coeff_bits)
    if item_bytes == 0 or items.nbytes % item_bytes:
        raise ValueError(f"items holds {items.nbytes} bytes: not whole items of {n_polys} polynomials of 2048 {coeff_bits}-bit coefficients")
    n = items.nbytes // item_bytes
    head = (k, int(p_db), items.ctypes.data_as(C.c_void_p), int(coeff_bits), int(polys_per_item), int(poly0), int(n_polys), int(first_item), n)
    return fingerprint_call(lib().spiral_gpu_fingerprint_host, head, n, per_item)


def fingerprint_add(*parts) -> int:
    """the sum mod P = 2^61 - 1 of fingerprints (the partials of shards, or of adjoining ranges); raises for a value outside [0, P)"""
    total = 0
    for v in parts:
        if not _is_int(v, 0, FINGERPRINT_MODULUS):
            raise ValueError(f"{v!r} is no fingerprint: an int in [0, 2^61 - 1)")
        total = int(lib().spiral_gpu_fingerprint_add(total, int(v)))
    return total


def fingerprint_of_polys(key, poly_sums, polys_per_item: int = 4, poly0: int = 0, n_polys=None, first_item: int = 0, per_item: bool = False):
    """f and F from a table of polynomial sums g, on the host (no GPU): poly_sums[k][q] = g(first_item + k, poly0 + q) for the polynomials poly0 ..
    poly0 + n_polys - 1 (default: to the last) of an item of polys_per_item.  Returns F, or (F, the per-item values as a uint64 array) with per_item;
    see include/spiral_gpu.h "Fingerprints", Tracked"""
    k = fingerprint_key(key)
    for name, v, hi in (("polys_per_item", polys_per_item, 2**32), ("poly0", poly0, 2**32), ("first_item", first_item, 2**64)):
        if not _is_int(v, 0, hi):
            raise ValueError(f"{name} = {v!r} is out of range")
    if n_polys is None:
        n_polys = max(int(polys_per_item) - int(poly0), 0)
    if not _is_int(n_polys, 0, 2**32):
        raise ValueError(f"n_polys = {n_polys!r} is out of range")
    g = np.ascontiguousarray(poly_sums)
    if g.dtype != np.uint64:
        raise TypeError(f"polynomial sums are a uint64 array, not {g.dtype}")
    if int(n_polys) == 0 or g.size % int(n_polys):
        raise ValueError(f"poly_sums holds {g.size} words: not whole items of {n_polys} polynomials")
    n = g.size // int(n_polys)
    head = (k, g.ctypes.data_as(U64P), int(polys_per_item), int(poly0), int(n_polys), int(first_item), n)
    return fingerprint_call(lib().spiral_gpu_fingerprint_of_polys, head, n, per_item)


class TrackedFingerprint:
    """the tracked-fingerprint calls of Server and PackServer (include/spiral_gpu.h "Fingerprints", Tracked).  The class says which library calls are
    its own (_fp_prefix) and what its table holds (_fp_table: local items, polynomials held of an item, items of the database)"""

    def _fp(self, name: str):
        return getattr(lib(), f"{self._fp_prefix}_fingerprint_{name}")

    def fingerprint_track(self, key, poly_sums=None):
        """start tracking under `key`: the table of polynomial sums and F computed from the image in its current form, or, with poly_sums (a uint64
        array, [local item][polynomial held], as fingerprint_tracked_polys of an unsharded or equally sharded server returns it), adopted without
        reading the image.  The update calls keep both current; every loader ends tracking.  Owner only"""
        k = fingerprint_key(key)
        if poly_sums is None:
            check(self._fp("track")(self.h, k, None))
            return
        g = np.ascontiguousarray(poly_sums)
        items, polys, _ = self._fp_table()
        if g.dtype != np.uint64 or g.size != items * polys:
            raise ValueError(f"poly_sums must be {items} x {polys} uint64 words (local items x polynomials held), not {g.size} of {g.dtype}")
        check(self._fp("track")(self.h, k, g.ctypes.data_as(U64P)))

    def fingerprint_untrack(self):
        check(self._fp("untrack")(self.h))

    def fingerprint_tracked(self):
        """(F, n_updates): the tracked combined fingerprint of what this server holds after everything enqueued on its stream, and the number of
        polynomials whose table word the update calls have replaced since fingerprint_track.  Raises when the image is not tracked"""
        F, n = C.c_uint64(0), C.c_uint64(0)
        check(self._fp("tracked")(self.h, None, C.byref(F), C.byref(n)))
        return int(F.value), int(n.value)

    def fingerprint_tracked_key(self):
        """the key the image is tracked under, as a pair of ints"""
        k = (C.c_uint64 * 2)()
        check(self._fp("tracked")(self.h, k, None, None))
        return int(k[0]), int(k[1])

    def fingerprint_tracked_polys(self, first_item: int = 0, n_items=None) -> np.ndarray:
        """the table's words g of database items first_item .. (default: to the end) as a uint64 array [item][polynomial held]; a j-shard or column
        shard returns 0 for an item it does not hold, so the shards' arrays add to the unsharded table"""
        _, polys, total = self._fp_table()
        first_item, n_items = fingerprint_range(first_item, n_items, total)
        out = np.zeros((n_items, polys), dtype=np.uint64)
        check(self._fp("tracked_polys")(self.h, first_item, n_items, out.ctypes.data_as(U64P)))
        return out

    def fingerprint_scrub(self, first_item: int = 0, n_items=None):
        """recompute the polynomial sums of a range from the image in its current form and compare them with the table on the device:
        (n_bad, first_bad) with first_bad = None, or the lowest (database item, polynomial) that differs"""
        _, _, total = self._fp_table()
        first_item, n_items = fingerprint_range(first_item, n_items, total)
        n_bad, item, poly = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
        check(self._fp("scrub")(self.h, first_item, n_items, C.byref(n_bad), C.byref(item), C.byref(poly)))
        return int(n_bad.value), ((int(item.value), int(poly.value)) if n_bad.value else None)


def update_args(items, coeff_bits: int, item_ids, polys_per_item: int):
    """the argument list of an update_db_items call, checked before anything reaches the library: items as one contiguous array holding exactly
    len(item_ids) plaintexts of polys_per_item x 2048 coeff_bits-wide coefficients, item_ids as distinct non-negative integers (-> uint64)"""
    ids = np.asarray(item_ids)
    if ids.ndim != 1:
        raise ValueError("item_ids must be a flat list of item indices")
    if ids.size == 0:
        ids = ids.astype(np.uint64)
    elif ids.dtype.kind not in "iu":
        raise TypeError(f"item_ids must be integers, not {ids.dtype}")
    if ids.size and ids.dtype.kind == "i" and (ids < 0).any():
        raise ValueError("item_ids must be non-negative")
    ids = np.ascontiguousarray(ids, dtype=np.uint64)
    if np.unique(ids).size != ids.size:
        raise ValueError("item_ids holds a duplicate id")
    if not isinstance(coeff_bits, (int, np.integer)) or isinstance(coeff_bits, bool):
        raise TypeError("coeff_bits must be an integer")
    items = np.ascontiguousarray(items)
    want = ids.size * polys_per_item * 2048 * int(coeff_bits)
    if items.nbytes * 8 != want:
        raise ValueError(f"items holds {items.nbytes} bytes, {len(ids)} plaintexts of {coeff_bits}-bit coefficients take {want // 8}")
    return items, ids
