"""ctypes binding of include/iteres_amd.h (libiteres_amd.so) for the test-suite, bench.py and smoke().

This is plumbing above the C ABI, not a second implementation: every call lands in the HIP engine.
If the shared library is missing or no GPU is usable the calls raise — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ITX_LIB", os.path.join(HERE, "libiteres_amd.so"))   # ITX_LIB: timing-only experiment builds

MODE_STAT, MODE_FILTER = 0, 1
F5_NOLOOKUP = 0x20        # include/iteres_amd.h ITX_F5_NOLOOKUP
ACCUM_DEFAULT, ACCUM_ATOMIC, ACCUM_PARTITION = 0, 1, 2

EXPORTS = [
    "itx_last_error", "itx_abi_version", "itx_device_count", "itx_table_create", "itx_table_destroy",
    "itx_table_get_info", "itx_table_cov_offsets", "itx_table_debug_copy", "itx_engine_create", "itx_engine_destroy", "itx_engine_set_tidmap",
    "itx_engine_staging", "itx_engine_submit_slot", "itx_engine_classify_slot", "itx_engine_wait_slot", "itx_engine_submit_device",
    "itx_engine_classify_device", "itx_engine_first_hit_slot", "itx_engine_first_hit_device", "itx_engine_sync", "itx_engine_reset", "itx_engine_finish", "itx_engine_get_stats",
    "itx_engine_partial_size", "itx_engine_export_partial", "itx_engine_finish_partial",
    "itx_inflater_create", "itx_inflater_destroy", "itx_inflate_bgzf", "itx_inflater_last_ms", "itx_pinned_alloc", "itx_pinned_free",
    "itx_bamwin_push", "itx_bamwin_push_begin", "itx_bamwin_push_copied", "itx_bamwin_push_end", "itx_bamwin_patch", "itx_bamwin_truncate", "itx_bamwin_carry", "itx_bamwin_avail", "itx_bamwin_peek", "itx_bamwin_skip",
    "itx_bamwin_parse", "itx_bamwin_fetch", "itx_bamwin_bytes", "itx_bamwin_tids", "itx_bamwin_device_batch",
    "itx_engine_submit_device_own", "itx_engine_wait_own",
    "itx_engine_partial_buffers", "itx_inflater_reserve", "itx_inflater_last_resolve_all_ms", "itx_timing_report", "itx_xaveto_create", "itx_xaveto_destroy", "itx_xaveto_set_tidmap", "itx_xaveto_hits", "itx_xaveto_stream", "itx_bamwin_xa_veto", "itx_comm_create", "itx_comm_destroy", "itx_comm_reduce_sum",
    "itx_backlog_create", "itx_backlog_destroy", "itx_backlog_room", "itx_backlog_append", "itx_backlog_batch", "itx_dedup_create", "itx_dedup_destroy", "itx_dedup_set_tidmap", "itx_dedup_run", "itx_dedup_counts", "itx_bamwin_dedup",
    "itx_bigwig_start", "itx_bigwig_collect", "itx_bigwig_destroy",
    "itx_bed_create", "itx_bed_destroy", "itx_bed_set_tidmap", "itx_bamwin_bed", "itx_bed_run", "itx_bed_wait_kernels", "itx_bed_collect", "itx_bed_get_stats",
    "itx_names_create", "itx_names_destroy", "itx_names_hits", "itx_names_stream", "itx_bamwin_names", "itx_names_run", "itx_names_wait_kernels", "itx_names_append_host",
    "itx_names_finish", "itx_names_get_stats",
    "itx_gcov_create", "itx_gcov_destroy", "itx_gcov_set_tidmap", "itx_gcov_hits", "itx_gcov_stream", "itx_gcov_run", "itx_gcov_wait_kernels", "itx_gcov_add_host",
    "itx_gcov_finish", "itx_gcov_next", "itx_gcov_get_stats", "itx_gcov_bigwig_build", "itx_gcov_bigwig_result", "itx_gcov_copy_points",
    "itx_bamout_create", "itx_bamout_destroy", "itx_bamout_hits", "itx_bamout_stream", "itx_bamwin_bamout", "itx_bamout_run", "itx_bamout_wait_kernels",
    "itx_bamout_append_host", "itx_bamout_finish", "itx_bamout_collect", "itx_bamout_pending", "itx_bamout_get_stats", "itx_bamout_index_enable",
    "itx_bamout_index_finish", "itx_bamout_sort_enable", "itx_bamout_sort_next", "itx_bamout_sort_get_stats",
    "itx_bamout_set_level", "itx_bamout_get_level", "itx_bamout_annotate_enable", "itx_bamout_annotate_get_stats",
    "itx_bamout_mates_enable", "itx_bamout_mates_append_host", "itx_bamout_mates_host_rows", "itx_bamout_mates_get_stats",
    "itx_loci_create", "itx_loci_destroy", "itx_loci_order", "itx_loci_filter_text", "itx_loci_cpg_text",
    "itx_samtext_create", "itx_samtext_destroy", "itx_samtext_parse_begin", "itx_samtext_parse_end", "itx_samtext_fetch",
    "itx_samtext_parse_begin_bgzf", "itx_samtext_bgzf_info", "itx_samtext_text", "itx_samtext_strings",
]


class ItxError(RuntimeError):
    pass


class Row(C.Structure):
    _fields_ = [("chrom", C.c_int32), ("start", C.c_uint32), ("end", C.c_uint32), ("cons_start", C.c_uint32),
                ("cons_end", C.c_uint32), ("rep", C.c_uint32), ("fam", C.c_uint32), ("cla", C.c_uint32)]


ROW_DTYPE = np.dtype([("chrom", "<i4"), ("start", "<u4"), ("end", "<u4"), ("cons_start", "<u4"), ("cons_end", "<u4"),
                      ("rep", "<u4"), ("fam", "<u4"), ("cla", "<u4")])
assert ROW_DTYPE.itemsize == C.sizeof(Row) == 32


class TableInfo(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_rep", C.c_uint64), ("n_fam", C.c_uint64), ("n_cla", C.c_uint64),
                ("cov_len", C.c_uint64), ("n_units", C.c_uint64), ("n_slots", C.c_uint64), ("table_bytes", C.c_uint64),
                ("n_chrom", C.c_int32), ("bin_shift", C.c_int32), ("device", C.c_int32), ("reserved", C.c_int32)]


class Params(C.Structure):
    _fields_ = [("mapq_min", C.c_uint32), ("min_cov", C.c_float), ("extension", C.c_uint32), ("isize_max", C.c_uint32),
                ("treat_pe_as_se", C.c_int32), ("discard_half_mapped", C.c_int32), ("mode", C.c_int32), ("accum", C.c_int32)]


class Batch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("tid", "pos", "tmpend", "mapq", "flag5", "mpos", "isize")]


class Staging(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("tid", "pos", "tmpend", "mapq", "flag5", "mpos", "isize", "hit_row")] + [("capacity", C.c_size_t)]


class Result(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("cnt", "rep_cnt", "fam_cnt", "cla_cnt", "cov", "cov_uniq", "locus_cnt")]


class Stats(C.Structure):
    _fields_ = [("kernel_ms", C.c_double), ("records", C.c_uint64), ("hits", C.c_uint64), ("stage_ms", C.c_double * 5),
                ("submits", C.c_uint64), ("keys", C.c_uint64)]


class BwSummary(C.Structure):
    _fields_ = [("chrom_id", C.c_uint32), ("start", C.c_uint32), ("end", C.c_uint32), ("valid_count", C.c_uint32),
                ("min_val", C.c_float), ("max_val", C.c_float), ("sum_data", C.c_float), ("sum_squares", C.c_float)]


class BwResult(C.Structure):
    _fields_ = [("n_sec", C.c_uint64), ("n_blocks", C.c_uint64), ("n_levels", C.c_uint32), ("n_sum", C.c_uint64 * 10),
                ("slot_first", C.c_uint64 * 10), ("sum", C.POINTER(BwSummary) * 10), ("block_off", C.POINTER(C.c_uint64)),
                ("blocks", C.POINTER(C.c_uint8)), ("device_ms", C.c_double)]


BW_SUMMARY_DTYPE = np.dtype([("chrom_id", "<u4"), ("start", "<u4"), ("end", "<u4"), ("valid_count", "<u4"),
                             ("min_val", "<f4"), ("max_val", "<f4"), ("sum_data", "<f4"), ("sum_squares", "<f4")])
assert BW_SUMMARY_DTYPE.itemsize == C.sizeof(BwSummary) == 32

class BedText(C.Structure):
    _fields_ = [("all", C.c_void_p), ("uniq", C.c_void_p), ("all_bytes", C.c_uint64), ("uniq_bytes", C.c_uint64)]


class BedStats(C.Structure):
    _fields_ = [("batches", C.c_uint64), ("hard_batches", C.c_uint64), ("bytes", C.c_uint64), ("kernel_ms", C.c_double), ("wait_s", C.c_double)]


BED_ALL, BED_UNIQ = 1, 2


class GcovText(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("len", C.c_uint64), ("more", C.c_int32), ("pad", C.c_int32)]


class GcovStats(C.Structure):
    _fields_ = [("batches", C.c_uint64), ("host_batches", C.c_uint64), ("records", C.c_uint64), ("out_of_range", C.c_uint64), ("records_uniq", C.c_uint64),
                ("points", C.c_uint64 * 2), ("lines", C.c_uint64 * 2), ("bytes", C.c_uint64 * 2), ("rounds", C.c_uint64 * 2), ("slots", C.c_uint64),
                ("device_bytes", C.c_uint64), ("add_ms", C.c_double), ("points_ms", C.c_double), ("text_ms", C.c_double), ("zero_ms", C.c_double),
                ("wait_s", C.c_double), ("alloc_s", C.c_double), ("bw_items", C.c_uint64 * 2), ("bw_sections", C.c_uint64 * 2), ("bw_levels", C.c_uint64 * 2),
                ("bw_summaries", C.c_uint64 * 2), ("bw_ms", C.c_double)]


class GcovBwResult(C.Structure):
    _fields_ = [("n_items", C.c_uint64), ("n_sec", C.c_uint64), ("n_blocks", C.c_uint64), ("n_chrom", C.c_uint32), ("n_levels", C.c_uint32),
                ("chrom", C.c_void_p), ("sec_key", C.c_void_p), ("sec_count", C.c_void_p), ("reduction", C.c_uint32 * 10), ("n_sum", C.c_uint64 * 10),
                ("slot_first", C.c_uint64 * 10), ("sum", C.c_void_p * 10), ("block_off", C.c_void_p), ("blocks", C.c_void_p), ("reduce_rounds", C.c_uint32),
                ("pad", C.c_uint32), ("items_ms", C.c_double), ("chain_ms", C.c_double), ("fold_ms", C.c_double), ("deflate_ms", C.c_double)]


class NamesResult(C.Structure):
    _fields_ = [("text", C.c_void_p), ("text_bytes", C.c_uint64), ("row_off", C.c_void_p), ("row_cnt", C.c_void_p), ("n_entries", C.c_uint64)]


class NamesStats(C.Structure):
    _fields_ = [("batches", C.c_uint64), ("hard_batches", C.c_uint64), ("host_batches", C.c_uint64), ("entries", C.c_uint64), ("bytes", C.c_uint64),
                ("grows", C.c_uint64), ("gather_ms", C.c_double), ("finish_ms", C.c_double)]


class BamoutMembers(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("len", C.c_uint64), ("room", C.c_uint64), ("n_members", C.c_uint64)]


class BamoutStats(C.Structure):
    _fields_ = [("batches", C.c_uint64), ("host_batches", C.c_uint64), ("records", C.c_uint64), ("payload_bytes", C.c_uint64), ("members", C.c_uint64),
                ("out_bytes", C.c_uint64), ("grows", C.c_uint64), ("carry", C.c_uint64), ("gather_ms", C.c_double), ("member_ms", C.c_double),
                ("wait_ms", C.c_double)]


class BamoutIndexResult(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("len", C.c_uint64), ("status", C.c_int32), ("pad", C.c_int32), ("entries", C.c_uint64), ("chunks", C.c_uint64),
                ("grows", C.c_uint64), ("batch_ms", C.c_double), ("finish_ms", C.c_double)]


class BamoutSortStats(C.Structure):
    _fields_ = [("records", C.c_uint64), ("rounds", C.c_uint64), ("pool_grows", C.c_uint64), ("sort_ms", C.c_double), ("replay_ms", C.c_double)]


class BamoutMatesStats(C.Structure):
    _fields_ = [("candidates", C.c_uint64), ("candidate_bytes", C.c_uint64), ("grows", C.c_uint64), ("wanted", C.c_uint64), ("found", C.c_uint64),
                ("gather_ms", C.c_double), ("join_ms", C.c_double)]


class LociText(C.Structure):
    _fields_ = [("text", C.c_void_p), ("bytes", C.c_uint64), ("capacity", C.c_uint64), ("lines", C.c_uint64), ("hard", C.c_uint64), ("sort_ms", C.c_double),
                ("text_ms", C.c_double)]


LOCI_FILTER, LOCI_CPG = 0, 1


class SamTextResult(C.Structure):
    _fields_ = [("n_lines", C.c_uint64), ("n_rec", C.c_uint64), ("consumed", C.c_uint64), ("n_hard", C.c_uint64), ("first_hard_line", C.c_uint64),
                ("flags", C.c_int), ("kernel_ms", C.c_double)]


class SamTextBgzfInfo(C.Structure):
    _fields_ = [("text_len", C.c_uint64), ("carry_len", C.c_uint64), ("tail_len", C.c_uint64), ("n_bad", C.c_uint64), ("first_bad", C.c_uint64),
                ("inflate_ms", C.c_double)]


class SamTextStrings(C.Structure):
    _fields_ = [("text", C.c_void_p), ("text_len", C.c_uint64), ("qname_at", C.c_void_p), ("xa_at", C.c_void_p), ("kernel_ms", C.c_double)]


SAMTEXT_PAIRED, SAMTEXT_XA, SAMTEXT_NUL = 1, 2, 4
SAMTEXT_NO_STRING = 0xFFFFFFFF

_lib = None


def load():
    """Loads the in-tree shared library; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ItxError(f"{LIB_PATH} is missing: build it with `python -m iteres_amd.build` (hipcc, gfx950)")
    L = C.CDLL(LIB_PATH)
    L.itx_last_error.restype = C.c_char_p
    L.itx_table_create.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    L.itx_table_destroy.argtypes = [C.c_void_p]
    L.itx_table_destroy.restype = None
    L.itx_table_get_info.argtypes = [C.c_void_p, C.POINTER(TableInfo)]
    L.itx_table_cov_offsets.argtypes = [C.c_void_p, C.c_void_p]
    L.itx_table_debug_copy.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.itx_engine_create.argtypes = [C.c_void_p, C.POINTER(Params), C.c_size_t, C.POINTER(C.c_void_p)]
    L.itx_engine_partial_size.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.itx_engine_export_partial.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.itx_engine_finish_partial.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Result)]
    L.itx_engine_partial_buffers.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.itx_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    L.itx_comm_destroy.argtypes = [C.c_void_p]
    L.itx_comm_destroy.restype = None
    L.itx_comm_reduce_sum.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    L.itx_engine_destroy.argtypes = [C.c_void_p]
    L.itx_engine_destroy.restype = None
    L.itx_engine_set_tidmap.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.itx_engine_staging.argtypes = [C.c_void_p, C.c_int, C.POINTER(Staging)]
    L.itx_engine_submit_slot.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int, C.c_int]
    L.itx_engine_classify_slot.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_int]
    L.itx_engine_first_hit_slot.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    L.itx_engine_first_hit_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_size_t, C.c_void_p, C.c_void_p]
    L.itx_engine_wait_slot.argtypes = [C.c_void_p, C.c_int]
    L.itx_engine_submit_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_size_t, C.c_void_p, C.c_void_p]
    L.itx_engine_classify_device.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_size_t, C.c_void_p, C.c_void_p]
    L.itx_engine_sync.argtypes = [C.c_void_p]
    L.itx_engine_reset.argtypes = [C.c_void_p]
    L.itx_engine_finish.argtypes = [C.c_void_p, C.POINTER(Result)]
    L.itx_engine_get_stats.argtypes = [C.c_void_p, C.POINTER(Stats)]
    L.itx_inflater_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.itx_inflater_destroy.argtypes = [C.c_void_p]
    L.itx_inflater_destroy.restype = None
    L.itx_inflate_bgzf.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    L.itx_inflater_last_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.itx_bamwin_push.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]
    L.itx_bamwin_patch.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t]
    L.itx_bamwin_truncate.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    L.itx_bamwin_carry.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.itx_bamwin_avail.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_size_t)]
    L.itx_bamwin_peek.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t]
    L.itx_bamwin_skip.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    L.itx_bamwin_parse.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_size_t)]
    L.itx_bamwin_fetch.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(Staging), C.c_size_t, C.c_void_p, C.c_void_p]
    L.itx_bamwin_bytes.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.itx_dedup_create.argtypes = [C.c_int, C.c_void_p, C.c_int, C.POINTER(Params), C.c_size_t, C.POINTER(C.c_void_p)]
    L.itx_dedup_destroy.argtypes = [C.c_void_p]
    L.itx_dedup_destroy.restype = None
    L.itx_dedup_set_tidmap.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    L.itx_dedup_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.itx_dedup_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.itx_bigwig_start.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.itx_bigwig_collect.argtypes = [C.c_void_p, C.POINTER(BwResult)]
    L.itx_bigwig_destroy.argtypes = [C.c_void_p]
    L.itx_bigwig_destroy.restype = None
    L.itx_bamwin_dedup.argtypes = [C.c_void_p, C.c_void_p]
    L.itx_bed_create.argtypes = [C.c_int, C.c_void_p, C.c_int, C.POINTER(Params), C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    L.itx_bed_destroy.argtypes = [C.c_void_p]
    L.itx_bed_destroy.restype = None
    L.itx_bed_set_tidmap.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_int]
    L.itx_bamwin_bed.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64)]
    L.itx_bed_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Batch), C.c_size_t, C.POINTER(C.c_uint64)]
    L.itx_bed_wait_kernels.argtypes = [C.c_void_p]
    L.itx_bamwin_device_batch.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(Batch)]
    L.itx_xaveto_create.argtypes = [C.c_void_p, C.POINTER(Params), C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    L.itx_xaveto_destroy.argtypes = [C.c_void_p]
    L.itx_xaveto_destroy.restype = None
    L.itx_xaveto_set_tidmap.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.itx_xaveto_hits.argtypes = [C.c_void_p]
    L.itx_xaveto_hits.restype = C.c_void_p
    L.itx_xaveto_stream.argtypes = [C.c_void_p]
    L.itx_xaveto_stream.restype = C.c_void_p
    L.itx_bamwin_xa_veto.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.itx_bed_collect.argtypes = [C.c_void_p, C.POINTER(BedText)]
    L.itx_bed_get_stats.argtypes = [C.c_void_p, C.POINTER(BedStats)]
    L.itx_names_create.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p)]
    L.itx_names_destroy.argtypes = [C.c_void_p]
    L.itx_names_destroy.restype = None
    L.itx_names_hits.argtypes = [C.c_void_p]
    L.itx_names_hits.restype = C.c_void_p
    L.itx_names_stream.argtypes = [C.c_void_p]
    L.itx_names_stream.restype = C.c_void_p
    L.itx_bamwin_names.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
    L.itx_names_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint64)]
    L.itx_names_wait_kernels.argtypes = [C.c_void_p]
    L.itx_names_append_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.itx_names_finish.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(NamesResult)]
    L.itx_names_get_stats.argtypes = [C.c_void_p, C.POINTER(NamesStats)]
    L.itx_gcov_create.argtypes = [C.c_int, C.c_void_p, C.c_int, C.POINTER(Params), C.c_size_t, C.POINTER(C.c_void_p)]
    L.itx_gcov_destroy.argtypes = [C.c_void_p]
    L.itx_gcov_destroy.restype = None
    L.itx_gcov_set_tidmap.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.itx_gcov_hits.argtypes = [C.c_void_p]
    L.itx_gcov_hits.restype = C.c_void_p
    L.itx_gcov_stream.argtypes = [C.c_void_p]
    L.itx_gcov_stream.restype = C.c_void_p
    L.itx_gcov_run.argtypes = [C.c_void_p, C.POINTER(Batch), C.c_void_p, C.c_size_t, C.c_void_p]
    L.itx_gcov_wait_kernels.argtypes = [C.c_void_p]
    L.itx_gcov_add_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    L.itx_gcov_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    L.itx_gcov_next.argtypes = [C.c_void_p, C.c_int, C.POINTER(GcovText)]
    L.itx_gcov_get_stats.argtypes = [C.c_void_p, C.POINTER(GcovStats)]
    L.itx_gcov_bigwig_build.argtypes = [C.c_void_p, C.c_int]
    L.itx_gcov_bigwig_result.argtypes = [C.c_void_p, C.c_int, C.POINTER(GcovBwResult)]
    L.itx_gcov_copy_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.itx_bamout_create.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p)]
    L.itx_bamout_destroy.argtypes = [C.c_void_p]
    L.itx_bamout_destroy.restype = None
    L.itx_bamout_hits.argtypes = [C.c_void_p]
    L.itx_bamout_hits.restype = C.c_void_p
    L.itx_bamout_stream.argtypes = [C.c_void_p]
    L.itx_bamout_stream.restype = C.c_void_p
    L.itx_bamwin_bamout.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p]
    L.itx_bamout_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.itx_bamout_wait_kernels.argtypes = [C.c_void_p]
    L.itx_bamout_append_host.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.itx_bamout_finish.argtypes = [C.c_void_p]
    L.itx_bamout_collect.argtypes = [C.c_void_p, C.POINTER(BamoutMembers)]
    L.itx_bamout_pending.argtypes = [C.c_void_p]
    L.itx_bamout_get_stats.argtypes = [C.c_void_p, C.POINTER(BamoutStats)]
    L.itx_bamout_index_enable.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    L.itx_bamout_index_finish.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(BamoutIndexResult)]
    L.itx_bamout_sort_enable.argtypes = [C.c_void_p]
    L.itx_bamout_sort_next.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.itx_bamout_sort_get_stats.argtypes = [C.c_void_p, C.POINTER(BamoutSortStats)]
    L.itx_bamout_set_level.argtypes = [C.c_void_p, C.c_int]
    L.itx_bamout_get_level.argtypes = [C.c_void_p]
    L.itx_bamout_annotate_enable.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p, C.c_void_p, C.c_uint32] * 3
    L.itx_bamout_annotate_get_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.itx_bamout_mates_enable.argtypes = [C.c_void_p]
    L.itx_bamout_mates_append_host.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.itx_bamout_mates_host_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.itx_bamout_mates_get_stats.argtypes = [C.c_void_p, C.POINTER(BamoutMatesStats)]
    L.itx_loci_create.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                  C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.itx_loci_destroy.argtypes = [C.c_void_p]
    L.itx_loci_destroy.restype = None
    L.itx_loci_order.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    L.itx_loci_filter_text.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_ulonglong, C.POINTER(LociText)]
    L.itx_loci_cpg_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(LociText)]
    L.itx_samtext_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    L.itx_samtext_destroy.argtypes = [C.c_void_p]
    L.itx_samtext_destroy.restype = None
    L.itx_samtext_parse_begin.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int]
    L.itx_samtext_parse_end.argtypes = [C.c_void_p, C.c_int, C.POINTER(SamTextResult)]
    L.itx_samtext_fetch.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.POINTER(Staging), C.c_size_t] + [C.c_void_p] * 6
    L.itx_samtext_parse_begin_bgzf.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
    L.itx_samtext_bgzf_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(SamTextBgzfInfo)]
    L.itx_samtext_text.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t]
    L.itx_samtext_strings.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(SamTextStrings)]
    L.itx_pinned_alloc.argtypes = [C.c_size_t]
    L.itx_pinned_alloc.restype = C.c_void_p
    L.itx_pinned_free.argtypes = [C.c_void_p]
    L.itx_pinned_free.restype = None
    _lib = L
    return L


def _chk(rc, what):
    if rc != 0:
        raise ItxError(f"{what}: rc={rc}: {load().itx_last_error().decode(errors='replace')}")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def flag5(bamflag):
    f = np.asarray(bamflag).astype(np.uint32)
    return (((f & 0x1) != 0) * 1 + ((f & 0x4) != 0) * 2 + ((f & 0x8) != 0) * 4 + ((f & 0x10) != 0) * 8 + ((f & 0x40) != 0) * 16).astype(np.uint8)


def make_rows(chrom, start, end, cons_start, cons_end, rep, fam, cla):
    n = len(chrom)
    rows = np.empty(n, ROW_DTYPE)
    u = lambda a: (np.asarray(a).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
    rows["chrom"] = np.asarray(chrom, np.int32)
    for k, v in (("start", start), ("end", end), ("cons_start", cons_start), ("cons_end", cons_end), ("rep", rep), ("fam", fam), ("cla", cla)):
        rows[k] = u(v)
    return rows


class Table:
    def __init__(self, rows, chrom_size, rep_len, n_fam, n_cla, device=0):
        L = load()
        self.rows = np.ascontiguousarray(rows, ROW_DTYPE)
        cs = np.ascontiguousarray(chrom_size, np.int64)
        rl = np.ascontiguousarray(rep_len, np.uint32)
        h = C.c_void_p()
        bad = C.c_size_t(0)
        rc = L.itx_table_create(_p(self.rows), len(self.rows), _p(cs), len(cs), _p(rl), len(rl), int(n_fam), int(n_cla), int(device),
                                C.byref(h), C.byref(bad))
        self.bad_row = bad.value
        _chk(rc, "itx_table_create")
        self._h = h
        self.info = TableInfo()
        _chk(L.itx_table_get_info(self._h, C.byref(self.info)), "itx_table_get_info")
        self.cov_off = np.zeros(len(rl) + 1, np.uint64)
        _chk(L.itx_table_cov_offsets(self._h, _p(self.cov_off)), "itx_table_cov_offsets")
        self.n_rep, self.n_fam, self.n_cla, self.n_rows = len(rl), int(n_fam), int(n_cla), len(self.rows)
        self.device = device

    # include/iteres_amd.h ITX_TABLE_*: the arrays of the built table, in that order
    SNAPSHOT = ("iv", "orig", "bl", "row_unit", "part_unit", "unit_slot", "unit_ids", "unit_covoff", "chrom_off", "bin_off")

    def snapshot(self):
        """Tests only: every array of the built table as raw bytes (itx_table_debug_copy), by name."""
        L = load()
        out = {}
        for which, name in enumerate(self.SNAPSHOT):
            nb = C.c_size_t(0)
            _chk(L.itx_table_debug_copy(self._h, which, None, 0, C.byref(nb)), "itx_table_debug_copy")
            a = np.zeros(nb.value, np.uint8)
            _chk(L.itx_table_debug_copy(self._h, which, _p(a), a.nbytes, C.byref(nb)), "itx_table_debug_copy")
            out[name] = a
        return out

    def close(self):
        if getattr(self, "_h", None):
            load().itx_table_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    def __init__(self, table: Table, params: dict | None = None, batch_capacity: int = 1 << 20):
        L = load()
        q = dict(mapq_min=10, min_cov=0.0001, extension=150, isize_max=500, treat_pe_as_se=False, discard_half_mapped=False,
                 filter_mode=False, accum=ACCUM_DEFAULT)
        q.update(params or {})
        self.params = Params(int(q["mapq_min"]), float(np.float32(q["min_cov"])), int(q["extension"]), int(q["isize_max"]),
                             int(bool(q["treat_pe_as_se"])), int(bool(q["discard_half_mapped"])),
                             MODE_FILTER if q.get("filter_mode") else MODE_STAT, int(q["accum"]))
        self.table = table
        h = C.c_void_p()
        _chk(L.itx_engine_create(table._h, C.byref(self.params), int(batch_capacity), C.byref(h)), "itx_engine_create")
        self._h = h
        self.capacity = int(batch_capacity)

    def set_tidmap(self, tid2chrom):
        a = np.ascontiguousarray(tid2chrom, np.int32)
        _chk(load().itx_engine_set_tidmap(self._h, _p(a), len(a)), "itx_engine_set_tidmap")

    def staging(self, slot):
        st = Staging()
        _chk(load().itx_engine_staging(self._h, slot, C.byref(st)), "itx_engine_staging")
        n = st.capacity

        def view(ptr, ctype, dt):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(n,)).view(dt)
        return {"tid": view(st.tid, C.c_int32, np.int32), "pos": view(st.pos, C.c_int32, np.int32),
                "tmpend": view(st.tmpend, C.c_int32, np.int32), "mapq": view(st.mapq, C.c_uint8, np.uint8),
                "flag5": view(st.flag5, C.c_uint8, np.uint8), "mpos": view(st.mpos, C.c_int32, np.int32),
                "isize": view(st.isize, C.c_int32, np.int32), "hit_row": view(st.hit_row, C.c_int32, np.int32)}

    def submit_host(self, tid, pos, tmpend, mapq, flag5_, mpos=None, isize=None, want_hits=False, veto=None):
        """Streams host arrays through the pinned double buffers (slot ping-pong). Returns hit rows if asked.
        veto(offset, hit_rows) -> bool mask: records to mark ITX_F5_NOLOOKUP after a classify-only pass."""
        L = load()
        n = len(tid)
        hits = np.empty(n, np.int32) if want_hits else None
        paired = mpos is not None and isize is not None
        bufs = [self.staging(0), self.staging(1)]
        pending = [None, None]
        off, s = 0, 0
        while off < n or any(p is not None for p in pending):
            if pending[s] is not None:
                _chk(L.itx_engine_wait_slot(self._h, s), "itx_engine_wait_slot")
                a, b = pending[s]
                if want_hits:
                    hits[a:b] = bufs[s]["hit_row"][: b - a]
                pending[s] = None
            if off < n:
                m = min(self.capacity, n - off)
                sl = slice(off, off + m)
                bufs[s]["tid"][:m] = tid[sl]; bufs[s]["pos"][:m] = pos[sl]; bufs[s]["tmpend"][:m] = tmpend[sl]
                bufs[s]["mapq"][:m] = mapq[sl]; bufs[s]["flag5"][:m] = flag5_[sl]
                if paired:
                    bufs[s]["mpos"][:m] = mpos[sl]; bufs[s]["isize"][:m] = isize[sl]
                if veto is not None:
                    # what a caller with an XA-style veto does: classify, look at the chosen rows, mark, then count
                    _chk(L.itx_engine_classify_slot(self._h, s, m, int(paired)), "itx_engine_classify_slot")
                    _chk(L.itx_engine_wait_slot(self._h, s), "itx_engine_wait_slot")
                    mask = np.asarray(veto(off, bufs[s]["hit_row"][:m].copy()), bool)
                    bufs[s]["flag5"][:m] |= mask.astype(np.uint8) * np.uint8(F5_NOLOOKUP)
                _chk(L.itx_engine_submit_slot(self._h, s, m, int(paired), int(want_hits)), "itx_engine_submit_slot")
                pending[s] = (off, off + m)
                off += m
            s ^= 1
        return hits

    def first_hits_host(self, tid, start, end):
        """First row in binKeeperFind's order for every plain interval (itx_engine_first_hit_slot), through the slots."""
        L = load()
        n = len(tid)
        hits = np.empty(n, np.int32)
        bufs = [self.staging(0), self.staging(1)]
        pending = [None, None]
        off, s = 0, 0
        while off < n or any(p is not None for p in pending):
            if pending[s] is not None:
                _chk(L.itx_engine_wait_slot(self._h, s), "itx_engine_wait_slot")
                a, b = pending[s]
                hits[a:b] = bufs[s]["hit_row"][: b - a]
                pending[s] = None
            if off < n:
                m = min(self.capacity, n - off)
                sl = slice(off, off + m)
                bufs[s]["tid"][:m] = tid[sl]; bufs[s]["pos"][:m] = start[sl]; bufs[s]["tmpend"][:m] = end[sl]
                bufs[s]["mapq"][:m] = 0; bufs[s]["flag5"][:m] = 0
                _chk(L.itx_engine_first_hit_slot(self._h, s, m), "itx_engine_first_hit_slot")
                pending[s] = (off, off + m)
                off += m
            s ^= 1
        return hits

    def submit_device(self, ptrs: dict, n: int, hit_ptr=None, stream=None, classify_only=False):
        b = Batch(*(ptrs.get(k) for k in ("tid", "pos", "tmpend", "mapq", "flag5", "mpos", "isize")))
        fn = load().itx_engine_classify_device if classify_only else load().itx_engine_submit_device
        _chk(fn(self._h, C.byref(b), int(n), hit_ptr, stream), "itx_engine_submit_device")

    def sync(self):
        _chk(load().itx_engine_sync(self._h), "itx_engine_sync")

    def reset(self):
        _chk(load().itx_engine_reset(self._h), "itx_engine_reset")

    def _result_arrays(self):
        t = self.table
        res = {"cnt": np.zeros(13, np.uint64), "rep_cnt": np.zeros(2 * t.n_rep, np.uint64), "fam_cnt": np.zeros(2 * t.n_fam, np.uint64),
               "cla_cnt": np.zeros(2 * t.n_cla, np.uint64), "cov": np.zeros(int(t.info.cov_len), np.uint32),
               "cov_uniq": np.zeros(int(t.info.cov_len), np.uint32), "locus_cnt": np.zeros(max(t.n_rows, 1), np.uint32)}
        r = Result(*(_p(res[k]) for k in ("cnt", "rep_cnt", "fam_cnt", "cla_cnt", "cov", "cov_uniq", "locus_cnt")))
        return res, r

    def finish(self):
        res, r = self._result_arrays()
        _chk(load().itx_engine_finish(self._h, C.byref(r)), "itx_engine_finish")
        return res

    def partial_size(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        _chk(load().itx_engine_partial_size(self._h, C.byref(a), C.byref(b)), "itx_engine_partial_size")
        return int(a.value), int(b.value)

    def export_partial(self, u64_ptr, u32_ptr, stream=None):
        _chk(load().itx_engine_export_partial(self._h, u64_ptr, u32_ptr, stream), "itx_engine_export_partial")

    def finish_partial(self, u64_ptr, u32_ptr):
        res, r = self._result_arrays()
        _chk(load().itx_engine_finish_partial(self._h, u64_ptr, u32_ptr, C.byref(r)), "itx_engine_finish_partial")
        return res

    def stats(self):
        s = Stats()
        _chk(load().itx_engine_get_stats(self._h, C.byref(s)), "itx_engine_get_stats")
        return {"kernel_ms": s.kernel_ms, "records": int(s.records), "hits": int(s.hits), "stage_ms": list(s.stage_ms),
                "submits": int(s.submits), "keys": int(s.keys)}

    def close(self):
        if getattr(self, "_h", None):
            load().itx_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bigwig:
    """itx_bigwig_start / collect / destroy (include/iteres_amd.h): the blocks and summaries of one bigWig built on the
    device from a finished engine's coverage. seqs: (offset into the coverage, length) in bigWig id order."""

    def __init__(self, engine: Engine, uniq: bool, seqs, reductions):
        off = np.ascontiguousarray([o for o, _ in seqs], np.uint64)
        ln = np.ascontiguousarray([n for _, n in seqs], np.uint32)
        red = np.ascontiguousarray(reductions, np.uint32)
        self._h = C.c_void_p()
        _chk(load().itx_bigwig_start(engine._h, int(bool(uniq)), _p(off), _p(ln), len(ln), _p(red), len(red), C.byref(self._h)),
             "itx_bigwig_start")

    def collect(self):
        """{"n_sec", "n_blocks", "n_sum": [..], "slot_first": [..], "levels": [BW_SUMMARY_DTYPE array], "block_off": uint64
        [n_blocks + 1], "blocks": bytes, "device_ms"}, copied out of the build's own buffers"""
        r = BwResult()
        _chk(load().itx_bigwig_collect(self._h, C.byref(r)), "itx_bigwig_collect")
        nl, nb = int(r.n_levels), int(r.n_blocks)
        block_off = np.ctypeslib.as_array(r.block_off, shape=(nb + 1,)).copy()
        levels = []
        for k in range(nl):
            n = int(r.n_sum[k])
            levels.append(np.frombuffer(C.string_at(r.sum[k], 32 * n), BW_SUMMARY_DTYPE).copy() if n else np.zeros(0, BW_SUMMARY_DTYPE))
        return {"n_sec": int(r.n_sec), "n_blocks": nb, "n_levels": nl, "n_sum": [int(r.n_sum[k]) for k in range(nl)],
                "slot_first": [int(r.slot_first[k]) for k in range(nl)], "levels": levels, "block_off": block_off,
                "blocks": C.string_at(r.blocks, int(block_off[nb])), "device_ms": float(r.device_ms)}

    def close(self):
        if getattr(self, "_h", None):
            load().itx_bigwig_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


BGZF_BLOCK = np.dtype([("coff", np.uint32), ("csize", np.uint32), ("uoff", np.uint32), ("usize", np.uint32)])


def index_bgzf(buf) -> np.ndarray:
    """The complete BGZF blocks of a byte buffer (what the host reader's indexer finds: header check, BSIZE, ISIZE)."""
    b = np.frombuffer(buf, np.uint8)
    out, off, uoff = [], 0, 0
    while off + 18 <= len(b):
        h = b[off:off + 18]
        if not (h[0] == 31 and h[1] == 139 and h[2] == 8 and (h[3] & 4) and h[12] == 66 and h[13] == 67):
            break
        bsize = int(h[16]) + (int(h[17]) << 8) + 1
        if off + bsize > len(b):
            break
        usize = int.from_bytes(bytes(b[off + bsize - 4:off + bsize]), "little")
        out.append((off, bsize, uoff, usize))
        off += bsize
        uoff += usize
    return np.array(out, BGZF_BLOCK)


class Inflater:
    """itx_inflate_bgzf: the BGZF blocks of a compressed chunk, one wavefront each (include/iteres_amd.h)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        _chk(load().itx_inflater_create(device, C.byref(self._h)), "itx_inflater_create")

    def inflate(self, comp: bytes, blocks: np.ndarray | None = None):
        blocks = index_bgzf(comp) if blocks is None else np.ascontiguousarray(blocks, BGZF_BLOCK)
        cbuf = np.zeros(len(comp) + 16, np.uint8)
        cbuf[:len(comp)] = np.frombuffer(comp, np.uint8)
        total = int(blocks["usize"].astype(np.uint64).sum())
        out = np.zeros(total + 16, np.uint8)
        status = np.full(max(len(blocks), 1), 255, np.uint8)
        _chk(load().itx_inflate_bgzf(self._h, _p(cbuf), len(comp), _p(blocks), len(blocks), _p(out), total, _p(status)), "itx_inflate_bgzf")
        return out[:total], status[:len(blocks)]

    def close(self):
        if self._h:
            load().itx_inflater_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Dedup:
    """-R on the device (include/iteres_amd.h itx_dedup_*, replacing generic.c:907-919): `run` takes the next records of the
    stream as torch DEVICE tensors (int32 tid / pos / tmpend, uint8 mapq / flag5, optional int32 mpos / isize) and ORs
    ITX_F5_NOLOOKUP into flag5 for the records the reference would `continue` over."""

    def __init__(self, chrom_size, params: dict | None = None, first_cells: int = 1 << 16, device: int = 0):
        L = load()
        q = dict(mapq_min=10, min_cov=1e-4, extension=150, isize_max=500, treat_pe_as_se=False, discard_half_mapped=False)
        q.update(params or {})
        p = Params(int(q["mapq_min"]), float(q["min_cov"]), int(q["extension"]), int(q["isize_max"]), int(bool(q["treat_pe_as_se"])),
                   int(bool(q["discard_half_mapped"])), MODE_STAT, ACCUM_DEFAULT)
        cs = np.ascontiguousarray(chrom_size, np.int64)
        self._h = C.c_void_p()
        _chk(L.itx_dedup_create(device, _p(cs), len(cs), C.byref(p), first_cells, C.byref(self._h)), "itx_dedup_create")

    def set_tidmap(self, tid2chrom, tid2name):
        a = np.ascontiguousarray(tid2chrom, np.int32)
        b = np.ascontiguousarray(tid2name, np.uint32)
        _chk(load().itx_dedup_set_tidmap(self._h, _p(a), _p(b), len(a)), "itx_dedup_set_tidmap")

    def run(self, tid, pos, tmpend, mapq, flag5, mpos=None, isize=None):
        n = int(tid.numel())
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        _chk(load().itx_dedup_run(self._h, ptr(tid), ptr(pos), ptr(tmpend), ptr(mapq), ptr(flag5), ptr(mpos), ptr(isize), n), "itx_dedup_run")

    def counts(self):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _chk(load().itx_dedup_counts(self._h, C.byref(a), C.byref(b), C.byref(c)), "itx_dedup_counts")
        return {"dup_unique": a.value, "dropped": b.value, "keys": c.value}

    def close(self):
        if self._h:
            load().itx_dedup_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class XaVeto:
    """The XA / NM veto on the device (include/iteres_amd.h itx_xaveto_*, replacing generic.c:303-341 and 972-982) over the records of
    an Inflater's last parsed window. `judge` classifies records [first, first + n) with the engine into the object's own buffer of
    chosen rows, the way the command does, lets the device read their tags and returns (n_vetoed, n_hard): with n_hard > 0
    nothing was marked, else the vetoed records carry ITX_F5_NOLOOKUP in the window's flag5."""

    def __init__(self, engine: "Engine", row_rep, rep_word, chrom_names, batch_capacity: int = 1 << 20):
        rr = np.ascontiguousarray(row_rep, np.uint32)
        rw = np.ascontiguousarray(rep_word, np.uint32)
        names = (C.c_char_p * len(chrom_names))(*[s if isinstance(s, bytes) else s.encode() for s in chrom_names])
        self.engine = engine
        self._h = C.c_void_p()
        _chk(load().itx_xaveto_create(engine.table._h, C.byref(engine.params), _p(rr), _p(rw), names, len(chrom_names), batch_capacity, C.byref(self._h)), "itx_xaveto_create")

    def set_tidmap(self, tid2chrom):
        a = np.ascontiguousarray(tid2chrom, np.int32)
        _chk(load().itx_xaveto_set_tidmap(self._h, _p(a), len(a)), "itx_xaveto_set_tidmap")

    def judge(self, inflater, first, n, with_mates=False):
        L = load()
        db = Batch()
        _chk(L.itx_bamwin_device_batch(inflater._h, first, int(with_mates), C.byref(db)), "itx_bamwin_device_batch")
        _chk(L.itx_engine_classify_device(self.engine._h, C.byref(db), n, L.itx_xaveto_hits(self._h), L.itx_xaveto_stream(self._h)), "itx_engine_classify_device")
        vetoed, hard = C.c_uint64(), C.c_uint64()
        _chk(L.itx_bamwin_xa_veto(inflater._h, self._h, first, n, C.byref(vetoed), C.byref(hard)), "itx_bamwin_xa_veto")
        return vetoed.value, hard.value

    def close(self):
        if self._h:
            load().itx_xaveto_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bed:
    """The bed text of stat -B / -V built on the device (include/iteres_amd.h itx_bed_*, replacing generic.c:925-936). `start_window`
    takes records of an Inflater's last parsed window, `run` plain torch DEVICE tensors (uint8 record bytes, uint32-as-int32
    offsets, and the per-record arrays); both return how many records need the host's reading (then nothing was started).
    `collect` hands out the (-B, -V) text of the oldest started batch as bytes."""

    def __init__(self, chrom_size, params: dict | None = None, want: int = BED_ALL | BED_UNIQ, batch_capacity: int = 1 << 20, device: int = 0):
        q = dict(mapq_min=10, min_cov=1e-4, extension=150, isize_max=500, treat_pe_as_se=False, discard_half_mapped=False)
        q.update(params or {})
        p = Params(int(q["mapq_min"]), float(q["min_cov"]), int(q["extension"]), int(q["isize_max"]), int(bool(q["treat_pe_as_se"])),
                   int(bool(q["discard_half_mapped"])), MODE_STAT, ACCUM_DEFAULT)
        cs = np.ascontiguousarray(chrom_size, np.int64)
        self._h = C.c_void_p()
        _chk(load().itx_bed_create(device, _p(cs), len(cs), C.byref(p), want, batch_capacity, C.byref(self._h)), "itx_bed_create")

    def set_tidmap(self, tid2chrom, tid2name):
        a = np.ascontiguousarray(tid2chrom, np.int32)
        names = (C.c_char_p * max(len(a), 1))(*[None if s is None else (s if isinstance(s, bytes) else s.encode()) for s in tid2name])
        _chk(load().itx_bed_set_tidmap(self._h, _p(a), names, len(a)), "itx_bed_set_tidmap")

    def start_window(self, inflater, first, n):
        hard = C.c_uint64()
        _chk(load().itx_bamwin_bed(inflater._h, self._h, first, n, C.byref(hard)), "itx_bamwin_bed")
        return hard.value

    def run(self, rec_bytes, rec_off, tid, pos, tmpend, mapq, flag5, mpos=None, isize=None):
        ptr = lambda t: None if t is None else t.data_ptr()
        b = Batch(ptr(tid), ptr(pos), ptr(tmpend), ptr(mapq), ptr(flag5), ptr(mpos), ptr(isize))
        hard = C.c_uint64()
        _chk(load().itx_bed_run(self._h, ptr(rec_bytes), ptr(rec_off), C.byref(b), int(tid.numel()), C.byref(hard)), "itx_bed_run")
        return hard.value

    def collect(self):
        t = BedText()
        _chk(load().itx_bed_collect(self._h, C.byref(t)), "itx_bed_collect")
        return (C.string_at(t.all, t.all_bytes) if t.all_bytes else b"", C.string_at(t.uniq, t.uniq_bytes) if t.uniq_bytes else b"")

    def stats(self):
        s = BedStats()
        _chk(load().itx_bed_get_stats(self._h, C.byref(s)), "itx_bed_get_stats")
        return {k: getattr(s, k) for k, _ in BedStats._fields_}

    def close(self):
        if self._h:
            load().itx_bed_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Gcov:
    """The genome coverage of filter -G built on the device (include/iteres_amd.h itx_gcov_*). `run` takes the per-record arrays as
    torch DEVICE tensors and an int32 tensor of chosen rows (-1: none), `add_host` intervals as host arrays; `finish(order, names)`
    finds the change points, `text(which)` joins the rounds of a file (0: all counted reads, 1: MAPQ >= -Q) into bytes."""

    def __init__(self, chrom_size, params: dict | None = None, batch_capacity: int = 1 << 20, device: int = 0):
        q = dict(mapq_min=10, min_cov=1e-4, extension=150, isize_max=500, treat_pe_as_se=False, discard_half_mapped=False)
        q.update(params or {})
        p = Params(int(q["mapq_min"]), float(q["min_cov"]), int(q["extension"]), int(q["isize_max"]), int(bool(q["treat_pe_as_se"])),
                   int(bool(q["discard_half_mapped"])), MODE_FILTER, ACCUM_DEFAULT)
        cs = np.ascontiguousarray(chrom_size, np.int64)
        self.n_chrom = len(cs)
        self._h = C.c_void_p()
        _chk(load().itx_gcov_create(device, _p(cs), len(cs), C.byref(p), batch_capacity, C.byref(self._h)), "itx_gcov_create")

    def set_tidmap(self, tid2chrom):
        a = np.ascontiguousarray(tid2chrom, np.int32)
        _chk(load().itx_gcov_set_tidmap(self._h, _p(a), len(a)), "itx_gcov_set_tidmap")

    def run(self, hit_row, tid, pos, tmpend, mapq, flag5, mpos=None, isize=None):
        import torch
        ptr = lambda t: None if t is None else t.data_ptr()
        b = Batch(ptr(tid), ptr(pos), ptr(tmpend), ptr(mapq), ptr(flag5), ptr(mpos), ptr(isize))
        _chk(load().itx_gcov_run(self._h, C.byref(b), C.c_void_p(hit_row.data_ptr()), int(hit_row.numel()), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
             "itx_gcov_run")

    def wait_kernels(self):
        _chk(load().itx_gcov_wait_kernels(self._h), "itx_gcov_wait_kernels")

    def add_host(self, chrom, start, end, uniq):
        c, s, e, u = (np.ascontiguousarray(chrom, np.int32), np.ascontiguousarray(start, np.uint32), np.ascontiguousarray(end, np.uint32),
                      np.ascontiguousarray(uniq, np.uint8))
        _chk(load().itx_gcov_add_host(self._h, _p(c), _p(s), _p(e), _p(u), len(c)), "itx_gcov_add_host")

    def finish(self, order, names, round_bytes: int = 0):
        o = np.ascontiguousarray(order, np.uint32)
        names = [n if isinstance(n, bytes) else n.encode() for n in names]
        off = np.zeros(len(names) + 1, np.uint64)
        off[1:] = np.cumsum([len(n) for n in names], dtype=np.uint64)
        blob = np.frombuffer(b"".join(names) + b"\0", np.uint8).copy()
        _chk(load().itx_gcov_finish(self._h, _p(o), len(o), _p(blob), _p(off), round_bytes), "itx_gcov_finish")

    def next(self, which):
        t = GcovText()
        _chk(load().itx_gcov_next(self._h, which, C.byref(t)), "itx_gcov_next")
        return (C.string_at(t.bytes, t.len) if t.len else b""), bool(t.more)

    def text(self, which):
        parts, more = [], True
        while more:
            b, more = self.next(which)
            parts.append(b)
        return b"".join(parts), [len(x) for x in parts]

    def stats(self):
        s = GcovStats()
        _chk(load().itx_gcov_get_stats(self._h, C.byref(s)), "itx_gcov_get_stats")
        return {k: (getattr(s, k) if isinstance(getattr(s, k), (int, float)) else list(getattr(s, k))) for k, _ in GcovStats._fields_}

    def bigwig_build(self, which):
        """builds the bigWig content of file `which` on the device (after finish; before, between or after the text rounds)"""
        _chk(load().itx_gcov_bigwig_build(self._h, which), "itx_gcov_bigwig_build")

    def bigwig(self, which):
        """what bigwig_build made: n_items (0: the file has no data, nothing else is there), chrom (index into chrom_size per bigWig id),
        sec_key (n_sec x 3: id, start, end), sec_count, reductions, sums (per level, the 32-byte records as bytes), blocks (the zlib
        streams: sections, then each level's zoom blocks from slot_first[level] on), and the device times of the build's parts"""
        r = GcovBwResult()
        _chk(load().itx_gcov_bigwig_result(self._h, which, C.byref(r)), "itx_gcov_bigwig_result")
        if not r.n_items:
            return {"n_items": 0}
        arr = lambda p, n, t: np.frombuffer(C.string_at(p, n * np.dtype(t).itemsize), t).copy()
        off = arr(r.block_off, r.n_blocks + 1, np.uint64)
        raw = C.string_at(r.blocks, int(off[-1]))
        return {"n_items": r.n_items, "chrom": arr(r.chrom, r.n_chrom, np.uint32), "sec_key": arr(r.sec_key, 3 * r.n_sec, np.uint32).reshape(-1, 3),
                "sec_count": arr(r.sec_count, r.n_sec, np.uint32), "reductions": list(r.reduction[:r.n_levels]),
                "sums": [C.string_at(r.sum[k], 32 * r.n_sum[k]) for k in range(r.n_levels)], "slot_first": list(r.slot_first[:r.n_levels]),
                "blocks": [raw[int(off[i]):int(off[i + 1])] for i in range(r.n_blocks)], "reduce_rounds": r.reduce_rounds,
                "ms": {"items": r.items_ms, "chain": r.chain_ms, "fold": r.fold_ms, "deflate": r.deflate_ms}}

    def points(self, which):
        """the change points of file `which` as (n, 4) uint32: position, depth from here on, place of the chromosome in finish's order, 0"""
        n = int(self.stats()["points"][which])
        out = np.zeros((n, 4), np.uint32)
        _chk(load().itx_gcov_copy_points(self._h, which, _p(out) if n else None), "itx_gcov_copy_points")
        return out

    def close(self):
        if self._h:
            load().itx_gcov_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Names:
    """The read lists of filter -r built on the device (include/iteres_amd.h itx_names_*, replacing generic.c:662-666 and the list
    part of generic.c:1729-1731). `append_window` takes records of an Inflater's last parsed window and a torch DEVICE int32 tensor
    of their chosen rows (-1: none), `run` plain torch DEVICE tensors (uint8 record bytes, uint32-as-int32 offsets, int32 rows);
    both return how many records need the host's reading (then nothing was appended). `append_host` takes (row, name bytes) pairs.
    `finish(n_rows)` sorts by row, stable in append order, and returns {row: b",".join(names)} with the per-row counts."""

    def __init__(self, batch_capacity: int = 1 << 20, pool_bytes: int = 0, device: int = 0):
        self._h = C.c_void_p()
        _chk(load().itx_names_create(device, batch_capacity, pool_bytes, C.byref(self._h)), "itx_names_create")

    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def append_window(self, inflater, first, n, hit_row):
        hard = C.c_uint64()
        _chk(load().itx_bamwin_names(inflater._h, self._h, first, n, C.c_void_p(hit_row.data_ptr()), self._stream(), C.byref(hard)), "itx_bamwin_names")
        return hard.value

    def run(self, rec_bytes, rec_off, hit_row):
        hard = C.c_uint64()
        _chk(load().itx_names_run(self._h, C.c_void_p(rec_bytes.data_ptr()), C.c_void_p(rec_off.data_ptr()), C.c_void_p(hit_row.data_ptr()), int(hit_row.numel()),
                                  self._stream(), C.byref(hard)), "itx_names_run")
        return hard.value

    def append_host(self, rows, names):
        r = np.ascontiguousarray(rows, np.uint32)
        off = np.zeros(len(r) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
        blob = np.frombuffer(b"".join(names) + b"\0", np.uint8).copy()
        _chk(load().itx_names_append_host(self._h, _p(r), _p(blob), _p(off), len(r)), "itx_names_append_host")

    def wait_kernels(self):
        _chk(load().itx_names_wait_kernels(self._h), "itx_names_wait_kernels")

    def finish(self, n_rows):
        res = NamesResult()
        _chk(load().itx_names_finish(self._h, n_rows, C.byref(res)), "itx_names_finish")
        row_off = np.ctypeslib.as_array(C.cast(res.row_off, C.POINTER(C.c_uint64)), (n_rows,))
        row_cnt = np.ctypeslib.as_array(C.cast(res.row_cnt, C.POINTER(C.c_uint32)), (n_rows,)).copy()
        text = C.string_at(res.text, res.text_bytes) if res.text_bytes else b""
        lists = {}
        for r in np.flatnonzero(row_off != np.uint64(0xffffffffffffffff)):
            o = int(row_off[r])
            lists[int(r)] = text[o:text.index(b"\0", o)]
        return lists, row_cnt, text, int(res.n_entries)

    def stats(self):
        s = NamesStats()
        _chk(load().itx_names_get_stats(self._h, C.byref(s)), "itx_names_get_stats")
        return {k: getattr(s, k) for k, _ in NamesStats._fields_}

    def close(self):
        if self._h:
            load().itx_names_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Bamout:
    """The BAM of filter -b built on the device (include/iteres_amd.h itx_bamout_*): the records that chose a row, gathered into one
    stream of bytes and cut into BGZF members there. `append_window` takes records of an Inflater's last parsed window and a torch
    DEVICE int32 tensor of their chosen rows (-1: none), `run` plain torch DEVICE tensors (uint8 record bytes, uint32-as-int32
    offsets, int32 rows), `append_host` whole records as bytes. Every call collects what is pending, so the members made so far are
    in `self.out` (a bytearray) in stream order; `finish()` adds the last, short member and returns all of them. After
    `sort_enable()` (filter -b -s) nothing leaves during the pass; `sort_all()` in place of `finish()` returns the members of the
    stream sorted by coordinate. `set_level()` (filter -b -l), before the first batch, chooses how the members are encoded."""

    def __init__(self, batch_capacity: int = 1 << 20, stream_bytes: int = 0, device: int = 0):
        self._h = C.c_void_p()
        self.out = bytearray()
        self.last = None                                                   # the last collect's (address, len, room)
        _chk(load().itx_bamout_create(device, batch_capacity, stream_bytes, C.byref(self._h)), "itx_bamout_create")

    _stream = staticmethod(Names._stream)

    def collect(self):
        """the oldest pending batch's members -> self.out; returns their bytes (b"" when nothing was pending or no payload was completed)"""
        m = BamoutMembers()
        _chk(load().itx_bamout_collect(self._h, C.byref(m)), "itx_bamout_collect")
        got = C.string_at(m.bytes, m.len) if m.len else b""
        if m.bytes:
            self.last = (m.bytes, int(m.len), int(m.room))
        self.out += got
        return got

    def _drain(self):
        while load().itx_bamout_pending(self._h):
            self.collect()

    def append_window(self, inflater, first, n, hit_row, collect=True):
        _chk(load().itx_bamwin_bamout(inflater._h, self._h, first, n, C.c_void_p(hit_row.data_ptr()), self._stream()), "itx_bamwin_bamout")
        if collect:
            self._drain()

    def run(self, rec_bytes, rec_off, hit_row, collect=True):
        _chk(load().itx_bamout_run(self._h, C.c_void_p(rec_bytes.data_ptr()), C.c_void_p(rec_off.data_ptr()), C.c_void_p(hit_row.data_ptr()), int(hit_row.numel()),
                                   self._stream()), "itx_bamout_run")
        if collect:
            self._drain()

    def append_host(self, records: bytes, collect=True):
        _chk(load().itx_bamout_append_host(self._h, records, len(records)), "itx_bamout_append_host")
        if collect:
            self._drain()

    def wait_kernels(self):
        _chk(load().itx_bamout_wait_kernels(self._h), "itx_bamout_wait_kernels")

    def finish(self):
        self._drain()                                                      # (the last member needs a place of its own)
        _chk(load().itx_bamout_finish(self._h), "itx_bamout_finish")
        self._drain()
        return bytes(self.out)

    def index_enable(self, l_ref):
        """before the first batch: the .bai index of the stream is built beside it (l_ref: the header's reference lengths)"""
        a = (C.c_int32 * max(len(l_ref), 1))(*l_ref)
        _chk(load().itx_bamout_index_enable(self._h, len(l_ref), a), "itx_bamout_index_enable")

    def index_finish(self, first_member_offset):
        """after finish(): (status, the .bai file's bytes or None, the result's counters)"""
        r = BamoutIndexResult()
        _chk(load().itx_bamout_index_finish(self._h, first_member_offset, C.byref(r)), "itx_bamout_index_finish")
        info = {k: getattr(r, k) for k, _ in BamoutIndexResult._fields_ if k not in ("bytes", "pad")}
        return r.status, (C.string_at(r.bytes, r.len) if r.status == 0 else None), info

    def sort_enable(self):
        """before the first batch: the records are held on the device and leave in coordinate order (sort_next in place of finish)"""
        _chk(load().itx_bamout_sort_enable(self._h), "itx_bamout_sort_enable")

    def sort_next(self, collect=True):
        """after the last batch: sorts (the first call) and replays one round of at most batch_capacity records; True while
        another round follows. `sort_all()` is the whole loop."""
        if collect:
            self._drain()
        more = C.c_int(0)
        _chk(load().itx_bamout_sort_next(self._h, C.byref(more)), "itx_bamout_sort_next")
        if collect:
            self._drain()
        return bool(more.value)

    def sort_all(self):
        while self.sort_next():
            pass
        return bytes(self.out)

    def set_level(self, level: int):
        """before the first batch: the members' level (filter -b -l): 0 stored, 1 the fast encoder, 6 the default"""
        _chk(load().itx_bamout_set_level(self._h, level), "itx_bamout_set_level")

    def level(self):
        return int(load().itx_bamout_get_level(self._h))

    def annotate_enable(self, rows, reps, clas, fams):
        """before the first batch (filter -b -a): every counted record leaves with the tags of its row behind it (csrc/itx_reptag.h).
        rows: a ROW_DTYPE array; reps / clas / fams: the names (bytes) that rows' rep / cla / fam index."""
        rows = np.ascontiguousarray(rows, ROW_DTYPE)
        args = []
        for names in (reps, clas, fams):
            off = np.cumsum([0] + [len(x) for x in names]).astype(np.uint64)
            pool = np.frombuffer(b"".join(names) + b"\0", np.uint8).copy()
            args += [pool, off, len(names)]
        _chk(load().itx_bamout_annotate_enable(self._h, rows.ctypes.data, len(rows), *[a if isinstance(a, int) else a.ctypes.data for a in args]),
             "itx_bamout_annotate_enable")

    def tag_bytes(self):
        n = C.c_uint64(0)
        _chk(load().itx_bamout_annotate_get_stats(self._h, C.byref(n)), "itx_bamout_annotate_get_stats")
        return int(n.value)

    def mates_enable(self):
        """after sort_enable(), before the first batch (filter -b -s -m): the mates of the counted pairs join the sorted stream"""
        _chk(load().itx_bamout_mates_enable(self._h), "itx_bamout_mates_enable")

    def mates_append_host(self, records: bytes):
        """all the records of a window the caller counted itself: the candidate mates among them join the candidate store"""
        _chk(load().itx_bamout_mates_append_host(self._h, records, len(records)), "itx_bamout_mates_append_host")

    def mates_host_rows(self, rows):
        """with annotate_enable(): the chosen rows of the records of the next append_host, one per record"""
        a = np.ascontiguousarray(rows, np.int32)
        _chk(load().itx_bamout_mates_host_rows(self._h, a.ctypes.data, len(a)), "itx_bamout_mates_host_rows")

    def mates_stats(self):
        s = BamoutMatesStats()
        _chk(load().itx_bamout_mates_get_stats(self._h, C.byref(s)), "itx_bamout_mates_get_stats")
        return {k: getattr(s, k) for k, _ in BamoutMatesStats._fields_}

    def sort_stats(self):
        s = BamoutSortStats()
        _chk(load().itx_bamout_sort_get_stats(self._h, C.byref(s)), "itx_bamout_sort_get_stats")
        return {k: getattr(s, k) for k, _ in BamoutSortStats._fields_}

    def stats(self):
        s = BamoutStats()
        _chk(load().itx_bamout_get_stats(self._h, C.byref(s)), "itx_bamout_get_stats")
        return {k: getattr(s, k) for k, _ in BamoutStats._fields_}

    def close(self):
        if self._h:
            load().itx_bamout_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SamText:
    """SAM text split and parsed on the device (include/iteres_amd.h itx_samtext_*, the line rule: csrc/itx_samline.h). `names`: the
    @SQ names as bytes, in header order. `parse(text, final, slot)` returns the result fields as a dict; `fetch(slot, first, n)` the
    records' arrays and side values as numpy arrays. A chunk with a hard line has n_rec == 0: the caller parses it itself."""

    def __init__(self, names, max_chunk_bytes: int = 1 << 20, device: int = 0):
        off = np.zeros(len(names) + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in names], dtype=np.uint64)
        blob = np.frombuffer(b"".join(names) + b"\0", np.uint8).copy()
        self._h = C.c_void_p()
        self._text = {}
        _chk(load().itx_samtext_create(device, _p(blob), _p(off), len(names), max_chunk_bytes, C.byref(self._h)), "itx_samtext_create")

    def begin(self, text: bytes, final: bool, slot: int = 0):
        buf = np.frombuffer(text + b"\0", np.uint8).copy()           # stays alive until the parse has ended
        self._text[slot] = buf
        _chk(load().itx_samtext_parse_begin(self._h, slot, _p(buf), len(text), int(final)), "itx_samtext_parse_begin")

    def end(self, slot: int = 0):
        res = SamTextResult()
        _chk(load().itx_samtext_parse_end(self._h, slot, C.byref(res)), "itx_samtext_parse_end")
        return {k: getattr(res, k) for k, _ in SamTextResult._fields_}

    def parse(self, text: bytes, final: bool, slot: int = 0):
        self.begin(text, final, slot)
        return self.end(slot)

    def begin_bgzf(self, comp: bytes, final: bool, slot: int = 0, skip: int = 0, blocks: np.ndarray | None = None):
        """the members of `comp` (all complete ones, or `blocks`) inflated on the device; the slot's text is the tail the stream's
        previous chunk left, then the inflated bytes from `skip` on"""
        blocks = index_bgzf(comp) if blocks is None else np.ascontiguousarray(blocks, BGZF_BLOCK)
        buf = np.frombuffer(comp + b"\0", np.uint8).copy()           # stays alive until the parse has ended
        self._text[slot] = (buf, blocks)
        _chk(load().itx_samtext_parse_begin_bgzf(self._h, slot, _p(buf), len(comp), _p(blocks) if len(blocks) else _p(np.zeros(1, BGZF_BLOCK)),
                                                 len(blocks), skip, int(final)), "itx_samtext_parse_begin_bgzf")

    def parse_bgzf(self, comp: bytes, final: bool, slot: int = 0, skip: int = 0, blocks: np.ndarray | None = None):
        """-> (the result fields, the BGZF fields: text_len, carry_len, tail_len, n_bad, first_bad, inflate_ms)"""
        self.begin_bgzf(comp, final, slot, skip, blocks)
        res = self.end(slot)
        return res, self.bgzf_info(slot)

    def bgzf_info(self, slot: int = 0):
        info = SamTextBgzfInfo()
        _chk(load().itx_samtext_bgzf_info(self._h, slot, C.byref(info)), "itx_samtext_bgzf_info")
        return {k: getattr(info, k) for k, _ in SamTextBgzfInfo._fields_}

    def text(self, slot: int = 0, off: int = 0, n: int | None = None) -> bytes:
        """bytes [off, off + n) of the slot's text (all of it by default: its length is known for a BGZF chunk only)"""
        if n is None:
            n = self.bgzf_info(slot)["text_len"] - off
        out = np.zeros(n + 1, np.uint8)
        _chk(load().itx_samtext_text(self._h, slot, off, _p(out), n), "itx_samtext_text")
        return out[:n].tobytes()

    def strings(self, slot, first, n, want=3):
        """-> (the packed text, qname_at, xa_at, the 16 bytes the object keeps behind the text): read names (want & 1) and XA values
        (want & 2) of records [first, first + n), each followed by a NUL; SAMTEXT_NO_STRING where a record has none"""
        o = SamTextStrings()
        _chk(load().itx_samtext_strings(self._h, slot, first, n, want, C.byref(o)), "itx_samtext_strings")
        if not n:
            return b"", np.zeros(0, np.uint32), np.zeros(0, np.uint32), b""
        raw = C.string_at(o.text, o.text_len + 16)
        at = lambda p: np.frombuffer(C.string_at(p, 4 * n), np.uint32).copy()
        return raw[:o.text_len], at(o.qname_at), at(o.xa_at), raw[o.text_len:]

    def fetch(self, slot, first, n, side=True):
        a = {k: np.full(n + 1, 7, dt) for k, dt in (("tid", np.int32), ("pos", np.int32), ("tmpend", np.int32), ("mapq", np.uint8), ("flag5", np.uint8),
                                                      ("mpos", np.int32), ("isize", np.int32))}
        st = Staging(*[_p(a[k]) for k in ("tid", "pos", "tmpend", "mapq", "flag5", "mpos", "isize")], None, n)
        s = {k: np.full(n + 1, 7, dt) for k, dt in (("line_off", np.uint32), ("qname_len", np.uint32), ("xa_off", np.uint32), ("xa_len", np.uint32),
                                                        ("nm", np.int32), ("xa_mark", np.uint8))} if side else {}
        ptrs = [_p(s[k]) if side else None for k in ("line_off", "qname_len", "xa_off", "xa_len", "nm", "xa_mark")]
        _chk(load().itx_samtext_fetch(self._h, slot, first, n, C.byref(st), 0, *ptrs), "itx_samtext_fetch")
        a.update(s)
        return {k: v[:n] for k, v in a.items()}

    def close(self):
        if self._h:
            load().itx_samtext_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
