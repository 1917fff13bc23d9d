"""ctypes binding of libmcensus_hip.so (include/mcensus.h).  No CPU fallback: if the HIP library is
missing or no MI355X is visible, importing the engine fails loudly."""
import contextlib
import ctypes as C
import gzip
import json
import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmcensus_hip.so")
DATA_DIR = os.path.join(_HERE, "data")


class McRow(C.Structure):
    _fields_ = [("query", C.c_int32), ("subject", C.c_int32), ("ident", C.c_double), ("alnlen", C.c_int32),
                ("mismatch", C.c_int32), ("gapopen", C.c_int32), ("qstart", C.c_int32), ("qend", C.c_int32),
                ("sstart", C.c_int32), ("send", C.c_int32), ("loge", C.c_double), ("bits", C.c_double),
                ("score", C.c_int32), ("nmatch", C.c_int32)]


class McBestHit(C.Structure):
    _fields_ = [("read", C.c_int32), ("family", C.c_int32), ("aln", C.c_int32), ("target_len", C.c_int32),
                ("bits", C.c_double)]


class McStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("reads", "seed_tasks", "gap_tasks", "hsps", "rows", "reads_with_rows", "classified", "bucket_lookups", "key_probes")] + \
               [(n, C.c_float) for n in ("ms_translate", "ms_seed", "ms_eval", "ms_gapped", "ms_sort", "ms_finish", "ms_total")] + \
               [("_pad", C.c_float)] + [(n, C.c_int64) for n in ("seed_exact_asks", "seed_wild_asks", "seed_pair_asks", "seed_probes", "range_splits")]


class McLibrary(C.Structure):
    _fields_ = [("paired_end", C.c_int32), ("insert", C.c_int32), ("error_model", C.c_int32), ("error_rate", C.c_double)]


ERROR_MODELS = {None: 0, "uniform": 1, "illumina": 2}       # mc_library.error_model (MC_ERR_NONE, MC_ERR_UNIFORM, MC_ERR_ILLUMINA)


class McReaderStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("sampled", "too_short", "low_qual", "dups", "records", "bases", "exhausted", "ragged_end")]


ROW_DTYPE = np.dtype([("query", "<i4"), ("subject", "<i4"), ("ident", "<f8"), ("alnlen", "<i4"), ("mismatch", "<i4"),
                      ("gapopen", "<i4"), ("qstart", "<i4"), ("qend", "<i4"), ("sstart", "<i4"), ("send", "<i4"),
                      ("loge", "<f8"), ("bits", "<f8"), ("score", "<i4"), ("nmatch", "<i4")], align=True)
BEST_DTYPE = np.dtype([("read", "<i4"), ("family", "<i4"), ("aln", "<i4"), ("target_len", "<i4"), ("bits", "<f8")], align=True)
REC_DESC_DTYPE = np.dtype([("h1", "<u8"), ("h2", "<u8"), ("seq_off", "<u8"), ("len", "<u4"), ("flags", "u1"), ("pad", "u1", (3,))])   # mc_rec_desc

_lib = None


def _share_hip_runtime():
    """One HIP runtime per process.  A PyTorch-ROCm wheel brings its own copy of libamdhip64 (file name libamdhip64.so, SONAME
    libamdhip64.so.7); this library needs libamdhip64.so.7.  With torch imported first the loader hands this library torch's copy (the
    SONAME matches) and all is well; the other way round torch asks for "libamdhip64.so", which matches nothing loaded, gets its own
    copy beside the system's, and the second runtime fails to initialise the GPU.  So: where a torch with a HIP
    runtime of its own is installed and not yet imported, that copy is loaded first and both use it - in whatever order the application
    then imports them.  MCENSUS_HIP_RUNTIME=system in the environment: leave it to the loader."""
    if os.environ.get("MCENSUS_HIP_RUNTIME", "") == "system" or "torch" in sys.modules:
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so") if spec is not None and spec.origin else None
        if cand and os.path.isfile(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:                                   # (no torch, or one without a runtime of its own: the system's it is)
        pass


def load_library():
    """Load libmcensus_hip.so and declare the prototypes of include/mcensus.h."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MCENSUS_LIB", LIB_PATH)      # development: an alternative build of the same library
    if not os.path.isfile(path):
        raise RuntimeError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
    _share_hip_runtime()
    lib = C.CDLL(path)
    lib.mc_last_error.restype = C.c_char_p
    lib.mc_device_count.restype = C.c_int
    lib.mc_open.restype = C.c_void_p
    lib.mc_open.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32]
    lib.mc_close.argtypes = [C.c_void_p]
    lib.mc_set_index_cache.argtypes = [C.c_char_p]
    lib.mc_index_cache_check.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int32, C.c_char_p]
    lib.mc_open_rapdb.restype = C.c_void_p
    lib.mc_open_rapdb.argtypes = [C.c_char_p, C.c_int32]
    lib.mc_marker_count.restype = C.c_int32
    lib.mc_marker_count.argtypes = [C.c_void_p]
    lib.mc_marker_name.restype = C.c_char_p
    lib.mc_marker_name.argtypes = [C.c_void_p, C.c_int32]
    lib.mc_set_families.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]
    lib.mc_rapdb_verify.argtypes = [C.c_char_p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int32]
    lib.mc_rapdb_write.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int32, C.c_char_p]
    lib.mc_index_view.argtypes = [C.c_void_p] + [C.POINTER(C.c_void_p)] * 5 + [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.POINTER(C.c_double)]
    lib.mc_set_run.argtypes = [C.c_void_p, C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.mc_search.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
    lib.mc_search_varlen.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
    lib.mc_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.mc_run.argtypes = [C.c_void_p, C.c_int64]
    lib.mc_attach.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.mc_run_range.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64]
    lib.mc_set_counting.argtypes = [C.c_void_p, C.c_int]
    lib.mc_debug_stage.restype = C.c_int64
    lib.mc_debug_stage.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]
    lib.mc_range_begin.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64]
    lib.mc_range_end.argtypes = [C.c_void_p]
    lib.mc_ranges_in_flight.argtypes = [C.c_void_p]
    lib.mc_ranges_translated_ahead.restype = C.c_int64
    lib.mc_ranges_translated_ahead.argtypes = [C.c_void_p]
    lib.mc_ahead_kernel_ms.restype = C.c_float
    lib.mc_ahead_kernel_ms.argtypes = [C.c_void_p]
    lib.mc_result_rows.restype = C.c_int64
    lib.mc_result_rows.argtypes = [C.c_void_p, C.POINTER(C.POINTER(McRow))]
    lib.mc_result_best_hits.restype = C.c_int64
    lib.mc_result_best_hits.argtypes = [C.c_void_p, C.POINTER(C.POINTER(McBestHit))]
    lib.mc_result_stats.argtypes = [C.c_void_p, C.POINTER(McStats)]
    lib.mc_write_m8.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    lib.mc_write_m8_named.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.POINTER(C.c_char_p), C.c_int64, C.c_int64]
    lib.mc_reader_last_error.restype = C.c_char_p
    lib.mc_set_host_threads.restype = None
    lib.mc_set_host_threads.argtypes = [C.c_int32]
    lib.mc_reader_open.restype = C.c_void_p
    lib.mc_reader_open.argtypes = [C.POINTER(C.c_char_p), C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_char_p]
    lib.mc_reader_open_range.restype = C.c_void_p
    lib.mc_reader_open_range.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double]
    lib.mc_reader_run.restype = C.c_int64
    lib.mc_reader_run.argtypes = [C.c_void_p]
    lib.mc_reader_reads.restype = C.POINTER(C.c_uint8)
    lib.mc_reader_reads.argtypes = [C.c_void_p]
    lib.mc_reader_get_stats.argtypes = [C.c_void_p, C.POINTER(McReaderStats)]
    lib.mc_reader_open_bz2_part.restype = C.c_void_p
    lib.mc_reader_open_bz2_part.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double]
    lib.mc_bz2_blocks.restype = C.c_int64
    lib.mc_bz2_blocks.argtypes = [C.c_char_p]
    lib.mc_gz_chunks.restype = C.c_int64
    lib.mc_gz_chunks.argtypes = [C.c_char_p, C.c_int64]
    lib.mc_reader_open_gz_part.restype = C.c_void_p
    lib.mc_reader_open_gz_part.argtypes = [C.c_char_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double]
    lib.mc_reader_gz_provide.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    lib.mc_reader_gz_end_state.restype = C.c_int64
    lib.mc_reader_gz_end_state.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.mc_reader_gz_finish.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p]
    lib.mc_reader_describe.restype = C.c_int64
    lib.mc_reader_describe.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.mc_dupset_open.restype = C.c_void_p
    lib.mc_dupset_close.argtypes = [C.c_void_p]
    lib.mc_dupset_walk.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_void_p]
    lib.mc_reader_take.restype = C.c_int64
    lib.mc_reader_take.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.mc_reader_times.restype = C.c_int32
    lib.mc_reader_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32]
    lib.mc_reader_close.argtypes = [C.c_void_p]
    lib.mc_reader_trim.restype = None
    lib.mc_reader_trim.argtypes = [C.c_int64]
    lib.mc_count_bases.restype = C.c_int64
    lib.mc_count_bases.argtypes = [C.POINTER(C.c_char_p), C.c_int32]
    lib.mc_quality_offset.restype = C.c_int32
    lib.mc_quality_offset.argtypes = [C.c_char_p]
    lib.mc_reader_start.argtypes = [C.c_void_p]
    lib.mc_reader_fetch.restype = C.c_int64
    lib.mc_reader_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
    lib.mc_reader_join.restype = C.c_int64
    lib.mc_reader_join.argtypes = [C.c_void_p]
    lib.mc_reader_read_len.restype = C.c_int32
    lib.mc_reader_read_len.argtypes = [C.c_void_p]
    lib.mc_reader_nreads.restype = C.c_int64
    lib.mc_reader_nreads.argtypes = [C.c_void_p]
    lib.mc_search_files.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.mc_search_files_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int64]
    lib.mc_set_keep_rows.argtypes = [C.c_void_p, C.c_int]
    lib.mc_set_best_hits_only.argtypes = [C.c_void_p, C.c_int]
    lib.mc_grid_classify.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_double), C.c_int32,
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    lib.mc_bootstrap.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    lib.mc_bootstrap_ms.restype = C.c_float
    lib.mc_bootstrap_ms.argtypes = [C.c_void_p]
    lib.mc_fit_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.mc_weights_mue.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.mc_fit_weights_ms.restype = C.c_float
    lib.mc_fit_weights_ms.argtypes = [C.c_void_p]
    lib.mc_genome_open.restype = C.c_void_p
    lib.mc_genome_open.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    lib.mc_genome_close.restype = None
    lib.mc_genome_close.argtypes = [C.c_void_p]
    lib.mc_genome_set_library.argtypes = [C.c_void_p, C.c_void_p]
    lib.mc_simulate.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.mc_train_library.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int32), C.c_int32,
                                     C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    lib.mc_train_times.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.mc_genome_set_read_lengths.argtypes = [C.c_void_p, C.c_int32]
    lib.mc_simulate_varlen.restype = C.c_int64
    lib.mc_simulate_varlen.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_int64, C.c_void_p]
    lib.mc_train_library_bases.restype = C.c_int64
    lib.mc_train_library_bases.argtypes = [C.c_void_p]
    lib.mc_community_open.restype = C.c_void_p
    lib.mc_community_open.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    lib.mc_community_close.restype = None
    lib.mc_community_close.argtypes = [C.c_void_p]
    lib.mc_community_set_library.argtypes = [C.c_void_p, C.c_void_p]
    lib.mc_community_simulate.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.mc_community_library.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_uint64]
    lib.mc_community_member_reads.argtypes = [C.c_void_p, C.c_void_p]
    lib.mc_community_times.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    lib.mc_set_run_classes.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.mc_search_classes.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64]
    lib.mc_result_best_classes.restype = C.c_int64
    lib.mc_result_best_classes.argtypes = [C.c_void_p, C.POINTER(C.POINTER(C.c_uint8))]
    lib.mc_result_class_reads.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.mc_debug_classes_prologue.restype = C.c_int64
    lib.mc_debug_classes_prologue.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_float)]
    lib.mc_reader_open_classes.restype = C.c_void_p
    lib.mc_reader_open_classes.argtypes = [C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_char_p]
    lib.mc_reader_stride.restype = C.c_int32
    lib.mc_reader_stride.argtypes = [C.c_void_p]
    lib.mc_set_abundance.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int32, C.c_double, C.c_double]
    lib.mc_abundance_reset.argtypes = [C.c_void_p]
    lib.mc_abundance_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.mc_abundance_ms.restype = C.c_float
    lib.mc_abundance_ms.argtypes = [C.c_void_p]
    lib.mc_set_coverage.argtypes = [C.c_void_p, C.c_int]
    lib.mc_coverage_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mc_coverage_depth.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.mc_coverage_ms.restype = C.c_float
    lib.mc_coverage_ms.argtypes = [C.c_void_p]
    lib.mc_set_ties.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32]
    lib.mc_ties_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.mc_ties_coverage_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mc_ties_ms.restype = C.c_float
    lib.mc_ties_ms.argtypes = [C.c_void_p]
    lib.mc_set_curve.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.mc_curve_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.mc_curve_k.restype = C.c_int32
    lib.mc_curve_k.argtypes = [C.c_void_p]
    lib.mc_curve_ms.restype = C.c_float
    lib.mc_curve_ms.argtypes = [C.c_void_p]
    lib.mc_set_gene_bootstrap.argtypes = [C.c_void_p, C.c_int64]
    lib.mc_gene_bootstrap.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.mc_gene_bootstrap_ms.restype = C.c_float
    lib.mc_gene_bootstrap_ms.argtypes = [C.c_void_p]
    lib.mc_group_bootstrap.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.mc_group_bootstrap_ms.restype = C.c_float
    lib.mc_group_bootstrap_ms.argtypes = [C.c_void_p]
    lib.mc_group_bootstrap_kernels_ms.restype = None
    lib.mc_group_bootstrap_kernels_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.mc_set_tie_bootstrap.argtypes = [C.c_void_p, C.c_int64]
    lib.mc_tie_bootstrap.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.mc_tie_bootstrap_ms.restype = C.c_float
    lib.mc_tie_bootstrap_ms.argtypes = [C.c_void_p]
    lib.mc_tie_bootstrap_kernels_ms.restype = None
    lib.mc_tie_bootstrap_kernels_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.mc_set_coverage_bootstrap.argtypes = [C.c_void_p, C.c_int64]
    lib.mc_coverage_bootstrap.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    lib.mc_coverage_bootstrap_ms.restype = C.c_float
    lib.mc_coverage_bootstrap_ms.argtypes = [C.c_void_p]
    lib.mc_coverage_bootstrap_kernels_ms.restype = None
    lib.mc_coverage_bootstrap_kernels_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.mc_set_abundance_classes.argtypes = [C.c_void_p, C.c_int]
    lib.mc_abundance_classes_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.mc_abundance_classes_ms.restype = C.c_float
    lib.mc_abundance_classes_ms.argtypes = [C.c_void_p]
    lib.mc_open_stats.restype = C.c_void_p
    lib.mc_open_stats.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_int64, C.c_int32]
    lib.mc_set_gene_fold.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mc_gene_fold_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mc_abundance_count.restype = C.c_int32
    lib.mc_abundance_count.argtypes = [C.c_void_p]
    lib.mc_abundance_residues.restype = C.c_int64
    lib.mc_abundance_residues.argtypes = [C.c_void_p]
    lib.mc_depth_stats.argtypes = [C.c_void_p, C.c_int32, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mc_depth_stats_ms.restype = C.c_float
    lib.mc_depth_stats_ms.argtypes = [C.c_void_p]
    lib.mc_set_identity.argtypes = [C.c_void_p, C.c_int]
    lib.mc_identity_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.mc_identity_hist.argtypes = [C.c_void_p, C.c_void_p]
    lib.mc_identity_ms.restype = C.c_float
    lib.mc_identity_ms.argtypes = [C.c_void_p]
    lib.mc_identity_scan_ms.restype = C.c_float
    lib.mc_identity_scan_ms.argtypes = [C.c_void_p]
    lib.mc_debug_live.restype = None
    lib.mc_debug_live.argtypes = [C.POINTER(C.c_int64)]
    _lib = lib
    return lib


EXPORTED_SYMBOLS = ["mc_last_error", "mc_device_count", "mc_open", "mc_close", "mc_set_index_cache", "mc_index_cache_check", "mc_open_rapdb", "mc_marker_count", "mc_marker_name", "mc_set_families", "mc_rapdb_verify", "mc_rapdb_write", "mc_index_view", "mc_set_run", "mc_search", "mc_search_varlen",
                    "mc_upload", "mc_attach", "mc_run", "mc_run_range", "mc_set_counting", "mc_debug_stage", "mc_range_begin", "mc_range_end", "mc_ranges_in_flight", "mc_ranges_translated_ahead", "mc_ahead_kernel_ms", "mc_result_rows", "mc_result_best_hits", "mc_result_stats", "mc_write_m8", "mc_write_m8_named",
                    "mc_reader_last_error", "mc_set_host_threads", "mc_reader_open", "mc_reader_open_range", "mc_reader_open_bz2_part", "mc_bz2_blocks", "mc_gz_chunks", "mc_reader_open_gz_part", "mc_reader_gz_provide", "mc_reader_gz_end_state", "mc_reader_gz_finish", "mc_reader_run", "mc_reader_reads", "mc_reader_get_stats", "mc_reader_times", "mc_reader_describe", "mc_dupset_open", "mc_dupset_close", "mc_dupset_walk", "mc_reader_take", "mc_reader_close", "mc_reader_trim", "mc_count_bases", "mc_quality_offset",
                    "mc_reader_start", "mc_reader_fetch", "mc_reader_join", "mc_reader_read_len", "mc_reader_nreads", "mc_search_files", "mc_search_files_multi", "mc_set_keep_rows", "mc_set_best_hits_only", "mc_grid_classify", "mc_bootstrap", "mc_bootstrap_ms",
                    "mc_fit_weights", "mc_weights_mue", "mc_fit_weights_ms",
                    "mc_genome_open", "mc_genome_close", "mc_genome_set_library", "mc_simulate", "mc_train_library", "mc_train_times",
                    "mc_genome_set_read_lengths", "mc_simulate_varlen", "mc_train_library_bases",
                    "mc_community_open", "mc_community_close", "mc_community_set_library", "mc_community_simulate", "mc_community_library", "mc_community_member_reads",
                    "mc_community_times",
                    "mc_set_run_classes", "mc_search_classes", "mc_result_best_classes", "mc_result_class_reads", "mc_debug_classes_prologue", "mc_reader_open_classes", "mc_reader_stride",
                    "mc_set_abundance", "mc_abundance_reset", "mc_abundance_read", "mc_abundance_ms",
                    "mc_set_coverage", "mc_coverage_read", "mc_coverage_depth", "mc_coverage_ms", "mc_depth_stats", "mc_depth_stats_ms",
                    "mc_set_ties", "mc_ties_read", "mc_ties_coverage_read", "mc_ties_ms",
                    "mc_set_curve", "mc_curve_read", "mc_curve_k", "mc_curve_ms",
                    "mc_set_gene_bootstrap", "mc_gene_bootstrap", "mc_gene_bootstrap_ms", "mc_group_bootstrap", "mc_group_bootstrap_ms", "mc_group_bootstrap_kernels_ms",
                    "mc_set_tie_bootstrap", "mc_tie_bootstrap", "mc_tie_bootstrap_ms", "mc_tie_bootstrap_kernels_ms",
                    "mc_set_coverage_bootstrap", "mc_coverage_bootstrap", "mc_coverage_bootstrap_ms", "mc_coverage_bootstrap_kernels_ms",
                    "mc_set_abundance_classes", "mc_abundance_classes_read", "mc_abundance_classes_ms", "mc_open_stats", "mc_set_gene_fold", "mc_gene_fold_stats",
                    "mc_abundance_count", "mc_abundance_residues",
                    "mc_set_identity", "mc_identity_read", "mc_identity_hist", "mc_identity_ms", "mc_identity_scan_ms", "mc_debug_live"]


class DupSet:
    """The sampler's set of accepted sequences for -d, walked over record descriptors (mc_dupset_*): verdicts in file order."""

    def __init__(self):
        self.lib = load_library()
        self.s = self.lib.mc_dupset_open()
        if not self.s:
            raise RuntimeError(self.lib.mc_reader_last_error().decode())

    def walk(self, path, descs):
        import numpy as np
        d = np.ascontiguousarray(descs)
        v = np.empty(len(d), np.uint8)
        if self.lib.mc_dupset_walk(self.s, path.encode(), d.ctypes.data, len(d), v.ctypes.data) != 0:
            raise RuntimeError(self.lib.mc_reader_last_error().decode())
        return v

    def close(self):
        if getattr(self, "s", None):
            self.lib.mc_dupset_close(self.s)
            self.s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ReferenceError_(Exception):
    """The reference's Python would have raised inside run_pipeline (which prints the error and returns None)."""


class Reader:
    """The native sampler (mc_reader_*): process_seqfile's rules on plain / .gz / .bz2 FASTA / FASTQ files.  Needs no GPU."""

    def __init__(self, paths, read_len, nreads, fastq, quality_offset, min_quality, mean_quality, max_unknown, filter_dups, fasta_out=None):
        lib = load_library()
        if nreads is None:                   # the reference's "no cap" (its `read_id == args['nreads']` is never true for None)
            nreads = (1 << 63) - 1
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        self.lib, self.read_len = lib, read_len
        self.r = lib.mc_reader_open(arr, len(paths), read_len, nreads, 1 if fastq else 0, int(quality_offset), float(min_quality), float(mean_quality),
                                    float(max_unknown), 1 if filter_dups else 0, fasta_out.encode() if fasta_out else None)
        if not self.r:
            raise RuntimeError(lib.mc_reader_last_error().decode())

    @classmethod
    def with_classes(cls, paths, class_len, nreads, fastq, quality_offset, min_quality, mean_quality, max_unknown, filter_dups, fasta_out=None):
        """The sampler under length classes (mc_reader_open_classes): a record's L is the largest class length it reaches; rows of
        class_len[-1] bytes, the read's first L bases and then 0 bytes.  read_len is the row stride."""
        lib = load_library()
        self = cls.__new__(cls)
        if nreads is None:
            nreads = (1 << 63) - 1
        arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
        cl = (C.c_int32 * len(class_len))(*[int(x) for x in class_len])
        self.lib, self.class_len = lib, [int(x) for x in class_len]
        self.r = lib.mc_reader_open_classes(arr, len(paths), cl, len(class_len), nreads, 1 if fastq else 0, int(quality_offset), float(min_quality), float(mean_quality),
                                            float(max_unknown), 1 if filter_dups else 0, fasta_out.encode() if fasta_out else None)
        if not self.r:
            raise RuntimeError(lib.mc_reader_last_error().decode())
        self.read_len = lib.mc_reader_stride(self.r)
        return self

    @classmethod
    def on_range(cls, path, byte_lo, byte_hi, read_len, nreads, fastq, quality_offset, min_quality, mean_quality, max_unknown):
        """The sampler on the records that start in [byte_lo, byte_hi) of one plain file (mc_reader_open_range)."""
        lib = load_library()
        self = cls.__new__(cls)
        self.lib, self.read_len = lib, read_len
        if nreads is None:
            nreads = (1 << 63) - 1
        self.r = lib.mc_reader_open_range(path.encode(), int(byte_lo), int(byte_hi), read_len, nreads, 1 if fastq else 0, int(quality_offset), float(min_quality),
                                          float(mean_quality), float(max_unknown))
        if not self.r:
            raise RuntimeError(lib.mc_reader_last_error().decode())
        return self

    @classmethod
    def on_bz2_part(cls, path, block_lo, block_hi, kind, read_len, nreads, fastq, quality_offset, min_quality, mean_quality, max_unknown):
        """The sampler on the records that start in the text of blocks [block_lo, block_hi) of one .bz2 file (mc_reader_open_bz2_part)."""
        lib = load_library()
        self = cls.__new__(cls)
        self.lib, self.read_len = lib, read_len
        if nreads is None:
            nreads = (1 << 63) - 1
        self.r = lib.mc_reader_open_bz2_part(path.encode(), int(block_lo), int(block_hi), ord(kind), read_len, nreads, 1 if fastq else 0, int(quality_offset),
                                             float(min_quality), float(mean_quality), float(max_unknown))
        if not self.r:
            raise RuntimeError(lib.mc_reader_last_error().decode())
        return self

    @classmethod
    def on_gz_part(cls, path, chunk_lo, chunk_hi, chunk_bytes, kind, read_len, nreads, fastq, quality_offset, min_quality, mean_quality, max_unknown):
        """The sampler on the records that start in the text of chunks [chunk_lo, chunk_hi) of one .gz file (mc_reader_open_gz_part): start() it,
        gz_provide() the state of the slice in front (not for chunk 0), gz_end_state() for the next slice's owner, join(), gz_finish()."""
        lib = load_library()
        self = cls.__new__(cls)
        self.lib, self.read_len = lib, read_len
        if nreads is None:
            nreads = (1 << 63) - 1
        self.r = lib.mc_reader_open_gz_part(path.encode(), int(chunk_lo), int(chunk_hi), int(chunk_bytes), ord(kind), read_len, nreads, 1 if fastq else 0, int(quality_offset),
                                            float(min_quality), float(mean_quality), float(max_unknown))
        if not self.r:
            raise RuntimeError(lib.mc_reader_last_error().decode())
        return self

    def start(self):
        if self.lib.mc_reader_start(self.r) != 0:
            raise RuntimeError(self.lib.mc_reader_last_error().decode())

    def join(self):
        return self.check(self.lib.mc_reader_join(self.r))

    def gz_provide(self, state):
        self.lib.mc_reader_gz_provide(self.r, state if state else None, len(state) if state else 0)

    def gz_end_state(self):
        """bytes for the owner of the next slice, or None when this slice failed"""
        buf = C.create_string_buffer(32768 + 64)
        n = self.lib.mc_reader_gz_end_state(self.r, buf, len(buf))
        return None if n < 0 else buf.raw[:n]

    def gz_finish(self, crc_in):
        """crc_in / result: 12 bytes (CRC | length of the open member's bytes so far); raises ReferenceError_ on a CRC mismatch"""
        out = C.create_string_buffer(12)
        self.check(self.lib.mc_reader_gz_finish(self.r, crc_in, out))
        return out.raw

    def close(self):
        if getattr(self, "r", None):
            self.lib.mc_reader_close(self.r)
            self.r = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, n):
        if n == -3:
            raise ReferenceError_(self.lib.mc_reader_last_error().decode())
        if n < 0:
            raise RuntimeError(self.lib.mc_reader_last_error().decode())
        return n

    def run(self):
        return self.check(self.lib.mc_reader_run(self.r))

    def stats(self):
        st = McReaderStats()
        self.lib.mc_reader_get_stats(self.r, C.byref(st))
        return {k: getattr(st, k) for k, _ in McReaderStats._fields_}

    def describe(self):
        """The records of the window of a reader opened with on_range, one 32-byte descriptor each (mc_reader_describe): a numpy
        structured array (a copy: it travels to the other ranks)."""
        import numpy as np
        p = C.c_void_p()
        n = self.check(self.lib.mc_reader_describe(self.r, C.byref(p)))
        if n == 0:
            return np.zeros(0, REC_DESC_DTYPE)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n * REC_DESC_DTYPE.itemsize,)).view(REC_DESC_DTYPE).copy()

    def take(self, verdicts, max_take):
        """(k, read_len) uint8: the accepted reads of the described window (verdict bit 8), at most max_take (mc_reader_take)."""
        import numpy as np
        v = np.ascontiguousarray(verdicts, dtype=np.uint8)
        k = int(min(max_take, int(np.count_nonzero(v & 8))))
        out = np.empty((k, self.read_len), np.uint8)
        got = self.check(self.lib.mc_reader_take(self.r, v.ctypes.data, len(v), k, out.ctypes.data))
        return out[:got]

    def times(self):
        """Seconds of the last run by phase (mc_reader_times)."""
        v = (C.c_double * 7)()
        k = self.lib.mc_reader_times(self.r, v, 7)
        names = ("run", "input_wait", "guesses", "parse", "stitch", "verdicts_places_copies", "dup_class_walkers")
        return {names[i]: round(v[i], 4) for i in range(max(k, 0))}

    def reads(self, n):
        """(n, read_len) uint8 view of the sampled reads; it keeps the reader alive."""
        if not n:
            return np.zeros((0, self.read_len), np.uint8)
        buf = (C.c_uint8 * (n * self.read_len)).from_address(C.addressof(self.lib.mc_reader_reads(self.r).contents))
        buf._owner = self
        a = np.frombuffer(buf, dtype=np.uint8).reshape(n, self.read_len)
        return a


def sample_reads(paths, read_len, nreads, fastq, quality_offset, min_quality, mean_quality, max_unknown, filter_dups, fasta_out=None):
    """Native process_seqfile: returns (reads uint8 (n, read_len), stats dict).  Needs no GPU."""
    rd = Reader(paths, read_len, nreads, fastq, quality_offset, min_quality, mean_quality, max_unknown, filter_dups, fasta_out)
    n = rd.run()
    return rd.reads(n), rd.stats()


def count_bases(paths):
    lib = load_library()
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    n = lib.mc_count_bases(arr, len(paths))
    if n == -3:
        raise ReferenceError_(lib.mc_reader_last_error().decode())
    if n < 0:
        raise RuntimeError(lib.mc_reader_last_error().decode())
    return n


def gz_chunks(path, chunk_bytes=1 << 20):
    """Chunks the parallel gzip reader cuts a .gz file into (mc_gz_chunks), or -1."""
    return int(load_library().mc_gz_chunks(path.encode(), int(chunk_bytes)))


def bz2_blocks(path):
    """Blocks of a .bz2 file all of whose streams check out (mc_bz2_blocks), or -1."""
    return int(load_library().mc_bz2_blocks(path.encode()))


def quality_offset(path):
    """auto_detect_quality_offset by the native parser: 32 or 64; None when the Python path has to decide (a record without
    qualities, an unreadable file: it then fails the way the reference does)."""
    v = load_library().mc_quality_offset(path.encode())
    return v if v in (32, 64) else None


def debug_live():
    """Test aid (mc_debug_live): the device buffers, pinned host buffers, streams and events the library holds in this process."""
    out = (C.c_int64 * 4)()
    load_library().mc_debug_live(out)
    return tuple(out)


def rapdb_verify(rapdb_path, names, seqs):
    """0 when the prerapsearch database holds exactly the index mc_open() builds from (names, seqs).  No GPU involved."""
    lib = load_library()
    n = len(names)
    return lib.mc_rapdb_verify(rapdb_path.encode(), (C.c_char_p * n)(*[s.encode() for s in names]), (C.c_char_p * n)(*[s.encode() for s in seqs]), n)


def rapdb_write(names, seqs, path):
    """Writes <path> and <path>.info as `prerapsearch -d markers.faa -n <path>` would.  No GPU involved."""
    lib = load_library()
    n = len(names)
    if lib.mc_rapdb_write((C.c_char_p * n)(*[s.encode() for s in names]), (C.c_char_p * n)(*[s.encode() for s in seqs]), n, path.encode()) != 0:
        raise RuntimeError(lib.mc_last_error().decode())


def load_markers(path=None):
    """(names, seqs) of the canonical marker FASTA shipped as package data."""
    path = path or os.path.join(DATA_DIR, "markers.faa.gz")
    names, seqs = [], []
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rt") as f:
        for line in f:
            if line.startswith(">"):
                names.append(line[1:].split()[0])
                seqs.append([])
            else:
                seqs[-1].append(line.strip())
    return names, ["".join(s) for s in seqs]


def load_model(path=None):
    """The packaged model.json, or the one at `path` (a file, or a model directory holding model.json)."""
    if path and os.path.isdir(path):
        path = os.path.join(path, "model.json")
    with open(path or os.path.join(DATA_DIR, "model.json")) as f:
        return json.load(f)


ALN_STAT = {"hits": 0, "cov": 1, "aln": 2}


def _wfit_default(name):
    """a default of the weight fit, read out of csrc/mc_wfit.h (the one statement)"""
    import re
    with open(os.path.join(_HERE, "csrc", "mc_wfit.h")) as f:
        return int(re.search(r"#define\s+%s\s+(\d+)" % name, f.read()).group(1))


WFIT_DEFAULT_C, WFIT_DEFAULT_G = _wfit_default("MC_WFIT_C"), _wfit_default("MC_WFIT_G")


def user_cache_dir():
    """~/.cache/microbecensus_amd (XDG_CACHE_HOME honoured), created with mode 0700; None when it cannot be made or is not this
    user's alone (owned by somebody else, or group / world writable) - nothing is cached then."""
    root = os.path.join(os.environ.get("XDG_CACHE_HOME") or os.path.join(os.path.expanduser("~"), ".cache"), "microbecensus_amd")
    return _private_dir(root)


def _private_dir(root):
    """root, made with mode 0700 if it is not there; None when it cannot be made or is not this user's alone."""
    try:
        os.makedirs(root, mode=0o700, exist_ok=True)
        st = os.stat(root)
        if st.st_uid != os.getuid() or (st.st_mode & 0o022):
            return None
    except OSError:
        return None
    return root


_index_cache_set = False


def use_index_cache():
    """Points mc_open() at the per-user cache of built indexes (once per process; MC_INDEX_CACHE=0 in the environment: no cache,
    MC_INDEX_CACHE=<dir>: that directory - like the default one only if it is this user's alone: a cached index is
    read back into device arrays the kernels index, and although mc_open compares it with its inputs and checks its offsets
    (mc_index_matches_input), a directory others can write is not a place to take it from)."""
    global _index_cache_set
    if _index_cache_set:
        return
    _index_cache_set = True
    v = os.environ.get("MC_INDEX_CACHE")
    if v == "0":
        return
    d = _private_dir(v) if v else user_cache_dir()      # (a directory named in the environment passes the same test: this user's, not group / world writable)
    if d:
        load_library().mc_set_index_cache(d.encode())


def read_fasta_genome(path):
    """(bases, contig_off) of a .fna[.gz]: every record's sequence, line breaks dropped, case kept, one after another."""
    opener = gzip.open if path.endswith(".gz") else open
    parts, off = [], [0]
    cur = None
    with opener(path, "rb") as f:
        for line in f:
            if line.startswith(b">"):
                if cur is not None:
                    parts.append(b"".join(cur)); off.append(off[-1] + len(parts[-1]))
                cur = []
            elif cur is not None:
                cur.append(line.strip())
    if cur is not None:
        parts.append(b"".join(cur)); off.append(off[-1] + len(parts[-1]))
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.array(off, dtype=np.int64)


class _SimSource:
    """What Genome and Community share: a handle (attribute _HANDLE) on a device-resident source of reads, and the C functions
    (_SET_LIBRARY, _SIMULATE, _CLOSE) that set its library kind, simulate (n, read_len) reads of it and close it."""

    def set_library(self, error_model=None, error_rate=None, paired_end=False, insert=None):
        """The kind of library simulate() and the engine's fused pass (Engine.train_library() of a genome, Engine.community_library()
        of a community) make of this source from now on (mc_genome_set_library, mc_community_set_library): error_model None,
        'uniform' (error_rate per base) or 'illumina'; paired_end with an insert of at least the read length (rows 2k, 2k + 1 are the
        mates of fragment k).  No argument: the default, single end without errors."""
        if error_model not in ERROR_MODELS:
            raise ValueError("unknown error model %r" % (error_model,))
        lib = None
        if error_model is not None or paired_end:
            lib = C.byref(McLibrary(1 if paired_end else 0, int(insert or 0), ERROR_MODELS[error_model], float(error_rate or 0.0)))
        self._call(self._SET_LIBRARY, lib)

    def simulate(self, read_len, n, seed, library_id, first=0):
        out = np.empty((int(n), int(read_len)), dtype=np.uint8)
        self._call(self._SIMULATE, int(read_len), int(first), int(n), int(seed), int(library_id), out.ctypes.data_as(C.c_void_p))
        return out

    def _call(self, fn, *args):
        if getattr(self.lib, fn)(getattr(self, self._HANDLE), *args) != 0:
            raise RuntimeError("%s failed: %s" % (fn, self.lib.mc_last_error().decode()))

    def close(self):
        if getattr(self, self._HANDLE, None):
            getattr(self.lib, self._CLOSE)(getattr(self, self._HANDLE))
            setattr(self, self._HANDLE, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Genome(_SimSource):
    """A genome resident on one device (mc_genome_open): Genome(bases, contig_off) or Genome.from_fasta(path)."""
    _HANDLE, _SET_LIBRARY, _SIMULATE, _CLOSE = "g", "mc_genome_set_library", "mc_simulate", "mc_genome_close"

    def __init__(self, bases, contig_off, device=0):
        lib = load_library()
        self.lib = lib
        self.bases = np.ascontiguousarray(bases, dtype=np.uint8)
        self.contig_off = np.ascontiguousarray(contig_off, dtype=np.int64)
        assert self.contig_off.ndim == 1 and len(self.contig_off) >= 2 and self.contig_off[-1] == len(self.bases)
        self.device = device
        self.g = lib.mc_genome_open(self.bases.ctypes.data_as(C.c_void_p), self.contig_off.ctypes.data_as(C.c_void_p), len(self.contig_off) - 1, device)
        if not self.g:
            raise RuntimeError("mc_genome_open failed: %s" % lib.mc_last_error().decode())

    @classmethod
    def from_fasta(cls, path, device=0):
        bases, off = read_fasta_genome(path)
        return cls(bases, off, device)

    def set_read_lengths(self, reference):
        """reference=True: the libraries of this genome have seq_sim.py's read lengths, read_len + insertions - deletions
        (mc_genome_set_read_lengths MC_READLEN_REFERENCE); False: every read keeps read_len bases (the default)."""
        self.set_read_length_mode(1 if reference else 0)

    def set_read_length_mode(self, mode):
        self._call("mc_genome_set_read_lengths", int(mode))

    def simulate_varlen(self, read_len, n, seed, library_id, first=0):
        """Reads [first, first + n) in the reference read-length mode: (bases uint8, offsets int64 of n + 1)."""
        offsets = np.zeros(int(n) + 1, np.int64)
        args = (self.g, int(read_len), int(first), int(n), int(seed), int(library_id))
        total = self.lib.mc_simulate_varlen(*args, None, 0, offsets.ctypes.data_as(C.c_void_p))
        if total < 0:
            raise RuntimeError("mc_simulate_varlen failed: %s" % self.lib.mc_last_error().decode())
        bases = np.empty(max(int(total), 1), np.uint8)
        if self.lib.mc_simulate_varlen(*args, bases.ctypes.data_as(C.c_void_p), int(total), offsets.ctypes.data_as(C.c_void_p)) != total:
            raise RuntimeError("mc_simulate_varlen failed: %s" % self.lib.mc_last_error().decode())
        return bases[:int(total)], offsets


class Community(_SimSource):
    """A mock community resident on one device (mc_community_open): members = [(bases, contig_off)] of the member genomes, copies = the
    number of cells of each.  Its libraries draw a read from member m with probability proportional to copies[m] x (valid starts of
    m); csrc/mc_simlib.h states the draw."""
    _HANDLE, _SET_LIBRARY, _SIMULATE, _CLOSE = "c", "mc_community_set_library", "mc_community_simulate", "mc_community_close"

    def __init__(self, members, copies, device=0):
        lib = load_library()
        self.lib = lib
        if len(members) < 1 or len(members) != len(copies):
            raise ValueError("a community needs members and as many copies")
        offs, first, at, nc = [np.zeros(1, np.int64)], [0], 0, 0
        for bases, off in members:
            off = np.asarray(off, dtype=np.int64)
            assert off.ndim == 1 and len(off) >= 2 and off[0] == 0 and off[-1] == len(bases)
            offs.append(off[1:] + at)
            at += int(off[-1])
            nc += len(off) - 1
            first.append(nc)
        self.bases = np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.uint8) for b, _ in members]))
        self.contig_off = np.ascontiguousarray(np.concatenate(offs))
        self.member_first = np.array(first, dtype=np.int32)
        self.copies = np.array([int(k) for k in copies], dtype=np.int64)
        self.sizes = [int(len(b)) for b, _ in members]
        self.device, self.M = device, len(members)
        self.c = lib.mc_community_open(self.bases.ctypes.data_as(C.c_void_p), self.contig_off.ctypes.data_as(C.c_void_p), nc, self.member_first.ctypes.data_as(C.c_void_p),
                                       self.copies.ctypes.data_as(C.c_void_p), self.M, device)
        if not self.c:
            raise RuntimeError("mc_community_open failed: %s" % lib.mc_last_error().decode())

    def member_reads(self):
        """int64 (M,): the reads of the last simulate() / Engine.community_library() by the member they came from."""
        out = np.zeros(self.M, np.int64)
        self._call("mc_community_member_reads", out.ctypes.data_as(C.c_void_p))
        return out


def _grid_pids(max_pids):
    """The grid's max_pids as the C ints the ABI takes.  A non-integral value is refused: the reference's pid_filter compares the
    printed identity with the float, and the kernel's integer test would not be that comparison."""
    out = []
    for p in max_pids:
        f = float(p)
        if not math.isfinite(f) or f != int(f):
            raise ValueError("max_pids must be integers (%r given)" % (p,))
        out.append(int(f))
    return out


class Engine:
    """One MI355X: marker index resident in HBM + the search/classify pipeline."""

    def __init__(self, device=0, names=None, seqs=None, marker_family=None, nfam=None, stats=None):
        """stats: (residues, sequences) of the database the alignment statistics are those of, when (names, seqs) are its segments
        (mc_open_stats; abundance.split_genes); None: the database's own."""
        lib = load_library()
        use_index_cache()
        if names is None:
            names, seqs = load_markers()
            model = load_model()
            marker_family, nfam = model["marker_family"], len(model["families"])
        self.lib, self.names, self.nfam = lib, names, nfam
        n = len(names)
        an = (C.c_char_p * n)(*[s.encode() for s in names])
        asq = (C.c_char_p * n)(*[s.encode() for s in seqs])
        fam = (C.c_int32 * n)(*marker_family)
        self.h = lib.mc_open(an, asq, n, fam, nfam, device) if stats is None else lib.mc_open_stats(an, asq, n, fam, nfam, device, int(stats[0]), int(stats[1]))
        if not self.h:
            raise RuntimeError("%s failed: %s" % ("mc_open" if stats is None else "mc_open_stats", lib.mc_last_error().decode()))
        self.read_len = None

    @classmethod
    def from_rapdb(cls, rapdb_path, device=0, family_of=None, families=None):
        """Engine on a database written by prerapsearch (e.g. the reference's data/rapdb_2.15).  family_of: marker name ->
        family name (gene_fam.map); default: the packaged model's."""
        lib = load_library()
        self = cls.__new__(cls)
        self.lib = lib
        self.h = lib.mc_open_rapdb(rapdb_path.encode(), device)
        if not self.h:
            raise RuntimeError("mc_open_rapdb failed: %s" % lib.mc_last_error().decode())
        n = lib.mc_marker_count(self.h)
        self.names = [lib.mc_marker_name(self.h, i).decode() for i in range(n)]
        if family_of is None:
            model = load_model()
            pk_names, _ = load_markers()
            families = model["families"]
            fam_idx = dict(zip(pk_names, model["marker_family"]))
            fam = [fam_idx.get(nm, 0) for nm in self.names]       # (a database of other sequences: one family; searching needs none)
        else:
            fam = [families.index(family_of[nm]) for nm in self.names]
        self.nfam = len(families)
        self._check(lib.mc_set_families(self.h, (C.c_int32 * n)(*fam), self.nfam), "mc_set_families")
        self.read_len = None
        return self

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.lib.mc_last_error().decode()))

    def close(self):
        if getattr(self, "h", None):
            self.lib.mc_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_run(self, read_len, pars=None, families=None, loge_thr=1.0):
        """pars: {family: [min_cov, max_aaid, min_score, aln_stat]} as find_opt_pars returns for this length."""
        nf = self.nfam
        cov = (C.c_double * nf)(*([0.0] * nf)); score = (C.c_double * nf)(*([0.0] * nf))
        aaid = (C.c_int32 * nf)(*([100] * nf)); stat = (C.c_int32 * nf)(*([0] * nf))
        if pars is not None:
            for i, fam in enumerate(families):
                p = pars[fam]
                cov[i], aaid[i], score[i], stat[i] = float(p[0]), int(round(float(p[1]))), float(p[2]), ALN_STAT[p[3]]
                assert float(p[1]) == aaid[i]
        self._check(self.lib.mc_set_run(self.h, read_len, loge_thr, cov, score, aaid, stat), "mc_set_run")
        self.read_len = read_len

    def set_run_classes(self, class_len, pars_by_len=None, families=None, loge_thr=1.0):
        """Length classes (mc_set_run_classes): class_len ascending; pars_by_len[L] = find_opt_pars(pars.map, L) per class length."""
        nf, K = self.nfam, len(class_len)
        cov = (C.c_double * (nf * K))(*([0.0] * (nf * K))); score = (C.c_double * (nf * K))(*([0.0] * (nf * K)))
        aaid = (C.c_int32 * (nf * K))(*([100] * (nf * K))); stat = (C.c_int32 * (nf * K))(*([0] * (nf * K)))
        if pars_by_len is not None:
            for k, L in enumerate(class_len):
                for i, fam in enumerate(families):
                    p = pars_by_len[L][fam]
                    j = k * nf + i
                    cov[j], aaid[j], score[j], stat[j] = float(p[0]), int(round(float(p[1]))), float(p[2]), ALN_STAT[p[3]]
                    assert float(p[1]) == aaid[j]
        cl = (C.c_int32 * max(K, 1))(*[int(x) for x in class_len])
        self._check(self.lib.mc_set_run_classes(self.h, cl, K, loge_thr, cov, score, aaid, stat), "mc_set_run_classes")
        self.class_len = [int(x) for x in class_len]
        self.read_len = self.class_len[-1]

    @contextlib.contextmanager
    def _rows_kept(self, keep_rows):
        """keep_rows=False: the m8 rows of the searches inside stay on the device (mc_set_keep_rows), as under search_files"""
        if not keep_rows:
            self._check(self.lib.mc_set_keep_rows(self.h, 0), "mc_set_keep_rows")
        try:
            yield
        finally:
            if not keep_rows:
                self.lib.mc_set_keep_rows(self.h, 1)

    def search_classes(self, rows, first_read_id=0, keep_rows=True):
        """rows: uint8 array (n, class_len[-1]), a read's bases then 0 bytes (mc_search_classes).  Returns (best_hits, classes, class_reads):
        the best hits in ascending read id, the class index of each, and the rows per class (last entry: rows below the lowest class);
        with keep_rows=False nothing - the counters that were switched on are what the search is for."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        assert rows.ndim == 2
        with self._rows_kept(keep_rows):
            self._check(self.lib.mc_search_classes(self.h, rows.ctypes.data_as(C.c_void_p), rows.shape[0], rows.shape[1], first_read_id), "mc_search_classes")
        return self.class_results() if keep_rows else None

    def class_results(self):
        best = self.best_hits()
        pc = C.POINTER(C.c_uint8)()
        m = self.lib.mc_result_best_classes(self.h, C.byref(pc))
        if m < 0:
            raise RuntimeError("mc_result_best_classes failed: %s" % self.lib.mc_last_error().decode())
        cls = np.ctypeslib.as_array(pc, shape=(m,)).copy() if m else np.zeros(0, np.uint8)
        out = (C.c_int64 * (len(self.class_len) + 1))()
        self._check(self.lib.mc_result_class_reads(self.h, out), "mc_result_class_reads")
        return best, cls, np.array(list(out), np.int64)

    def classes_prologue(self, rows, want_sorted=True):
        """Test and timing aid (mc_debug_classes_prologue): perm, start, word0, the sorted bytes (or None) and the two kernel times."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        n, K = rows.shape[0], len(self.class_len)
        perm = np.zeros(n, np.uint32); start = np.zeros(K + 2, np.uint32); word0 = np.zeros(K + 1, np.int64)
        cap = n * rows.shape[1] + 16 * K + 16
        srt = np.zeros(cap if want_sorted else 0, np.uint8)
        ms = (C.c_float * 2)()
        nb = self.lib.mc_debug_classes_prologue(self.h, rows.ctypes.data_as(C.c_void_p), n, rows.shape[1], perm.ctypes.data_as(C.c_void_p), start.ctypes.data_as(C.c_void_p),
                                                word0.ctypes.data_as(C.c_void_p), srt.ctypes.data_as(C.c_void_p) if want_sorted else None, len(srt), ms)
        if nb < 0:
            raise RuntimeError("mc_debug_classes_prologue failed: %s" % self.lib.mc_last_error().decode())
        return perm, start, word0, (srt[:nb] if want_sorted else None), (ms[0], ms[1])

    def search(self, reads, first_read_id=0, keep_rows=True):
        """reads: uint8 array (n, read_len) of bases.  Returns (rows, best_hits) as numpy structured arrays; with keep_rows=False nothing."""
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        assert reads.ndim == 2 and reads.shape[1] == self.read_len
        with self._rows_kept(keep_rows):
            self._check(self.lib.mc_search(self.h, reads.ctypes.data_as(C.c_void_p), reads.shape[0], first_read_id), "mc_search")
        return self.results() if keep_rows else None

    def search_varlen(self, reads, first_read_id=0):
        """reads of mixed lengths (mc_search_varlen): a list of bytes / str, or (bases uint8 array, offsets int64 array of n + 1).
        Each read is searched at its own length; best hits are classified at set_run()'s length.  Returns (rows, best_hits)."""
        if isinstance(reads, tuple):
            bases, offsets = reads
            bases = np.ascontiguousarray(bases, dtype=np.uint8)
            offsets = np.ascontiguousarray(offsets, dtype=np.int64)
            if bases.ndim != 1 or offsets.ndim != 1 or len(offsets) < 1:
                raise ValueError("search_varlen: bases and offsets must be 1-D, offsets of n + 1 values")
            if len(offsets) > 1 and (offsets[0] < 0 or offsets[-1] > len(bases) or (np.diff(offsets) < 0).any()):
                raise ValueError("search_varlen: offsets must ascend from >= 0 to at most len(bases)")
        else:
            seqs = [s.encode("latin-1") if isinstance(s, str) else bytes(s) for s in reads]
            bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
            offsets = np.zeros(len(seqs) + 1, np.int64)
            np.cumsum([len(s) for s in seqs], out=offsets[1:])
        self._check(self.lib.mc_search_varlen(self.h, bases.ctypes.data_as(C.c_void_p), offsets.ctypes.data_as(C.c_void_p), len(offsets) - 1, first_read_id),
                    "mc_search_varlen")
        return self.results()

    def set_best_hits_only(self, on):
        """Only the reads that can be classified are ranked (mc_set_best_hits_only): same best hits, no rows."""
        self._check(self.lib.mc_set_best_hits_only(self.h, 1 if on else 0), "mc_set_best_hits_only")

    def search_files(self, reader, first_read_id=0, keep_rows=True, best_only=False):
        """process_seqfile + search_seqs + classify_reads in one call (mc_search_files): the reader samples beside the search."""
        self._check(self.lib.mc_set_keep_rows(self.h, 1 if keep_rows else 0), "mc_set_keep_rows")
        self.set_best_hits_only(best_only)
        try:
            rc = self.lib.mc_search_files(self.h, reader.r, first_read_id)
            if rc == -3:
                raise ReferenceError_(self.lib.mc_last_error().decode())
            self._check(rc, "mc_search_files")
        finally:
            self.lib.mc_set_keep_rows(self.h, 1)
            self.lib.mc_set_best_hits_only(self.h, 0)
        return self.results()

    def set_abundance(self, on=True, min_ident=0, min_aln=0, min_bits=0.0, max_loge=1.0):
        """Per-gene read counts for RPKG (mc_set_abundance; csrc/k_abundance.h states the rule): from now on every read that is searched
        adds its best row - among those with identity >= min_ident percent (an integer), alignment length >= min_aln, bit score >=
        min_bits and log10 E <= max_loge - to the counters of that row's subject.  on=True zeroes the counters; on=False frees them.
        With search_files(keep_rows=False) no m8 row reaches the host."""
        if on and (isinstance(min_ident, float) and min_ident != int(min_ident)):
            raise ValueError("min_ident must be an integer percent (%r given)" % (min_ident,))
        self._check(self.lib.mc_set_abundance(self.h, 1 if on else 0, int(min_ident), int(min_aln), float(min_bits), float(max_loge)), "mc_set_abundance")

    def abundance_reset(self):
        """Zeroes the abundance counters and abundance_ms() (mc_abundance_reset)."""
        self._check(self.lib.mc_abundance_reset(self.h), "mc_abundance_reset")

    def abundance_count(self):
        """The sequences every abundance table is sized by (mc_abundance_count): the database's, or the genes' under set_gene_fold."""
        return int(self.lib.mc_abundance_count(self.h))

    def set_gene_fold(self, seg_gene=None, seg_off=None, gene_len=None):
        """The fold of long genes (mc_set_gene_fold; csrc/mc_fold.h states the rule): the engine was opened on SEGMENTS - seg_gene[s] and
        seg_off[s] are the gene and the offset in it of database sequence s, gene_len[g] the residues of gene g (abundance.split_genes
        makes all three) - and from now on every row of a range is folded onto its gene before the abundance kernels see it: counts,
        coverage, ties, curve, gene bootstrap and classes are the genes', and every array they return has one entry per GENE.  Rows
        that reach the host (search, keep_rows) stay the engine's.  None turns it off.  Refused, naming the value: a map that does
        not ascend gene by gene, offsets or lengths that do not fit the segments, a range in flight, abundance counting on with
        tables of another size (set it before set_abundance)."""
        if seg_gene is None:
            self._check(self.lib.mc_set_gene_fold(self.h, 0, None, None, None), "mc_set_gene_fold")
            return
        sg, so, gl = (np.ascontiguousarray(x, dtype=np.int32) for x in (seg_gene, seg_off, gene_len))
        if sg.shape != (len(self.names),) or so.shape != sg.shape:
            raise ValueError("seg_gene and seg_off hold %d and %d values, the database %d sequences" % (sg.size, so.size, len(self.names)))
        self._check(self.lib.mc_set_gene_fold(self.h, int(gl.size), sg.ctypes.data_as(C.c_void_p), so.ctypes.data_as(C.c_void_p), gl.ctypes.data_as(C.c_void_p)), "mc_set_gene_fold")

    def gene_fold_stats(self):
        """{"ngenes": the genes of the fold (0: off), "edge_rows": the rows that touched an interior segment edge since the last reset -
        the witness that the overlap was wide enough -, "ms": k_fold's milliseconds since then (HIP events)} (mc_gene_fold_stats)."""
        ng, edge, ms = C.c_int32(0), C.c_int64(0), C.c_float(0)
        self._check(self.lib.mc_gene_fold_stats(self.h, C.byref(ng), C.byref(edge), C.byref(ms)), "mc_gene_fold_stats")
        return {"ngenes": int(ng.value), "edge_rows": int(edge.value), "ms": float(ms.value)}

    def abundance(self):
        """The counters as they stand (mc_abundance_read): {"reads": int64[nseq], "aligned": int64[nseq], "searched": int, "assigned": int}."""
        n = self.abundance_count()
        reads = np.zeros(n, np.int64); aligned = np.zeros(n, np.int64)
        searched, assigned = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.mc_abundance_read(self.h, reads.ctypes.data_as(C.c_void_p), aligned.ctypes.data_as(C.c_void_p), C.byref(searched), C.byref(assigned)),
                    "mc_abundance_read")
        return {"reads": reads, "aligned": aligned, "searched": int(searched.value), "assigned": int(assigned.value)}

    def abundance_ms(self):
        """milliseconds the abundance kernels took since the last reset (HIP events)"""
        return float(self.lib.mc_abundance_ms(self.h))

    def set_coverage(self, on=True):
        """Coverage breadth and depth of the genes beside the counts (mc_set_coverage; csrc/k_coverage.h states the rule): from now on
        a read's best row - the one set_abundance counts - adds 1 to the depth of the subject residues sstart .. send (0-based, inclusive).
        on=True zeroes the depth AND the abundance counters; on=False frees it.  Refused while set_abundance is off."""
        self._check(self.lib.mc_set_coverage(self.h, 1 if on else 0), "mc_set_coverage")

    def coverage(self):
        """The per-gene figures as they stand (mc_coverage_read): {"covered", "spanned", "max_depth"}, int64[nseq] each."""
        n = self.abundance_count()
        out = {k: np.zeros(n, np.int64) for k in ("covered", "spanned", "max_depth")}
        self._check(self.lib.mc_coverage_read(self.h, *(out[k].ctypes.data_as(C.c_void_p) for k in ("covered", "spanned", "max_depth"))), "mc_coverage_read")
        return out

    def coverage_depth(self):
        """The depth of every residue (mc_coverage_depth): one uint32 array, the genes one after the other in FASTA order - the caller
        splits it by the genes' lengths."""
        depth = np.zeros(int(self.lib.mc_abundance_residues(self.h)), np.uint32)
        self._check(self.lib.mc_coverage_depth(self.h, depth.ctypes.data_as(C.c_void_p), depth.size), "mc_coverage_depth")
        return depth

    def coverage_ms(self):
        """milliseconds the coverage scan kernels took since the last reset (HIP events); the marks are part of abundance_ms()"""
        return float(self.lib.mc_coverage_ms(self.h))

    def depth_stats(self, keep=80, any=False):
        """Order statistics of every gene's depth as it stands (mc_depth_stats; csrc/mc_depthstats.h states the rule; one selection kernel, no
        residue's depth leaves the device): {"median", "trimmed_sum", "low", "high"}, int64[nseq] each, and "keep" - with the depths sorted to x,
        cut = len x (100 - keep) // 200, lo = cut, hi = len - cut: median = x[(len - 1) // 2], low = x[lo], high = x[hi - 1], trimmed_sum = the sum
        of x[lo .. hi - 1].  any: of the any-depth of set_ties.  Refused: keep outside 1 .. 100, coverage off, any without ties."""
        n = self.abundance_count()
        out = {k: np.zeros(n, np.int64) for k in ("median", "trimmed_sum", "low", "high")}
        self._check(self.lib.mc_depth_stats(self.h, int(keep), 1 if any else 0, *(out[k].ctypes.data_as(C.c_void_p) for k in ("median", "trimmed_sum", "low", "high"))), "mc_depth_stats")
        out["keep"] = int(keep)
        return out

    def depth_stats_ms(self):
        """milliseconds the selection kernels of depth_stats() took since the last reset (HIP events)"""
        return float(self.lib.mc_depth_stats_ms(self.h))

    def set_identity(self, on=True):
        """The alignment identity of the assigned reads beside the counts (mc_set_identity; csrc/mc_identity.h states the rule): from now on
        a read's best row - the one set_abundance counts - adds 1 to its gene's bin floor(100 x nmatch / alnlen) and its nmatch, mismatch and
        gapopen to the gene's three sums.  on=True zeroes them AND every other abundance counter; on=False frees them.  Refused while
        set_abundance is off."""
        self._check(self.lib.mc_set_identity(self.h, 1 if on else 0), "mc_set_identity")

    def identity(self, levels=()):
        """The per-gene figures as they stand (mc_identity_read; one scan kernel, the histogram stays on the device): {"matched", "mismatched",
        "gap_opens": int64[nseq]; "ident_min", "ident_median", "ident_max": int32[nseq], -1 for a gene without reads (the median is the lower
        one); "levels": the levels as given; "ge": int64[nseq, len(levels)], the reads in bins >= each level}.  levels: up to 8 integers in
        0 .. 100, strictly ascending - anything else is refused."""
        n = self.abundance_count()
        lv = np.ascontiguousarray(list(levels), dtype=np.int32)
        out = {k: np.zeros(n, np.int64) for k in ("matched", "mismatched", "gap_opens")}
        out.update({k: np.zeros(n, np.int32) for k in ("ident_min", "ident_median", "ident_max")})
        ge = np.zeros((n, lv.size), np.int64)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
        self._check(self.lib.mc_identity_read(self.h, ptr(lv), int(lv.size), *(out[k].ctypes.data_as(C.c_void_p) for k in ("matched", "mismatched", "gap_opens", "ident_min", "ident_median", "ident_max")),
                                              ptr(ge)), "mc_identity_read")
        out.update({"levels": [int(x) for x in lv], "ge": ge})
        return out

    def identity_hist(self):
        """The histogram itself (mc_identity_hist): uint32[nseq, 101], the reads of every gene by the floor of their best row's identity."""
        hist = np.zeros((self.abundance_count(), 101), np.uint32)
        self._check(self.lib.mc_identity_hist(self.h, hist.ctypes.data_as(C.c_void_p)), "mc_identity_hist")
        return hist

    def identity_ms(self):
        """milliseconds k_identity took over the completed ranges since the last reset (HIP events); identity_scan_ms(): the scans of identity()"""
        return float(self.lib.mc_identity_ms(self.h))

    def identity_scan_ms(self):
        return float(self.lib.mc_identity_scan_ms(self.h))

    def set_ties(self, on=True, group_of=None, ngroups=0):
        """The tie accounting beside the counts (mc_set_ties; csrc/k_ties.h states the rule): from now on every read that set_abundance
        counts also adds to candidates, unique and share of the DISTINCT subjects that tie for its highest bit score.  group_of: one
        group number in 0 .. ngroups - 1 per subject, or None.  on=True zeroes the tie counters AND the abundance counters and depth;
        on=False frees them.  Refused while set_abundance is off."""
        if on and group_of is not None:
            g = np.ascontiguousarray(group_of, dtype=np.int32)
            if g.shape != (self.abundance_count(),):
                raise ValueError("group_of holds %d values, the database %d sequences" % (g.size, self.abundance_count()))
            rc = self.lib.mc_set_ties(self.h, 1, g.ctypes.data_as(C.c_void_p), int(ngroups))
        else:
            rc = self.lib.mc_set_ties(self.h, 1 if on else 0, None, int(ngroups) if on else 0)
        self._check(rc, "mc_set_ties")
        self._ties_ngroups = int(ngroups) if on else 0

    def ties(self):
        """The tie counters as they stand (mc_ties_read): {"candidates", "unique": int64[nseq], "share": uint64[nseq] in units of 2^-32,
        "group_unique": int64[ngroups], "ambiguous", "group_ambiguous": int}."""
        n = self.abundance_count()
        out = {"candidates": np.zeros(n, np.int64), "unique": np.zeros(n, np.int64), "share": np.zeros(n, np.uint64),
               "group_unique": np.zeros(getattr(self, "_ties_ngroups", 0), np.int64)}
        amb, gamb = C.c_int64(0), C.c_int64(0)
        self._check(self.lib.mc_ties_read(self.h, *(out[k].ctypes.data_as(C.c_void_p) for k in ("candidates", "unique", "share", "group_unique")), C.byref(amb), C.byref(gamb)),
                    "mc_ties_read")
        out["ambiguous"], out["group_ambiguous"] = int(amb.value), int(gamb.value)
        return out

    def ties_coverage(self):
        """The per-gene figures of the any-depth (mc_ties_coverage_read): {"covered_any", "spanned_any", "max_depth_any"}, int64[nseq] each."""
        n = self.abundance_count()
        out = {k: np.zeros(n, np.int64) for k in ("covered_any", "spanned_any", "max_depth_any")}
        self._check(self.lib.mc_ties_coverage_read(self.h, *(out[k].ctypes.data_as(C.c_void_p) for k in ("covered_any", "spanned_any", "max_depth_any"))), "mc_ties_coverage_read")
        return out

    def set_curve(self, points):
        """A rarefaction curve beside the counts (mc_set_curve; csrc/k_curve.h states the rule): points - ascending read counts n_k, each
        >= 1, at most 64, repeats allowed - or None / an empty list to turn it off.  From now on every read that set_abundance assigns is
        also counted by the prefix of the sample it belongs to (its global id: first_read_id plus its index).  Turning it on zeroes the
        curve AND the abundance counters, depth and ties.  Refused while set_abundance is off; search_varlen is refused while it is on."""
        pts = [] if points is None else [int(x) for x in points]
        arr = np.array(pts, dtype=np.int64)
        self._check(self.lib.mc_set_curve(self.h, len(pts), arr.ctypes.data_as(C.c_void_p) if len(pts) else None), "mc_set_curve")

    def curve(self, covered=True):
        """The curve as it stands (mc_curve_read): {"reads", "aligned": int64[K, nseq], "covered": int64[K, nseq] (with covered=True:
        coverage must be on), "assigned": int64[K], "beyond": int} - row k is what abundance() and coverage()["covered"] return after
        a run on the first n_k reads alone; beyond counts the assigned reads behind the last point."""
        K, n = int(self.lib.mc_curve_k(self.h)), self.abundance_count()                  # (the library's K sizes the arrays, however the curve was set)
        out = {k: np.zeros((K, n), np.int64) for k in (("reads", "aligned", "covered") if covered else ("reads", "aligned"))}
        out["assigned"] = np.zeros(K, np.int64)
        beyond = C.c_int64(0)
        self._check(self.lib.mc_curve_read(self.h, out["reads"].ctypes.data_as(C.c_void_p), out["aligned"].ctypes.data_as(C.c_void_p),
                                           out["covered"].ctypes.data_as(C.c_void_p) if covered else None, out["assigned"].ctypes.data_as(C.c_void_p), C.byref(beyond)), "mc_curve_read")
        out["beyond"] = int(beyond.value)
        return out

    def curve_ms(self):
        """milliseconds the curve's kernels took since the last reset (HIP events): k_curve per range and one scan per curve()"""
        return float(self.lib.mc_curve_ms(self.h))

    def set_gene_bootstrap(self, capacity):
        """The bootstrap of the counts (mc_set_gene_bootstrap; csrc/mc_geneboot.h states the rule): from now on every read that
        set_abundance assigns is also kept as (global id, gene) in a device list of `capacity` entries - the most reads that may be
        assigned before gene_bootstrap() is called; 0 or None turns it off.  Turning it on zeroes the list AND the abundance counters,
        depth, ties and curve.  Refused while set_abundance is off; search_varlen is refused while it is on."""
        self._check(self.lib.mc_set_gene_bootstrap(self.h, int(capacity or 0)), "mc_set_gene_bootstrap")
        self.gene_bootstrap_capacity = int(capacity or 0)          # (what the tie list is sized by: abundance.tie_list_capacity)

    def gene_bootstrap(self, B, seed, scale, counts=False):
        """B Poisson-bootstrap replicates of the counts as they stand (mc_gene_bootstrap), under bootstrap()'s weights: {"stats":
        float64[nseq, 6] - sum, m2, x[lo], x[lo + 1], x[hi], x[hi + 1] of the used values (double)c[b][s] * scale[b] -, "used": m,
        "dropped": 0} and with counts=True "counts": int64[nseq, B].  scale: B doubles; replicate b is used when scale[b] is finite and
        > 0.  Raises when a read did not fit the list (the message names how many)."""
        B, n = int(B), self.abundance_count()
        sc = np.ascontiguousarray(scale, dtype=np.float64)
        if sc.shape != (max(B, 0),):
            raise ValueError("scale holds %d values, B is %d" % (sc.size, B))
        out = {"stats": np.zeros((n, 6), np.float64), "used": int((np.isfinite(sc) & (sc > 0)).sum())}
        if counts:
            out["counts"] = np.zeros((n, max(B, 0)), np.int64)
        dropped = C.c_int64(0)
        self._check(self.lib.mc_gene_bootstrap(self.h, B, int(seed) & 0xFFFFFFFFFFFFFFFF, sc.ctypes.data_as(C.c_void_p), out["counts"].ctypes.data_as(C.c_void_p) if counts else None,
                                               out["stats"].ctypes.data_as(C.c_void_p), C.byref(dropped)), "mc_gene_bootstrap")
        out["dropped"] = int(dropped.value)
        return out

    def group_bootstrap(self, B, seed, scale, group_of, ngroups, gene_kb, counts=False):
        """The same B replicates summed over groups of genes (mc_group_bootstrap; csrc/mc_groupboot.h states the rule): group_of: every
        gene's group in 0 .. ngroups - 1, gene_kb: every gene's length in kb, finite and > 0.  {"stats": float64[ngroups, 6] - sum, m2
        and the four order statistics of the group's used replicate values, the sum over its members in ascending gene index of
        (double)c[b][s] * scale[b] / gene_kb[s] -, "used": m, "dropped": 0} and with counts=True "counts": int64[ngroups, B], the
        members' replicate counts added.  The genes' replicate counts never leave the device.  Raises as gene_bootstrap does, and on a
        map or a gene_kb the library refuses (the message names the value)."""
        B, n, ngroups = int(B), self.abundance_count(), int(ngroups)
        sc = np.ascontiguousarray(scale, dtype=np.float64)
        if sc.shape != (max(B, 0),):
            raise ValueError("scale holds %d values, B is %d" % (sc.size, B))
        gof, kb = np.ascontiguousarray(group_of, dtype=np.int32), np.ascontiguousarray(gene_kb, dtype=np.float64)
        if gof.shape != (n,) or kb.shape != (n,):
            raise ValueError("group_of holds %d values and gene_kb %d, the genes are %d" % (gof.size, kb.size, n))
        out = {"stats": np.zeros((max(ngroups, 0), 6), np.float64), "used": int((np.isfinite(sc) & (sc > 0)).sum())}
        if counts:
            out["counts"] = np.zeros((max(ngroups, 0), max(B, 0)), np.int64)
        dropped = C.c_int64(0)
        self._check(self.lib.mc_group_bootstrap(self.h, B, int(seed) & 0xFFFFFFFFFFFFFFFF, sc.ctypes.data_as(C.c_void_p), gof.ctypes.data_as(C.c_void_p), ngroups,
                                                kb.ctypes.data_as(C.c_void_p), out["counts"].ctypes.data_as(C.c_void_p) if counts else None,
                                                out["stats"].ctypes.data_as(C.c_void_p), C.byref(dropped)), "mc_group_bootstrap")
        out["dropped"] = int(dropped.value)
        return out

    def group_bootstrap_ms(self):
        """milliseconds the kernels of the group_bootstrap() calls took since the last reset (HIP events): two per call, and three more
        where the call had to make the genes' replicate counts"""
        return float(self.lib.mc_group_bootstrap_ms(self.h))

    def group_bootstrap_kernels_ms(self):
        """of group_bootstrap_ms(), the share of each of the two kernels: {"values", "summary"}"""
        v, s = C.c_float(0), C.c_float(0)
        self.lib.mc_group_bootstrap_kernels_ms(self.h, C.byref(v), C.byref(s))
        return {"values": float(v.value), "summary": float(s.value)}

    def set_tie_bootstrap(self, capacity):
        """The bootstrap of the tie shares (mc_set_tie_bootstrap; csrc/mc_tieboot.h states the rule): from now on every read that set_ties
        counts is also kept as one (global id, gene, share) per gene of its tied set in a device list of `capacity` entries, at most 2^27 -
        the most entries (the sum of ties()["candidates"]) there may be before tie_bootstrap() is called; 0 or None turns it off.  Turning
        it on zeroes the list AND every abundance counter.  Refused while set_ties or set_gene_bootstrap is off - and either of them, set
        again or turned off, turns it off: call it behind them.  search_varlen is refused while it is on."""
        self._check(self.lib.mc_set_tie_bootstrap(self.h, int(capacity or 0)), "mc_set_tie_bootstrap")

    def tie_bootstrap(self, B, seed, scale, shares=False):
        """gene_bootstrap() on the tie shares as they stand (mc_tie_bootstrap): the same replicates, {"stats": float64[nseq, 6] - sum, m2,
        x[lo], x[lo + 1], x[hi], x[hi + 1] of the used values (double)cs[b][s] * (scale[b] * 2^-32) -, "used": m, "dropped": 0} and with
        shares=True "shares": uint64[nseq, B] in units of 2^-32.  Replicate b is used when scale[b] * 2^-32 is finite and > 0.  Raises when
        an entry did not fit the list (the message names how many)."""
        B, n = int(B), self.abundance_count()
        sc = np.ascontiguousarray(scale, dtype=np.float64)
        if sc.shape != (max(B, 0),):
            raise ValueError("scale holds %d values, B is %d" % (sc.size, B))
        s32 = sc * 2.0 ** -32
        out = {"stats": np.zeros((n, 6), np.float64), "used": int((np.isfinite(s32) & (s32 > 0)).sum())}
        if shares:
            out["shares"] = np.zeros((n, max(B, 0)), np.uint64)
        dropped = C.c_int64(0)
        self._check(self.lib.mc_tie_bootstrap(self.h, B, int(seed) & 0xFFFFFFFFFFFFFFFF, sc.ctypes.data_as(C.c_void_p), out["shares"].ctypes.data_as(C.c_void_p) if shares else None,
                                              out["stats"].ctypes.data_as(C.c_void_p), C.byref(dropped)), "mc_tie_bootstrap")
        out["dropped"] = int(dropped.value)
        return out

    def tie_bootstrap_ms(self):
        """milliseconds the tie bootstrap's kernels took since the last reset (HIP events): one kernel per range, three per tie_bootstrap()"""
        return float(self.lib.mc_tie_bootstrap_ms(self.h))

    def tie_bootstrap_kernels_ms(self):
        """of tie_bootstrap_ms(), the share of k_tieboot_collect and of the reads' kernels: {"collect", "read"}"""
        c, r = C.c_float(0), C.c_float(0)
        self.lib.mc_tie_bootstrap_kernels_ms(self.h, C.byref(c), C.byref(r))
        return {"collect": float(c.value), "read": float(r.value)}

    def set_coverage_bootstrap(self, capacity):
        """The bootstrap of the coverage columns (mc_set_coverage_bootstrap; csrc/mc_covboot.h states the rule): from now on every read that
        set_abundance assigns is also kept as (global id, gene, sstart, send) in a device list of `capacity` entries - the most reads there may
        be assigned before coverage_bootstrap() is called; 0 or None turns it off.  Turning it on zeroes the list AND every abundance counter.
        Refused while set_abundance or set_coverage is off - and either of them turned off turns it off: call it behind them.  It needs
        neither set_gene_bootstrap nor set_ties.  search_varlen is refused while it is on."""
        self._check(self.lib.mc_set_coverage_bootstrap(self.h, int(capacity or 0)), "mc_set_coverage_bootstrap")

    def coverage_bootstrap(self, B, seed, need=None, covered=False):
        """B Poisson-bootstrap replicates of the covered residues as they stand (mc_coverage_bootstrap), under bootstrap()'s weights: a read is
        present in replicate b when its weight is > 0.  {"stats": float64[nseq, 6] - sum, m2, x[lo], x[lo + 1], x[hi], x[hi + 1] of the B
        values covered_b, in residues -, "dropped": 0}; with need (uint32[nseq], every one >= 1) "detected": int64[nseq], the replicates with
        covered_b >= need; with covered=True "covered": int64[nseq, B].  Raises when a read did not fit the list (the message names how many)."""
        B, n = int(B), self.abundance_count()
        out = {"stats": np.zeros((n, 6), np.float64)}
        nd = None
        if need is not None:
            nd = np.ascontiguousarray(need, dtype=np.uint32)
            if nd.shape != (n,):
                raise ValueError("need holds %d values, the database %d genes" % (nd.size, n))
            out["detected"] = np.zeros(n, np.int64)
        if covered:
            out["covered"] = np.zeros((n, max(B, 0)), np.int64)
        dropped = C.c_int64(0)
        self._check(self.lib.mc_coverage_bootstrap(self.h, B, int(seed) & 0xFFFFFFFFFFFFFFFF, nd.ctypes.data_as(C.c_void_p) if nd is not None else None,
                                                   out["covered"].ctypes.data_as(C.c_void_p) if covered else None, out["stats"].ctypes.data_as(C.c_void_p),
                                                   out["detected"].ctypes.data_as(C.c_void_p) if nd is not None else None, C.byref(dropped)), "mc_coverage_bootstrap")
        out["dropped"] = int(dropped.value)
        return out

    def coverage_bootstrap_ms(self):
        """milliseconds the coverage bootstrap's kernels took since the last reset (HIP events): one kernel per range, three per coverage_bootstrap()"""
        return float(self.lib.mc_coverage_bootstrap_ms(self.h))

    def coverage_bootstrap_kernels_ms(self):
        """of coverage_bootstrap_ms(), the share of k_covboot_collect and of the reads' kernels: {"collect", "read"}"""
        c, r = C.c_float(0), C.c_float(0)
        self.lib.mc_coverage_bootstrap_kernels_ms(self.h, C.byref(c), C.byref(r))
        return {"collect": float(c.value), "read": float(r.value)}

    def set_abundance_classes(self, on=True):
        """The counts may ride on class runs (mc_set_abundance_classes; csrc/k_abund_classes.h states the rule): while it is on,
        search_classes and search_files on a class reader are no longer refused under set_abundance - every read is counted at the
        length class it reaches, coverage, ties and the gene bootstrap (global read ids) with it.  on=True zeroes every counter;
        on=False frees the per-class table.  Refused while set_abundance is off and while the curve is on."""
        self._check(self.lib.mc_set_abundance_classes(self.h, 1 if on else 0), "mc_set_abundance_classes")

    def abundance_classes(self):
        """The per-class table as it stands (mc_abundance_classes_read): {"rows", "assigned"}, int64[K + 1] each - per class of
        set_run_classes the rows sorted into it and the reads of it assigned to a gene; the last entry is the rows below the lowest class."""
        n = len(getattr(self, "class_len", [])) + 1
        out = {k: np.zeros(n, np.int64) for k in ("rows", "assigned")}
        self._check(self.lib.mc_abundance_classes_read(self.h, out["rows"].ctypes.data_as(C.c_void_p), out["assigned"].ctypes.data_as(C.c_void_p), n), "mc_abundance_classes_read")
        return out

    def abundance_classes_ms(self):
        """milliseconds the per-class table's kernel took since the last reset (HIP events): one single-thread kernel per piece"""
        return float(self.lib.mc_abundance_classes_ms(self.h))

    def gene_bootstrap_ms(self):
        """milliseconds the gene bootstrap's kernels took since the last reset (HIP events): one kernel per range, three per gene_bootstrap()"""
        return float(self.lib.mc_gene_bootstrap_ms(self.h))

    def ties_ms(self):
        """milliseconds the tie kernels took since the last reset (HIP events)"""
        return float(self.lib.mc_ties_ms(self.h))

    def upload(self, reads):
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        assert reads.ndim == 2 and reads.shape[1] == self.read_len
        self._check(self.lib.mc_upload(self.h, reads.ctypes.data_as(C.c_void_p), reads.shape[0]), "mc_upload")

    def run(self, first_read_id=0):
        self._check(self.lib.mc_run(self.h, first_read_id), "mc_run")

    def attach(self, device_ptr, nreads):
        """Adopt caller-owned device memory (nreads x read_len bytes) as the resident read set."""
        self._check(self.lib.mc_attach(self.h, C.c_void_p(device_ptr), nreads), "mc_attach")

    def set_counting(self, on):
        """Turns the seed kernel's algorithmic-traffic counters (stats bucket_lookups / key_probes) on or off."""
        self._check(self.lib.mc_set_counting(self.h, 1 if on else 0), "mc_set_counting")

    def range_begin(self, first, count, first_read_id=0):
        """Enqueues the front of the range (translation, seeds, seed evaluation) and returns at once.  range_end(), range_begin(next),
        then the results of the range that ended: the device runs the next front while the host looks at them.  One range at a time."""
        self._check(self.lib.mc_range_begin(self.h, first, count, first_read_id), "mc_range_begin")

    def range_end(self):
        """Completes the range in flight: rows() / best_hits() / stats() are its results."""
        self._check(self.lib.mc_range_end(self.h), "mc_range_end")

    def ranges_in_flight(self):
        return self.lib.mc_ranges_in_flight(self.h)

    def ranges_translated_ahead(self):
        """The ranges begun since the engine was opened whose translation had been issued ahead, in the background of the range before."""
        return int(self.lib.mc_ranges_translated_ahead(self.h))

    def ahead_kernel_ms(self):
        """The interval (ms) of the lookahead's kernel that the range which ended last used; 0 where it used none."""
        return float(self.lib.mc_ahead_kernel_ms(self.h))

    def run_range(self, first, count, first_read_id=0):
        self._check(self.lib.mc_run_range(self.h, first, count, first_read_id), "mc_run_range")

    def debug_stage(self, what):
        """Test aid: what a stage of the last run_range() left on the device (0 frames, 1 seed hits, 2 gap tasks, 3 HSP pool, 4 the
        gapped chain's three counts: gap_counts(), 5 the form of k_translate_seg that was launched: 1 staged, 0 direct, one uint32,
        6 its instantiation: 1 narrow - frames of at most 63 residues -, 0 wide, one uint32, 7 waves per workgroup x workgroups per CU
        of the last seed launch, one uint32) as a (records, record_bytes) uint8 array."""
        rec = C.c_int32(0)
        n = self.lib.mc_debug_stage(self.h, what, None, 0, C.byref(rec))
        if n < 0:
            raise RuntimeError("mc_debug_stage failed: %s" % self.lib.mc_last_error().decode())
        buf = np.zeros(n, np.uint8)
        if n and self.lib.mc_debug_stage(self.h, what, buf.ctypes.data_as(C.c_void_p), n, C.byref(rec)) != n:
            raise RuntimeError("mc_debug_stage failed: %s" % self.lib.mc_last_error().decode())
        return buf.reshape(-1, rec.value) if rec.value else buf

    def gap_counts(self):
        """Test aid: the counts of the gapped extension's chain of kernels in the last run_range() (defined when it ran unsplit:
        stats()["range_splits"] == 0) - the distinct flanks, those sent to the second window, those sent to full-size rows."""
        v = self.debug_stage(4).reshape(-1).view("<u4")
        return {"flanks": int(v[0]), "second_window": int(v[1]), "full_size": int(v[2])}

    def rows(self, copy=True):
        """m8 rows of the last run (structured array).  copy=False returns a view of the handle's buffer, valid until the next call."""
        pr = C.POINTER(McRow)()
        n = self.lib.mc_result_rows(self.h, C.byref(pr))
        if not n:
            return np.zeros(0, ROW_DTYPE)
        a = np.ctypeslib.as_array(C.cast(pr, C.POINTER(C.c_uint8)), shape=(n * C.sizeof(McRow),)).view(ROW_DTYPE)
        return a.copy() if copy else a

    def best_hits(self, copy=True):
        """best hit per classified read of the last run, ascending read id."""
        pb = C.POINTER(McBestHit)()
        m = self.lib.mc_result_best_hits(self.h, C.byref(pb))
        if not m:
            return np.zeros(0, BEST_DTYPE)
        a = np.ctypeslib.as_array(C.cast(pb, C.POINTER(C.c_uint8)), shape=(m * C.sizeof(McBestHit),)).view(BEST_DTYPE)
        return a.copy() if copy else a

    def results(self):
        return self.rows(), self.best_hits()

    def stats(self):
        s = McStats()
        self._check(self.lib.mc_result_stats(self.h, C.byref(s)), "mc_result_stats")
        return {k: getattr(s, k) for k, _ in McStats._fields_ if not k.startswith("_")}

    def write_m8(self, path, append=False):
        self._check(self.lib.mc_write_m8(self.h, path.encode(), 1 if append else 0), "mc_write_m8")

    def write_m8_named(self, path, names, append=False, first_read_id=0):
        arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
        self._check(self.lib.mc_write_m8_named(self.h, path.encode(), 1 if append else 0, arr, len(names), first_read_id), "mc_write_m8_named")

    def grid_classify(self, aln_covs, max_pids, min_scores):
        """The training grid (training/training.py:311-334) over the rows of the last search: (hits, aln, cov) arrays of shape
        (len(aln_covs), len(max_pids), len(min_scores), nfam)."""
        nc, npid, ns = len(aln_covs), len(max_pids), len(min_scores)
        shape = (nc, npid, ns, self.nfam)
        hits = np.zeros(shape, np.int64); aln = np.zeros(shape, np.int64); cov = np.zeros(shape, np.float64)
        self._check(self.lib.mc_grid_classify(self.h, (C.c_double * nc)(*aln_covs), nc, (C.c_int32 * npid)(*_grid_pids(max_pids)), npid, (C.c_double * ns)(*min_scores), ns,
                                              hits.ctypes.data_as(C.POINTER(C.c_int64)), aln.ctypes.data_as(C.POINTER(C.c_int64)), cov.ctypes.data_as(C.POINTER(C.c_double))),
                    "mc_grid_classify")
        return hits, aln, cov

    def bootstrap(self, best, stats, B, seed):
        """The per-family sums of the best hits under B Poisson-bootstrap replicates (mc_bootstrap; csrc/mc_boot.h states the weights).
        best: BEST_DTYPE array; stats: one aln_stat per family ('hits' / 'cov' / 'aln', or 0 / 1 / 2).  Returns (sums_i64 of shape
        (B, nfam + 1): hits and aln families, last column the replicate's classified reads; sums_f64 of shape (B, nfam): cov families)."""
        best = np.ascontiguousarray(best, dtype=BEST_DTYPE)
        nfam, B = len(stats), int(B)
        stat = (C.c_int32 * nfam)(*[ALN_STAT.get(s, s) for s in stats])
        si = np.zeros((max(B, 0), nfam + 1), np.int64); sf = np.zeros((max(B, 0), nfam), np.float64)
        self._check(self.lib.mc_bootstrap(self.h, best.ctypes.data_as(C.c_void_p), len(best), stat, nfam, B, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                          si.ctypes.data_as(C.POINTER(C.c_int64)), sf.ctypes.data_as(C.POINTER(C.c_double))), "mc_bootstrap")
        return si, sf

    def bootstrap_ms(self):
        """milliseconds the last bootstrap()'s kernels took (HIP events)"""
        return float(self.lib.mc_bootstrap_ms(self.h))

    def fit_weights(self, pred, truth, seed, read_len, candidates=None, generations=None):
        """The per-family weights of one read length (mc_fit_weights; csrc/mc_wfit.h states the search).  pred: (N, F) float64, NaN
        for NA; truth: (N,).  candidates / generations None: the header's defaults.  Returns (weights (F,), trace (G + 1, 3): best mue,
        winning candidate, sigma per generation, row 0 the start)."""
        pred = np.ascontiguousarray(pred, dtype=np.float64)
        truth = np.ascontiguousarray(truth, dtype=np.float64)
        if pred.ndim != 2 or truth.shape != (pred.shape[0],):
            raise ValueError("fit_weights: pred (N, F) and truth (N,)")
        Cn = 0 if candidates is None else int(candidates)
        Gn = -1 if generations is None else int(generations)
        rows = (WFIT_DEFAULT_G if Gn == -1 else max(Gn, 0)) + 1
        w = np.zeros(pred.shape[1], np.float64); trace = np.zeros((rows, 3), np.float64)
        self._check(self.lib.mc_fit_weights(self.h, pred.ctypes.data, truth.ctypes.data, pred.shape[0], pred.shape[1], int(seed) & 0xFFFFFFFFFFFFFFFF, int(read_len), Cn, Gn,
                                            w.ctypes.data, trace.ctypes.data), "mc_fit_weights")
        return w, trace

    def weights_mue(self, pred, truth, w):
        """mue of the weight vectors w (K, F) on the table (mc_weights_mue): (K,) float64"""
        pred = np.ascontiguousarray(pred, dtype=np.float64)
        truth = np.ascontiguousarray(truth, dtype=np.float64)
        w = np.ascontiguousarray(np.atleast_2d(w), dtype=np.float64)
        if pred.ndim != 2 or truth.shape != (pred.shape[0],) or w.shape[1] != pred.shape[1]:
            raise ValueError("weights_mue: pred (N, F), truth (N,) and w (K, F)")
        out = np.zeros(w.shape[0], np.float64)
        self._check(self.lib.mc_weights_mue(self.h, pred.ctypes.data, truth.ctypes.data, pred.shape[0], pred.shape[1], w.ctypes.data, w.shape[0], out.ctypes.data), "mc_weights_mue")
        return out

    def fit_weights_ms(self):
        """milliseconds the kernels of the last fit_weights() / weights_mue() took (HIP events)"""
        return float(self.lib.mc_fit_weights_ms(self.h))

    def simulate(self, genome, n, seed, library_id, first=0):
        """Reads [first, first + n) of library (seed, library_id) at this engine's read length: uint8 array (n, read_len)."""
        return genome.simulate(self.read_len, n, seed, library_id, first)

    def train_library(self, genome, nreads, seed, library_id, aln_covs, max_pids, min_scores):
        """One library pass on the device (mc_train_library): simulate, search and grid-classify nreads reads of the genome at this
        engine's read length.  (hits, aln, cov) arrays of shape (len(aln_covs), len(max_pids), len(min_scores), nfam), as
        grid_classify returns them."""
        nc, npid, ns = len(aln_covs), len(max_pids), len(min_scores)
        shape = (nc, npid, ns, self.nfam)
        hits = np.zeros(shape, np.int64); aln = np.zeros(shape, np.int64); cov = np.zeros(shape, np.float64)
        self._check(self.lib.mc_train_library(self.h, genome.g, int(nreads), int(seed), int(library_id), (C.c_double * nc)(*aln_covs), nc,
                                              (C.c_int32 * npid)(*_grid_pids(max_pids)), npid, (C.c_double * ns)(*min_scores), ns,
                                              hits.ctypes.data_as(C.POINTER(C.c_int64)), aln.ctypes.data_as(C.POINTER(C.c_int64)), cov.ctypes.data_as(C.POINTER(C.c_double))),
                    "mc_train_library")
        return hits, aln, cov

    def train_library_bases(self):
        """bases of the last train_library's reads: nreads x read_len, or their real total in the reference read-length mode"""
        return int(self.lib.mc_train_library_bases(self.h))

    def train_times(self):
        """{'simulate', 'search', 'grid'}: milliseconds of the last train_library (HIP events)."""
        ms = (C.c_float * 3)()
        self._check(self.lib.mc_train_times(self.h, ms), "mc_train_times")
        return {"simulate": ms[0], "search": ms[1], "grid": ms[2]}

    def community_library(self, community, nreads, seed, library_id):
        """One fused library pass of a community (mc_community_library): nreads reads simulated and searched on the device at this
        engine's run settings.  Returns the best hits - those of search() on the same reads; stats() holds the search's totals,
        community.member_reads() the reads per member."""
        self._check(self.lib.mc_community_library(self.h, community.c, int(nreads), int(seed), int(library_id)), "mc_community_library")
        return self.best_hits()

    def community_times(self):
        """{'simulate', 'search'}: milliseconds of the last community_library (HIP events)."""
        ms = (C.c_float * 2)()
        self._check(self.lib.mc_community_times(self.h, ms), "mc_community_times")
        return {"simulate": ms[0], "search": ms[1]}

    def index_view(self):
        p = [C.c_void_p() for _ in range(5)]
        nres, npost, thr = C.c_int64(), C.c_int64(), C.c_uint32()
        lp = (C.c_double * 10)()
        self._check(self.lib.mc_index_view(self.h, *[C.byref(x) for x in p], C.byref(nres), C.byref(npost), C.byref(thr), lp), "mc_index_view")
        nseq = len(self.names)

        def arr(ptr, dtype, n):
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n * np.dtype(dtype).itemsize,)).view(dtype).copy()
        return {"res": arr(p[0], "u1", nres.value), "off": arr(p[1], "<u4", nseq + 1), "bstart": arr(p[2], "<u4", 1000001),
                "post": arr(p[3], "<u4", npost.value), "keys": arr(p[4], "<u2", npost.value), "thr": thr.value, "letter_p": list(lp)}


def search_files_multi(engines, reader, first_read_id=0, keep_rows=False, best_only=False):
    """mc_search_files_multi: one sampler, its batches dealt to several engines (GPUs) of this process.  Returns the best hits of
    all engines in ascending read order."""
    lib = load_library()
    arr = (C.c_void_p * len(engines))(*[e.h for e in engines])
    for e in engines:
        lib.mc_set_keep_rows(e.h, 1 if keep_rows else 0)
        lib.mc_set_best_hits_only(e.h, 1 if best_only else 0)
    try:
        rc = lib.mc_search_files_multi(arr, len(engines), reader.r, first_read_id)
        if rc == -3:
            raise ReferenceError_(lib.mc_last_error().decode())
        if rc != 0:
            raise RuntimeError("mc_search_files_multi failed (%d): %s" % (rc, lib.mc_last_error().decode()))
    finally:
        for e in engines:
            lib.mc_set_keep_rows(e.h, 1)
            lib.mc_set_best_hits_only(e.h, 0)
    best = np.concatenate([e.best_hits() for e in engines])
    return best[np.argsort(best["read"], kind="stable")]
