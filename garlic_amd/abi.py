"""ctypes binding of libgarlic_hip.so (C ABI declared in include/garlic_hip.h).

This is plumbing for the tests and bench.py; the product is the shared library.  There is no
CPU fallback anywhere in this package: if the library is missing or no gfx950 device is
present, calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgarlic_hip.so")

OK, ERR_INVALID, ERR_HIP, ERR_STATE, ERR_NOMEM, ERR_RANGE = 0, 1, 2, 3, 4, 5
HOST, DEVICE = 0, 1
# GARLIC_VCF_*: what garlic_bed_set_rows_vcf answers per row
VCF_BAD_BYTE, VCF_HALF_MISSING, VCF_HAPLOID, VCF_ALLELE_INDEX, VCF_FEW_COLUMNS, VCF_MANY_COLUMNS = 1, 2, 3, 4, 5, 6
# GARLIC_TPED_*: what garlic_bed_set_rows_tped answers per row
TPED_LONG_ALLELE, TPED_BAD_BYTE, TPED_FEW_COLUMNS, TPED_MANY_COLUMNS = 1, 2, 3, 4
FEED_FROM_SCORES, FEED_CHAIN, FEED_SAMPLED_WLOD, FEED_TGLS_CHAIN = 0, 1, 2, 3   # garlic_lod_feed_info
FEED_TGLS_CHAIN_SHARED = 4   # garlic_lod_feed_multi_info: the size shared its chain launch with another size
FEED_ORDER_REFERENCE, FEED_ORDER_SORTED = 0, 1   # garlic_panel_set_feed_order
LD_PAIR_PLAIN, LD_PAIR_MFMA, LD_PAIR_LANE, LD_PAIR_TILED, LD_PAIR_FLAT = 0, 1, 2, 3, 4   # garlic_panel_ld_form_info
LD_SUM_PLAIN, LD_SUM_FLAT, LD_SUM_COL, LD_SUM_TILED = 0, 1, 2, 3
TGLS_DICTIONARY, TGLS_CONTINUOUS, TGLS_DICTIONARY16 = 1, 2, 3   # garlic_panel_tgls_mode
# GARLIC_TGLS_*: what garlic_tgls_set_rows_text answers per row; TGLS_RAW: gl_type of garlic_tgls_get_rows without conversion
TGLS_OK, TGLS_DEFERRED, TGLS_FEW_COLUMNS, TGLS_MANY_COLUMNS, TGLS_RAW = 0, 1, 2, 3, -1
TGLS_VCF_NO_KEY, TGLS_VCF_NO_VALUE = 4, 5   # garlic_tgls_set_rows_vcf's own
# GARLIC_BGZF_*: what garlic_bgzf_inflate answers per block
(BGZF_OK, BGZF_BAD_BLOCK_TYPE, BGZF_BAD_CODE_LENGTHS, BGZF_BAD_SYMBOL, BGZF_BAD_DISTANCE, BGZF_INPUT_ENDED, BGZF_OUTPUT_FULL,
 BGZF_OUTPUT_SHORT, BGZF_BAD_CRC) = range(9)
GL_GQ, GL_GL, GL_PL = 0, 1, 2
MISSING = -9999.0

# every symbol include/garlic_hip.h declares (tests check the library exports them all)
SYMBOLS = [
    "garlic_hip_abi_version", "garlic_hip_last_error", "garlic_hip_device_count",
    "garlic_ctx_create", "garlic_ctx_destroy", "garlic_ctx_synchronize",
    "garlic_panel_create", "garlic_panel_destroy", "garlic_panel_set_map",
    "garlic_panel_set_freq", "garlic_panel_set_genotypes", "garlic_panel_set_genotypes_2bit", "garlic_panel_set_gl", "garlic_panel_set_gl_codes",
    "garlic_panel_set_phase",
    "garlic_panel_set_ld", "garlic_lod_out_layout", "garlic_lod_windows", "garlic_lod_windows_multi",
    "garlic_wlod_windows", "garlic_lod_flatten", "garlic_last_call_stats",
    "garlic_panel_compute_ld", "garlic_ld_counts", "garlic_ld_finish", "garlic_roh_coverage",
    "garlic_panel_release_scratch",
    "garlic_lod_feed", "garlic_ctx_set_async",
    "garlic_recent_kernel_ms", "garlic_panel_tgls_mode", "garlic_lod_feed_subset", "garlic_lod_feed_multi",
    "garlic_device_alloc", "garlic_device_free", "garlic_panel_chain_kind", "garlic_device_alloc_stats",
    "garlic_panel_alloc_scores", "garlic_device_trim", "garlic_roh_coverage_fused", "garlic_roh_segments",
    "garlic_panel_alloc_scores_info", "garlic_lod_feed_info",
    "garlic_panel_set_tgls_term_budget", "garlic_panel_tgls_terms_info",
    "garlic_lod_feed_multi_tgls", "garlic_lod_feed_multi_info",
    "garlic_panel_compute_ld_multi", "garlic_ld_finish_multi", "garlic_panel_ld_info",
    "garlic_panel_set_feed_order", "garlic_feed_sort", "garlic_feed_sort_info",
    "garlic_panel_set_phase_bits", "garlic_panel_ld_form_info",
    "garlic_panel_set_gl_codes16",
    "garlic_bed_create", "garlic_bed_set_rows", "garlic_bed_census", "garlic_bed_destroy", "garlic_panel_set_genotypes_bed",
    "garlic_bed_extract", "garlic_bed_get_rows",
    "garlic_bed_set_order_rows", "garlic_bed_get_order_rows", "garlic_bed_set_rows_vcf", "garlic_panel_set_phase_bed",
    "garlic_bed_set_rows_tped", "garlic_bed_set_census",
    "garlic_tgls_create", "garlic_tgls_set_rows_text", "garlic_tgls_set_rows_values", "garlic_tgls_get_rows", "garlic_tgls_info",
    "garlic_tgls_get_values", "garlic_tgls_count_values", "garlic_tgls_set_rows_vcf", "garlic_device_upload",
    "garlic_tgls_destroy", "garlic_panel_set_gl_tgls",
    "garlic_feed_kde", "garlic_lod_kde", "garlic_feed_kde_info", "garlic_feed_kde_times",
    "garlic_gmm_fit", "garlic_gmm_fit_info",
    "garlic_kde_part_create", "garlic_lod_kde_part", "garlic_kde_part_destroy", "garlic_kde_part_count",
    "garlic_kde_part_moment", "garlic_kde_part_rank", "garlic_kde_part_sums", "garlic_kde_parts", "garlic_kde_parts_info",
    "garlic_feature_set_create", "garlic_feature_set_destroy", "garlic_feature_set_rows", "garlic_feature_set_sites",
    "garlic_feature_counts", "garlic_feature_counts_info", "garlic_feature_set_rows_bed", "garlic_feature_set_get_rows",
    "garlic_feed_kde_multi", "garlic_lod_kde_multi", "garlic_feed_kde_multi_info",
    "garlic_kde_part_set_create", "garlic_lod_kde_part_set", "garlic_kde_part_set_destroy", "garlic_kde_part_set_counts",
    "garlic_kde_part_set_moment", "garlic_kde_part_set_rank", "garlic_kde_part_set_sums", "garlic_kde_parts_multi",
    "garlic_kde_parts_multi_info",
    "garlic_bgzf_inflate", "garlic_text_lines", "garlic_device_download", "garlic_device_copy",
]
FEATURE_MAX_EFFECTS = 256   # GARLIC_FEATURE_MAX_EFFECTS
FEATURE_GROUP_EFFECTS = 32  # effects per launch
FEATURE_CHUNK_ROWS = 4096   # rows per wavefront
ROH_INTERVAL = np.dtype([("ind", "<i4"), ("chr", "<i4"), ("start", "<i4"), ("stop", "<i4"), ("cls", "<i4")])   # garlic_roh_interval
KDE_POINTS = 512   # GARLIC_KDE_POINTS
KDE_MAX_PARTS = 64   # GARLIC_KDE_MAX_PARTS
KDE_MAX_FEEDS = 32   # GARLIC_KDE_MAX_FEEDS
KDE_RANK_MAX = 1024  # probe keys of one garlic_kde_part_rank
GMM_MAX_K = 8      # GARLIC_GMM_MAX_K


class CallStats(C.Structure):
    _fields_ = [("n_segments", C.c_int64), ("n_runs", C.c_int64), ("n_chain_items", C.c_int64),
                ("n_valid_windows", C.c_int64), ("n_missing", C.c_int64),
                ("chain_kernel_ms", C.c_float), ("total_ms", C.c_float),
                ("n_stall_reruns", C.c_int64), ("n_count_timeouts", C.c_int64)]


class Kde(C.Structure):
    """garlic_kde"""
    _fields_ = [("n", C.c_int64), ("h", C.c_double), ("sd", C.c_double), ("q25", C.c_double), ("q75", C.c_double),
                ("lo", C.c_double), ("hi", C.c_double), ("x", C.c_double * KDE_POINTS), ("y", C.c_double * KDE_POINTS),
                ("raw", C.c_double * KDE_POINTS)]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("n", "h", "sd", "q25", "q75", "lo", "hi")}
        for k in ("x", "y", "raw"):
            d[k] = np.array(getattr(self, k), dtype=np.float64)
        return d


class Gmm(C.Structure):
    """garlic_gmm"""
    _fields_ = [("k", C.c_int32), ("iterations", C.c_int32), ("converged", C.c_int32),
                ("a", C.c_double * GMM_MAX_K), ("mean", C.c_double * GMM_MAX_K), ("var", C.c_double * GMM_MAX_K),
                ("loglik", C.c_double), ("bic", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k in ("k", "iterations", "converged", "loglik", "bic")}
        for k in ("a", "mean", "var"):
            d[k] = np.array(getattr(self, k), dtype=np.float64)[:self.k]
        return d


class GarlicError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libgarlic_hip error {code}: {msg}")
        self.code = code


_lib = None
_vp = C.c_void_p
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)


ABI_VERSION = 8   # GARLIC_HIP_ABI_VERSION of include/garlic_hip.h these bindings were written against


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C garlic_amd/csrc` (there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    L.garlic_hip_abi_version.restype = C.c_int
    if L.garlic_hip_abi_version() != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {L.garlic_hip_abi_version()}, these bindings need "
                          f"{ABI_VERSION}: rebuild it (make -C garlic_amd/csrc)")
    L.garlic_hip_last_error.restype = C.c_char_p
    L.garlic_hip_device_count.argtypes = [_i32p]
    L.garlic_ctx_create.argtypes = [C.c_int32, _vp, C.POINTER(_vp)]
    L.garlic_ctx_destroy.argtypes = [_vp]
    L.garlic_ctx_synchronize.argtypes = [_vp]
    L.garlic_ctx_set_async.argtypes = [_vp, C.c_int32]
    L.garlic_device_alloc.argtypes = [_vp, C.c_int64, C.POINTER(_vp)]
    L.garlic_device_alloc_stats.argtypes = [_vp, _i64p, _i64p, _i64p]
    L.garlic_panel_alloc_scores.argtypes = [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.POINTER(_vp),
                                            C.POINTER(C.c_float)]
    L.garlic_device_free.argtypes = [_vp, _vp]
    L.garlic_recent_kernel_ms.argtypes = [_vp, C.POINTER(C.c_float), C.c_int32, _i32p]
    L.garlic_panel_create.argtypes = [_vp, C.c_int32, _i32p, C.c_int32, C.POINTER(_vp)]
    L.garlic_panel_destroy.argtypes = [_vp]
    L.garlic_panel_set_map.argtypes = [_vp, _i32p, _f64p, _i32p, _i32p]
    L.garlic_panel_set_freq.argtypes = [_vp, _f64p]
    L.garlic_panel_set_genotypes.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32]
    L.garlic_panel_set_gl.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32]
    L.garlic_panel_release_scratch.argtypes = [_vp]
    L.garlic_lod_windows_multi.argtypes = [_vp, _i32p, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, _vp, C.c_int64, C.c_int32]
    L.garlic_panel_set_gl_codes.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, _vp, C.c_int32, C.c_int32]
    L.garlic_panel_set_gl_codes16.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, _vp, C.c_int32, C.c_int32]
    L.garlic_panel_set_genotypes_2bit.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32]
    L.garlic_panel_set_phase.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32]
    L.garlic_panel_set_ld.argtypes = [_vp, C.c_int32, _vp, C.c_int32]
    L.garlic_lod_out_layout.argtypes = [_vp, C.c_int32, C.c_int32, _i64p, _i64p, _i64p]
    L.garlic_lod_windows.argtypes = [_vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_int32, _vp, C.c_int32]
    L.garlic_wlod_windows.argtypes = [_vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32,
                                      C.c_double, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32]
    L.garlic_lod_flatten.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int64, _i64p]
    L.garlic_last_call_stats.argtypes = [_vp, C.POINTER(CallStats)]
    L.garlic_panel_compute_ld.argtypes = [_vp, C.c_int32, C.c_int32, _i32p, C.c_int32, _vp, C.c_int32]
    L.garlic_ld_counts.argtypes = [_vp, C.c_int32, C.c_int32, _i32p, C.c_int32, _vp, _vp, C.c_int32]
    L.garlic_ld_finish.argtypes = [_vp, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_int32]
    L.garlic_lod_feed.argtypes = [_vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_double, C.c_int32, _vp, C.c_int64, _i64p, _i64p]
    L.garlic_roh_coverage.argtypes = [_vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, _vp, C.c_int32,
                                      C.c_int32]
    L.garlic_roh_coverage_fused.argtypes = [_vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                            C.c_double, _vp, C.c_int32, C.c_int32]
    L.garlic_roh_segments.argtypes = [_vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double,
                                      C.c_double, C.c_double, _vp, C.c_int64, _i64p]
    L.garlic_lod_feed_subset.argtypes = [_vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_double, C.c_int32, _i32p, C.c_int32, _vp, C.c_int64, _i64p, _i64p]
    L.garlic_lod_feed_multi.argtypes = [_vp, _i32p, _i32p, C.c_int32, C.c_double, C.c_int32, _i32p, C.c_int32,
                                        C.POINTER(C.c_void_p), _i64p, _i64p, _i64p]
    L.garlic_lod_feed_multi_tgls.argtypes = [_vp, _i32p, _i32p, C.c_int32, C.c_int32, _i32p, C.c_int32,
                                             C.POINTER(C.c_void_p), _i64p, _i64p, _i64p]
    L.garlic_lod_feed_multi_info.argtypes = [_vp, C.c_int32, _i32p, _i32p, _i32p, _i32p]
    L.garlic_panel_tgls_mode.argtypes = [_vp, _i32p, _i32p]
    L.garlic_panel_chain_kind.argtypes = [_vp, _i32p]
    L.garlic_lod_feed_info.argtypes = [_vp, _i32p, _i64p]
    L.garlic_panel_set_tgls_term_budget.argtypes = [_vp, C.c_int64]
    L.garlic_panel_tgls_terms_info.argtypes = [_vp, _i64p, _i64p, _i32p, _i32p]
    L.garlic_panel_compute_ld_multi.argtypes = [_vp, _i32p, C.c_int32, C.c_int32, _i32p, C.c_int32, C.POINTER(_vp), C.c_int32]
    L.garlic_ld_finish_multi.argtypes = [_vp, _i32p, C.c_int32, C.c_int32, _vp, _vp, C.POINTER(_vp), C.c_int32]
    L.garlic_panel_ld_info.argtypes = [_vp, C.c_int32, _i32p, _i32p, _i32p, _i64p, _i32p, _i32p]
    L.garlic_panel_set_feed_order.argtypes = [_vp, C.c_int32]
    L.garlic_panel_set_phase_bits.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32]
    L.garlic_panel_ld_form_info.argtypes = [_vp, _i32p, _i32p, _i32p, _i32p]
    L.garlic_feed_sort.argtypes = [_vp, _vp, C.c_int64, C.c_int32]
    L.garlic_feed_sort_info.argtypes = [_vp, _i32p, _i32p, _i64p]
    L.garlic_feed_kde.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(Kde)]
    L.garlic_lod_kde.argtypes = [_vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                 _i32p, C.c_int32, C.POINTER(Kde), _i64p]
    L.garlic_feed_kde_info.argtypes = [_vp, _i64p, _i64p, _i64p]
    L.garlic_feed_kde_times.argtypes = [_vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.garlic_feed_kde_multi.argtypes = [_vp, C.POINTER(_vp), _i64p, C.c_int32, C.c_int32, C.POINTER(Kde), _i32p]
    L.garlic_lod_kde_multi.argtypes = [_vp, _i32p, _i32p, C.c_int32, C.c_double, C.c_int32, C.c_int32, _i32p, C.c_int32,
                                       C.POINTER(Kde), _i32p, _i64p]
    L.garlic_feed_kde_multi_info.argtypes = [_vp, C.c_int32, _i64p, _i64p, _i32p, _i32p, _i64p, C.POINTER(C.c_float),
                                             C.POINTER(C.c_float)]
    L.garlic_kde_part_create.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.POINTER(_vp)]
    L.garlic_lod_kde_part.argtypes = [_vp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                      _i32p, C.c_int32, C.POINTER(_vp), _i64p]
    L.garlic_kde_part_destroy.argtypes = [_vp]
    L.garlic_kde_part_count.argtypes = [_vp, _i64p]
    L.garlic_kde_part_moment.argtypes = [_vp, C.c_int32, C.c_double, _f64p, _f64p, _f64p]
    L.garlic_kde_part_rank.argtypes = [_vp, C.POINTER(C.c_uint64), C.c_int32, _i64p]
    L.garlic_kde_part_sums.argtypes = [_vp, _f64p, C.c_double, _f64p]
    L.garlic_kde_parts.argtypes = [C.POINTER(_vp), C.c_int32, C.POINTER(Kde)]
    L.garlic_kde_parts_info.argtypes = [C.POINTER(_vp), C.c_int32, _i64p, _i64p, _i32p, C.POINTER(C.c_float)]
    L.garlic_kde_part_set_create.argtypes = [_vp, C.POINTER(_vp), _i64p, C.c_int32, C.c_int32, C.POINTER(_vp)]
    L.garlic_lod_kde_part_set.argtypes = [_vp, _i32p, _i32p, C.c_int32, C.c_double, C.c_int32, C.c_int32, _i32p, C.c_int32,
                                          C.POINTER(_vp), _i64p]
    L.garlic_kde_part_set_destroy.argtypes = [_vp]
    L.garlic_kde_part_set_counts.argtypes = [_vp, _i64p]
    L.garlic_kde_part_set_moment.argtypes = [_vp, C.c_int32, _f64p, _f64p, _f64p, _f64p, _i32p]
    L.garlic_kde_part_set_rank.argtypes = [_vp, C.POINTER(C.c_uint64), C.c_int32, _i64p]
    L.garlic_kde_part_set_sums.argtypes = [_vp, _f64p, _f64p, _i32p, _f64p, _i64p]
    L.garlic_kde_parts_multi.argtypes = [C.POINTER(_vp), C.c_int32, C.POINTER(Kde), _i32p]
    L.garlic_kde_parts_multi_info.argtypes = [C.POINTER(_vp), C.c_int32, _i64p, _i64p, _i32p, _i32p, _i32p, C.POINTER(C.c_float),
                                              C.POINTER(C.c_float)]
    L.garlic_feature_set_create.argtypes = [_vp, C.c_int64, C.c_int32, C.POINTER(_vp)]
    L.garlic_feature_set_destroy.argtypes = [_vp]
    L.garlic_feature_set_rows.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int64]
    L.garlic_feature_set_sites.argtypes = [_vp, _i32p, _i32p, _i32p]
    L.garlic_feature_set_rows_bed.argtypes = [_vp, _vp, _vp, _vp, C.c_int64, C.c_int64]
    L.garlic_feature_set_get_rows.argtypes = [_vp, C.c_int64, C.c_int64, _vp, C.c_int64]
    L.garlic_feature_counts.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, _vp, C.c_int32]
    L.garlic_feature_counts_info.argtypes = [_vp, _i64p, _i64p, _i64p, C.POINTER(C.c_float)]
    L.garlic_gmm_fit.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int32, _f64p, _f64p, _f64p, C.c_int32, C.c_double, C.POINTER(Gmm)]
    L.garlic_gmm_fit_info.argtypes = [_vp, _i64p, _i64p, C.POINTER(C.c_float)]
    L.garlic_bed_create.argtypes = [_vp, C.c_int64, C.c_int32, C.POINTER(_vp)]
    L.garlic_bed_set_rows.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32]
    L.garlic_bed_census.argtypes = [_vp, _vp, _vp, C.c_int32]
    L.garlic_bed_destroy.argtypes = [_vp]
    L.garlic_bed_extract.argtypes = [_vp, _vp, C.c_int32, C.POINTER(_vp)]
    L.garlic_bed_get_rows.argtypes = [_vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_int32]
    L.garlic_panel_set_genotypes_bed.argtypes = [_vp, _vp, C.c_int64, _i64p]
    L.garlic_bed_set_order_rows.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32]
    L.garlic_bed_get_order_rows.argtypes = [_vp, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_int32]
    L.garlic_bed_set_rows_vcf.argtypes = [_vp, _vp, C.c_int64, _i64p, C.c_int64, C.c_int64, _vp, C.c_int32]
    L.garlic_panel_set_phase_bed.argtypes = [_vp, _vp, C.c_int64, _i64p]
    L.garlic_bed_set_rows_tped.argtypes = [_vp, _vp, C.c_int64, _i64p, C.c_int64, C.c_int64, C.c_uint8, _vp, _vp, C.c_int32]
    L.garlic_bed_set_census.argtypes = [_vp, _vp, _vp, C.c_int32]
    L.garlic_tgls_create.argtypes = [_vp, C.c_int64, C.c_int32, _i32p, C.c_int32, C.POINTER(_vp)]
    L.garlic_tgls_set_rows_text.argtypes = [_vp, _vp, C.c_int64, _i64p, C.c_int64, C.c_int64, _vp, C.c_int32]
    L.garlic_tgls_set_rows_vcf.argtypes = [_vp, _vp, C.c_int64, _i64p, C.c_int64, C.c_int64, C.c_char_p, _f64p, _vp, C.c_int32]
    L.garlic_device_upload.argtypes = [_vp, _vp, _vp, C.c_int64]
    L.garlic_device_download.argtypes = [_vp, _vp, _vp, C.c_int64]
    L.garlic_device_copy.argtypes = [_vp, _vp, _vp, C.c_int64]
    L.garlic_bgzf_inflate.argtypes = [_vp, _vp, C.c_int64, _i64p, C.c_int64, _vp, _i64p, _i32p, C.c_int32]
    L.garlic_text_lines.argtypes = [_vp, _vp, C.c_int64, C.c_int32, C.c_int64, C.c_int64, C.c_int64, _i64p, _i64p, _i64p, _vp, _i64p, _i64p,
                                    _i64p]
    L.garlic_tgls_set_rows_values.argtypes = [_vp, _vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32]
    L.garlic_tgls_get_rows.argtypes = [_vp, C.c_int32, C.c_int64, C.c_int64, _vp, C.c_int64, C.c_int32]
    L.garlic_tgls_info.argtypes = [_vp, _i32p, _i64p, _i64p]
    L.garlic_tgls_get_values.argtypes = [_vp, C.c_int32, _f64p, C.c_int32]
    L.garlic_tgls_count_values.argtypes = [_vp, C.c_int32, C.c_int64, C.c_int64, _i32p]
    L.garlic_tgls_destroy.argtypes = [_vp]
    L.garlic_panel_set_gl_tgls.argtypes = [_vp, _vp, C.c_int32, C.c_int64, _i64p]
    for name in SYMBOLS:
        f = getattr(L, name)
        if f.restype is C.c_int and name not in ("garlic_hip_abi_version",):
            f.restype = C.c_int
    _lib = L
    return L


def check(rc):
    if rc != OK:
        raise GarlicError(rc, lib().garlic_hip_last_error().decode())


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


class Context:
    """One device + one HIP stream (garlic_ctx).  stream: a hipStream_t handle (int) the caller owns, e.g.
    torch.cuda.Stream().cuda_stream; the calls then keep that stream's order.  None or 0: the context creates a private
    non-blocking stream.  Torch's DEFAULT stream has handle 0, so stream=torch.cuda.current_stream().cuda_stream on the
    default stream silently gets the private stream, unordered with torch's work: create a torch.cuda.Stream() instead."""

    def __init__(self, device=0, stream=None):
        self.handle = _vp()
        check(lib().garlic_ctx_create(device, _vp(stream) if stream else None, C.byref(self.handle)))
        self.device = device

    def synchronize(self):
        check(lib().garlic_ctx_synchronize(self.handle))

    def recent_kernel_ms(self, n=32):
        """HIP-event durations of the dominant kernel of the last <= n (<= 32) score calls, oldest first"""
        buf = (C.c_float * n)()
        got = C.c_int32()
        check(lib().garlic_recent_kernel_ms(self.handle, buf, n, C.byref(got)))
        return [float(buf[i]) for i in range(got.value)]

    def set_async(self, on=True):
        """device-output calls that repeat the previous call's arguments only enqueue (see garlic_hip.h)"""
        check(lib().garlic_ctx_set_async(self.handle, int(on)))

    def alloc_scores(self, n_doubles):
        """device memory for a score matrix through garlic_device_alloc (pooled; see garlic_hip.h)"""
        return DeviceBuffer(self, int(n_doubles) * 8)

    def trim(self):
        """garlic_device_trim: idle pooled score buffers give their memory back"""
        check(lib().garlic_device_trim(self.handle))

    def alloc_stats(self):
        """garlic_device_alloc_stats: (live, pooled, reserved) bytes of score memory on this context's device"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().garlic_device_alloc_stats(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def feed_sort(self, values, n=None):
        """garlic_feed_sort: ascending order in place (the array nrd0's gsl_sort leaves; key order in garlic_hip.h).
        values: a contiguous float64 numpy array (host; n defaults to its length) or a device address (int) of n doubles."""
        if isinstance(values, np.ndarray):
            assert values.dtype == np.float64 and values.flags["C_CONTIGUOUS"] and values.ndim == 1
            n = values.shape[0] if n is None else int(n)
            assert n <= values.shape[0]
            check(lib().garlic_feed_sort(self.handle, _vp(values.ctypes.data), n, HOST))
        else:
            check(lib().garlic_feed_sort(self.handle, _vp(values) if values else None, int(n), DEVICE))
        return values

    def feed_sort_info(self):
        """garlic_feed_sort_info: {passes_run, passes_skipped, scratch_bytes} of the last sort on this context"""
        run, skipped, nbytes = C.c_int32(), C.c_int32(), C.c_int64()
        check(lib().garlic_feed_sort_info(self.handle, C.byref(run), C.byref(skipped), C.byref(nbytes)))
        return {"passes_run": run.value, "passes_skipped": skipped.value, "scratch_bytes": nbytes.value}

    def feed_kde(self, values, n=None, out=None):
        """garlic_feed_kde: computeKDE's bandwidth, targets and density of an ascending feed, as a dict: n, h, sd, q25,
        q75, lo, hi and the float64 arrays x, y, raw [512].  values: a contiguous float64 numpy array (host; n defaults to
        its length) or a device address (int) of n doubles.  out: an abi.Kde to fill instead (returned as it is)."""
        k = Kde() if out is None else out
        if isinstance(values, np.ndarray):
            assert values.dtype == np.float64 and values.flags["C_CONTIGUOUS"] and values.ndim == 1
            n = values.shape[0] if n is None else int(n)
            assert n <= values.shape[0]
            check(lib().garlic_feed_kde(self.handle, _vp(values.ctypes.data), n, HOST, C.byref(k)))
        else:
            check(lib().garlic_feed_kde(self.handle, _vp(values) if values else None, int(n), DEVICE, C.byref(k)))
        return k.as_dict() if out is None else out

    def feed_kde_info(self):
        """garlic_feed_kde_info: {chunks, pairs_skipped, scratch_bytes} of the last KDE on this context"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().garlic_feed_kde_info(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return {"chunks": a.value, "pairs_skipped": b.value, "scratch_bytes": c.value}

    def feed_kde_times(self):
        """garlic_feed_kde_times: {moments_ms, sums_ms}, HIP-event times of the last KDE's kernels on this context"""
        a, b = C.c_float(), C.c_float()
        check(lib().garlic_feed_kde_times(self.handle, C.byref(a), C.byref(b)))
        return {"moments_ms": a.value, "sums_ms": b.value}

    def feed_kde_multi(self, feeds, ns=None, strict=False, outs=None):
        """garlic_feed_kde_multi: the KDEs of up to KDE_MAX_FEEDS ascending feeds from one set of launches.  feeds: a list
        of contiguous float64 numpy arrays (host; ns defaults to their lengths), or of device addresses (int) with ns their
        lengths.  Returns ([feed_kde's dict, or None for a refused feed], [status per feed], None).  strict: no per-feed
        status -- any refused feed raises.  outs: an (abi.Kde * len(feeds)) array to fill instead of a fresh one."""
        m = len(feeds)
        host = all(isinstance(f, np.ndarray) for f in feeds)
        assert host or not any(isinstance(f, np.ndarray) for f in feeds), "host arrays or device addresses, not both"
        if host:
            for f in feeds:
                assert f.dtype == np.float64 and f.flags["C_CONTIGUOUS"] and f.ndim == 1
            ns = [f.shape[0] for f in feeds] if ns is None else [int(v) for v in ns]
            ptrs = (_vp * max(m, 1))(*[f.ctypes.data for f in feeds])
        else:
            ptrs = (_vp * max(m, 1))(*[int(f) if f else None for f in feeds])
        lens = np.ascontiguousarray(ns, dtype=np.int64)
        assert lens.shape == (m,)
        return _kde_multi_result(lambda ks, st: lib().garlic_feed_kde_multi(self.handle, ptrs, _ptr(lens, _i64p), m, HOST if host else DEVICE,
                                                                           ks, st), m, strict, outs) + (None,)

    def feed_kde_multi_info(self, n):
        """garlic_feed_kde_multi_info for the first n feeds of the last multi-feed KDE on this context: {chunks [n],
        pairs_skipped [n], kernel_launches, host_waits, scratch_bytes, moments_ms, sums_ms}"""
        chunks, skipped = np.zeros(max(n, 1), dtype=np.int64), np.zeros(max(n, 1), dtype=np.int64)
        launches, waits, nbytes, a, b = C.c_int32(), C.c_int32(), C.c_int64(), C.c_float(), C.c_float()
        check(lib().garlic_feed_kde_multi_info(self.handle, n, _ptr(chunks, _i64p), _ptr(skipped, _i64p), C.byref(launches), C.byref(waits),
                                               C.byref(nbytes), C.byref(a), C.byref(b)))
        return {"chunks": [int(v) for v in chunks[:n]], "pairs_skipped": [int(v) for v in skipped[:n]], "kernel_launches": launches.value,
                "host_waits": waits.value, "scratch_bytes": nbytes.value, "moments_ms": a.value, "sums_ms": b.value}

    def kde_part(self, values, n=None):
        """garlic_kde_part_create: an ascending feed (garlic_feed_sort's key order) as one part of a split feed, an
        abi.KdePart.  values: a contiguous float64 numpy array (host, uploaded; n defaults to its length) or a device address
        (int) of n doubles, borrowed until the part is closed."""
        h = _vp()
        if isinstance(values, np.ndarray):
            assert values.dtype == np.float64 and values.flags["C_CONTIGUOUS"] and values.ndim == 1
            n = values.shape[0] if n is None else int(n)
            assert n <= values.shape[0]
            check(lib().garlic_kde_part_create(self.handle, _vp(values.ctypes.data), n, HOST, C.byref(h)))
        else:
            check(lib().garlic_kde_part_create(self.handle, _vp(values) if values else None, int(n), DEVICE, C.byref(h)))
        return KdePart(h)

    def kde_part_set(self, feeds, ns=None):
        """garlic_kde_part_set_create: one shard's parts of several split feeds, an abi.KdePartSet.  feeds: a list of
        contiguous float64 numpy arrays (host, uploaded; ns defaults to their lengths), or of device addresses (int, 0 for an
        empty feed) with ns their lengths, borrowed until the set is closed."""
        m = len(feeds)
        host = all(isinstance(f, np.ndarray) for f in feeds)
        assert host or not any(isinstance(f, np.ndarray) for f in feeds), "host arrays or device addresses, not both"
        if host:
            for f in feeds:
                assert f.dtype == np.float64 and f.flags["C_CONTIGUOUS"] and f.ndim == 1
            ns = [f.shape[0] for f in feeds] if ns is None else [int(v) for v in ns]
            ptrs = (_vp * max(m, 1))(*[f.ctypes.data for f in feeds])
        else:
            ptrs = (_vp * max(m, 1))(*[int(f) if f else None for f in feeds])
        lens = np.ascontiguousarray(ns, dtype=np.int64)
        assert lens.shape == (m,)
        h = _vp()
        check(lib().garlic_kde_part_set_create(self.handle, ptrs, _ptr(lens, _i64p), m, HOST if host else DEVICE, C.byref(h)))
        return KdePartSet(h, m)

    def gmm_fit(self, values, a0, mean0, var0, n=None, max_iter=1000, precision=1e-5, out=None):
        """garlic_gmm_fit: GMM::estimate's EM fit of len(a0) Gaussians, as a dict: k, iterations, converged, loglik, bic and
        the float64 arrays a, mean, var [k].  values: a contiguous float64 numpy array (host; n defaults to its length) or
        a device address (int) of n doubles.  out: an abi.Gmm to fill instead (returned as it is)."""
        g = Gmm() if out is None else out
        init = [np.ascontiguousarray(v, dtype=np.float64) for v in (a0, mean0, var0)]
        k = init[0].shape[0]
        assert all(v.shape == (k,) for v in init)
        ptrs = [_ptr(v, _f64p) for v in init]
        if isinstance(values, np.ndarray):
            assert values.dtype == np.float64 and values.flags["C_CONTIGUOUS"] and values.ndim == 1
            n = values.shape[0] if n is None else int(n)
            assert n <= values.shape[0]
            check(lib().garlic_gmm_fit(self.handle, _vp(values.ctypes.data), n, HOST, k, *ptrs, int(max_iter), float(precision), C.byref(g)))
        else:
            check(lib().garlic_gmm_fit(self.handle, _vp(values) if values else None, int(n), DEVICE, k, *ptrs, int(max_iter),
                                       float(precision), C.byref(g)))
        return g.as_dict() if out is None else out

    def gmm_fit_info(self):
        """garlic_gmm_fit_info: {blocks, scratch_bytes, em_ms} of the last GMM fit on this context"""
        a, b, c = C.c_int64(), C.c_int64(), C.c_float()
        check(lib().garlic_gmm_fit_info(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return {"blocks": a.value, "scratch_bytes": b.value, "em_ms": c.value}

    def close(self):
        if self.handle:
            lib().garlic_ctx_destroy(self.handle)
            self.handle = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class FeatureSet:
    """garlic_feature_set: the hom rows of annotated alleles over nind individuals (garlic_hip.h).  rows: uint8 [nrows,
    row_bytes], bit i & 7 of byte i >> 3 is individual i; chr / pos / effect: int32 [nrows], sorted by (chr, pos).  Close it
    before its context."""

    def __init__(self, ctx, nrows, nind, rows=None, chr=None, pos=None, effect=None):
        self.nrows, self.nind = int(nrows), int(nind)
        self.handle = _vp()
        check(lib().garlic_feature_set_create(ctx.handle, self.nrows, self.nind, C.byref(self.handle)))
        try:
            if rows is not None and self.nrows:
                self.set_rows(rows)
            if chr is not None:
                self.set_sites(chr, pos, effect)
        except Exception:
            self.close()
            raise

    def set_rows(self, rows, row_begin=0):
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        assert rows.ndim == 2
        check(lib().garlic_feature_set_rows(self.handle, _vp(rows.ctypes.data), rows.shape[1], int(row_begin), rows.shape[0]))

    def set_rows_bed(self, bed, file_row, allele, row_begin=0):
        """rows row_begin .. from a Bed image on the same device: row row_begin + k is image row file_row[k], hom A1 (allele[k]
        = 0), hom A2 (1) or empty (2)"""
        file_row = np.ascontiguousarray(file_row, dtype=np.int64)
        allele = np.ascontiguousarray(allele, dtype=np.uint8)
        assert file_row.ndim == 1 and file_row.shape == allele.shape
        n = file_row.shape[0]
        check(lib().garlic_feature_set_rows_bed(self.handle, bed.handle, _vp(file_row.ctypes.data) if n else None,
                                                _vp(allele.ctypes.data) if n else None, int(row_begin), n))

    def get_rows(self, row_begin=0, row_count=None):
        """uint8 [row_count, (nind + 7) // 8]: the rows as they stand on the device, in set_rows' format (waits for the set's work)"""
        row_count = self.nrows - row_begin if row_count is None else row_count
        rows = np.zeros((max(row_count, 0), (self.nind + 7) // 8), dtype=np.uint8)
        check(lib().garlic_feature_set_get_rows(self.handle, int(row_begin), int(row_count), _vp(rows.ctypes.data) if rows.size else None,
                                                rows.shape[1]))
        return rows

    def set_sites(self, chr, pos, effect):
        a = [np.ascontiguousarray(v, dtype=np.int32) for v in (chr, pos, effect)]
        assert all(v.shape == (self.nrows,) for v in a)
        check(lib().garlic_feature_set_sites(self.handle, *[_ptr(v, _i32p) for v in a]))

    @staticmethod
    def _intervals(intervals):
        iv = np.ascontiguousarray(intervals, dtype=ROH_INTERVAL)
        assert iv.ndim == 1
        return iv

    def counts(self, intervals, n_classes, n_effects):
        """garlic_feature_counts to the host: int64 [nind, n_classes + 1, n_effects]; intervals: an array of ROH_INTERVAL"""
        iv = self._intervals(intervals)
        out = np.full((self.nind, n_classes + 1, n_effects), -1, dtype=np.int64)
        check(lib().garlic_feature_counts(self.handle, _vp(iv.ctypes.data) if iv.shape[0] else None, iv.shape[0], int(n_classes),
                                          int(n_effects), _vp(out.ctypes.data), HOST))
        return out

    def counts_device(self, intervals, n_classes, n_effects, out):
        """the same into device memory (out: a torch int64 tensor of nind * (n_classes + 1) * n_effects elements, or its
        address): enqueued on the context's stream, no wait"""
        iv = self._intervals(intervals)
        ptr = out if isinstance(out, int) else out.data_ptr()
        if not isinstance(out, int):
            assert out.numel() >= self.nind * (n_classes + 1) * n_effects and out.element_size() == 8 and out.is_contiguous()
        check(lib().garlic_feature_counts(self.handle, _vp(iv.ctypes.data) if iv.shape[0] else None, iv.shape[0], int(n_classes),
                                          int(n_effects), _vp(ptr), DEVICE))

    def info(self):
        """garlic_feature_counts_info: {blocks, chunks, words_skipped, kernel_ms} of the last count (waits for it)"""
        b, c, w = C.c_int64(), C.c_int64(), C.c_int64()
        ms = C.c_float()
        check(lib().garlic_feature_counts_info(self.handle, C.byref(b), C.byref(c), C.byref(w), C.byref(ms)))
        return {"blocks": b.value, "chunks": c.value, "words_skipped": w.value, "kernel_ms": ms.value}

    def close(self):
        if self.handle:
            lib().garlic_feature_set_destroy(self.handle)
            self.handle = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _kde_multi_result(call, m, strict, outs):
    """runs call(outs, status) of a multi-feed KDE; -> ([dict or None], [status])"""
    ks = (Kde * max(m, 1))() if outs is None else outs
    status = None if strict else np.full(max(m, 1), -1, dtype=np.int32)
    check(call(ks, _ptr(status, _i32p)))
    codes = [OK] * m if strict else [int(v) for v in status[:m]]
    return [ks[i].as_dict() if codes[i] == OK else None for i in range(m)], codes


class KdePart:
    """garlic_kde_part: one sorted part of a split feed (Context.kde_part, Panel.lod_kde_part).  The step calls are what a
    caller with one process per GPU all-reduces between; kde_parts(parts) runs them all.  Close it before its context."""

    def __init__(self, handle):
        self.handle = handle

    def count(self):
        n = C.c_int64()
        check(lib().garlic_kde_part_count(self.handle, C.byref(n)))
        return n.value

    def moment(self, pass_, mean=0.0):
        """pass 0: (sum, x[0], x[n - 1]) -- (0.0, None, None) for an empty part; pass 1: the sum of (x - mean)^2"""
        v, lo, hi = C.c_double(), C.c_double(), C.c_double()
        check(lib().garlic_kde_part_moment(self.handle, int(pass_), float(mean), C.byref(v), C.byref(lo), C.byref(hi)))
        if pass_:
            return v.value
        return (v.value, lo.value, hi.value) if self.count() else (v.value, None, None)

    def rank(self, keys):
        """how many of the part's values have a key below each of keys (uint64, at most 1024): int64 array"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        below = np.zeros(keys.shape[0], dtype=np.int64)
        check(lib().garlic_kde_part_rank(self.handle, keys.ctypes.data_as(C.POINTER(C.c_uint64)), int(keys.shape[0]),
                                         _ptr(below, _i64p)))
        return below

    def sums(self, targets, h):
        """the part's 512 undivided Gaussian sums at targets for the bandwidth h"""
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        assert targets.shape == (KDE_POINTS,)
        out = np.zeros(KDE_POINTS, dtype=np.float64)
        check(lib().garlic_kde_part_sums(self.handle, _ptr(targets, _f64p), float(h), _ptr(out, _f64p)))
        return out

    def close(self):
        if self.handle:
            lib().garlic_kde_part_destroy(self.handle)
            self.handle = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _part_handles(parts):
    return (_vp * max(len(parts), 1))(*[None if p is None else p.handle for p in parts])


def kde_parts(parts, out=None):
    """garlic_kde_parts: the KDE of the union of the parts (KdePart objects, in this order), as Context.feed_kde's dict.
    out: an abi.Kde to fill instead (returned as it is)."""
    k = Kde() if out is None else out
    check(lib().garlic_kde_parts(_part_handles(parts), len(parts), C.byref(k)))
    return k.as_dict() if out is None else out


def kde_parts_info(parts):
    """garlic_kde_parts_info: {chunks [P], pairs_skipped [P], rank_rounds, sums_ms [P]} of the last KDE over these parts"""
    n = max(len(parts), 1)
    chunks, skipped = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    ms = np.zeros(n, dtype=np.float32)
    rounds = C.c_int32()
    check(lib().garlic_kde_parts_info(_part_handles(parts), len(parts), _ptr(chunks, _i64p), _ptr(skipped, _i64p), C.byref(rounds),
                                      ms.ctypes.data_as(C.POINTER(C.c_float))))
    return {"chunks": chunks[:len(parts)], "pairs_skipped": skipped[:len(parts)], "rank_rounds": rounds.value,
            "sums_ms": ms[:len(parts)]}


class KdePartSet:
    """garlic_kde_part_set: one shard's sorted parts of F split feeds (Context.kde_part_set, Panel.lod_kde_part_set).  The
    step calls work on all F feeds at once and are what a caller with one process per GPU all-reduces between;
    kde_parts_multi(sets) runs them all.  Close it before its context."""

    def __init__(self, handle, n_feeds):
        self.handle, self.n_feeds = handle, n_feeds

    def counts(self):
        n = np.zeros(self.n_feeds, dtype=np.int64)
        check(lib().garlic_kde_part_set_counts(self.handle, _ptr(n, _i64p)))
        return n

    def moment(self, pass_, means=None, status=None):
        """pass 0: (sums [F], lo [F], hi [F], status [F]) -- NaN in lo / hi of an empty or switched-off feed; pass 1: (the
        sums of (x - means[i])^2 [F], status).  status: int32 [F], nonzero switches a feed off (default: none)."""
        F = self.n_feeds
        st = np.zeros(F, dtype=np.int32) if status is None else np.ascontiguousarray(status, dtype=np.int32).copy()
        m = None if means is None else np.ascontiguousarray(means, dtype=np.float64)
        assert st.shape == (F,) and (m is None or m.shape == (F,))
        v, lo, hi = np.zeros(F), np.full(F, np.nan), np.full(F, np.nan)
        check(lib().garlic_kde_part_set_moment(self.handle, int(pass_), _ptr(m, _f64p), _ptr(v, _f64p), _ptr(lo, _f64p), _ptr(hi, _f64p),
                                               _ptr(st, _i32p)))
        return (v, st) if pass_ else (v, lo, hi, st)

    def rank(self, keys):
        """keys: uint64 [F, m], m <= 1024; how many values of feed i have a key below keys[i, t]: int64 [F, m]"""
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        assert keys.ndim == 2 and keys.shape[0] == self.n_feeds
        below = np.zeros(keys.shape, dtype=np.int64)
        check(lib().garlic_kde_part_set_rank(self.handle, keys.ctypes.data_as(C.POINTER(C.c_uint64)), int(keys.shape[1]),
                                             _ptr(below, _i64p)))
        return below

    def sums(self, targets, h, active=None):
        """targets [F, 512], h [F], active int32 [F] or None -> (the undivided Gaussian sums [F, 512], pairs_skipped [F])"""
        F = self.n_feeds
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        h = np.ascontiguousarray(h, dtype=np.float64)
        act = None if active is None else np.ascontiguousarray(active, dtype=np.int32)
        assert targets.shape == (F, KDE_POINTS) and h.shape == (F,) and (act is None or act.shape == (F,))
        out, skipped = np.zeros((F, KDE_POINTS)), np.zeros(F, dtype=np.int64)
        check(lib().garlic_kde_part_set_sums(self.handle, _ptr(targets, _f64p), _ptr(h, _f64p), _ptr(act, _i32p), _ptr(out, _f64p),
                                             _ptr(skipped, _i64p)))
        return out, skipped

    def close(self):
        if self.handle:
            lib().garlic_kde_part_set_destroy(self.handle)
            self.handle = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def kde_parts_multi(sets, strict=False, outs=None):
    """garlic_kde_parts_multi: the KDEs of the unions {feed i of every set, in this order}.  Returns ([feed_kde's dict, or
    None for a refused feed], [status per feed]); strict and outs as Context.feed_kde_multi."""
    m = sets[0].n_feeds if sets and sets[0] is not None else 0
    return _kde_multi_result(lambda ks, st: lib().garlic_kde_parts_multi(_part_handles(sets), len(sets), ks, st), m, strict, outs)


def kde_parts_multi_info(sets):
    """garlic_kde_parts_multi_info: {chunks [P, F], pairs_skipped [P, F], kernel_launches [P], host_waits [P], rank_rounds [P],
    moments_ms [P], sums_ms [P]} of the last KDE over these sets"""
    P, F = len(sets), sets[0].n_feeds
    chunks, skipped = np.zeros((P, F), dtype=np.int64), np.zeros((P, F), dtype=np.int64)
    launches, waits, rounds = (np.zeros(P, dtype=np.int32) for _ in range(3))
    mom, sums = np.zeros(P, dtype=np.float32), np.zeros(P, dtype=np.float32)
    fp = C.POINTER(C.c_float)
    check(lib().garlic_kde_parts_multi_info(_part_handles(sets), P, _ptr(chunks, _i64p), _ptr(skipped, _i64p), _ptr(launches, _i32p),
                                            _ptr(waits, _i32p), _ptr(rounds, _i32p), mom.ctypes.data_as(fp), sums.ctypes.data_as(fp)))
    return {"chunks": chunks, "pairs_skipped": skipped, "kernel_launches": launches, "host_waits": waits, "rank_rounds": rounds,
            "moments_ms": mom, "sums_ms": sums}


class DeviceBuffer:
    """garlic_device_alloc / garlic_device_free; `.ptr` for the device-output calls, `.tensor()` to look at it"""

    def __init__(self, ctx, nbytes, ptr=None):
        self.ctx, self.nbytes = ctx, nbytes
        if ptr is None:
            p = _vp()
            check(lib().garlic_device_alloc(ctx.handle, nbytes, C.byref(p)))
            ptr = p.value
        self.ptr = ptr

    def data_ptr(self):
        return self.ptr

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.nbytes // 8,), "typestr": "<f8", "data": (self.ptr, False), "version": 2, "strides": None}

    def tensor(self):
        """a float64 torch tensor over the same memory (valid while this object lives)"""
        import torch
        return torch.as_tensor(self, device=f"cuda:{self.ctx.device}")

    def free(self):
        if self.ptr:
            check(lib().garlic_device_free(self.ctx.handle, _vp(self.ptr)))
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def device_upload(ctx, dst_ptr, data):
    """garlic_device_upload: bytes / a contiguous numpy array to device address dst_ptr"""
    buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data).view(np.uint8).ravel()
    if buf.shape[0]:
        check(lib().garlic_device_upload(ctx.handle, _vp(dst_ptr), _vp(buf.ctypes.data), buf.shape[0]))


def device_download(ctx, src_ptr, nbytes):
    """garlic_device_download: nbytes from device address src_ptr as a uint8 array"""
    out = np.empty(int(nbytes), dtype=np.uint8)
    if nbytes:
        check(lib().garlic_device_download(ctx.handle, _vp(out.ctypes.data), _vp(src_ptr), int(nbytes)))
    return out


def device_copy(ctx, dst_ptr, src_ptr, nbytes):
    """garlic_device_copy: nbytes between device ranges that do not overlap"""
    check(lib().garlic_device_copy(ctx.handle, _vp(dst_ptr), _vp(src_ptr), int(nbytes)))


def bgzf_inflate(ctx, comp, block_begin, out_ptr, out_begin, comp_bytes=None, where=HOST):
    """garlic_bgzf_inflate: the BGZF blocks comp[block_begin[b], block_begin[b + 1]) to device memory out_ptr[out_begin[b],
    out_begin[b + 1]).  comp: bytes / uint8 array (host), or a device address with comp_bytes and where=DEVICE.
    Returns (status int32 [nblocks], error or None): a bad block fills its status and comes back as the GarlicError instead
    of being raised, so that a caller sees both."""
    bb = np.ascontiguousarray(block_begin, dtype=np.int64)
    ob = np.ascontiguousarray(out_begin, dtype=np.int64)
    assert bb.ndim == 1 and bb.shape == ob.shape and bb.shape[0] >= 1
    if where == HOST:
        buf = np.frombuffer(comp, dtype=np.uint8) if isinstance(comp, (bytes, bytearray)) else np.asarray(comp)
        assert buf.dtype == np.uint8 and buf.ndim == 1
        ptr, comp_bytes = buf.ctypes.data, buf.shape[0] if comp_bytes is None else comp_bytes
    else:
        ptr = int(comp)
    status = np.zeros(bb.shape[0] - 1, dtype=np.int32)
    rc = lib().garlic_bgzf_inflate(ctx.handle, _vp(ptr), int(comp_bytes), _ptr(bb, _i64p), bb.shape[0] - 1, _vp(out_ptr), _ptr(ob, _i64p),
                                   _ptr(status, _i32p), where)
    err = None
    if rc != OK:
        err = GarlicError(rc, lib().garlic_hip_last_error().decode())
        if rc != ERR_INVALID or not status.any():
            raise err
    return status, err


def text_lines(ctx, text_ptr, text_bytes, last, seen=0, head_bytes=0, capacity=None):
    """garlic_text_lines: the line index of the device text text_ptr[0, text_bytes), as SlabLines::take gives it.  capacity
    None: asked for with a first call without room (GARLIC_ERR_RANGE reports the count); a number: that much room, and
    the GarlicError (ERR_RANGE) when the slab holds more.  Returns a dict: begin, end, number (int64 [n_lines]), heads
    (uint8 [n_lines][head_bytes], None without head_bytes), consumed, seen."""
    n, consumed, seen_out = C.c_int64(), C.c_int64(), C.c_int64()

    def call(cap):
        begin, end, number = (np.zeros(cap, dtype=np.int64) for _ in range(3))
        heads = np.zeros((cap, head_bytes), dtype=np.uint8) if head_bytes else None
        rc = lib().garlic_text_lines(ctx.handle, _vp(text_ptr), int(text_bytes), int(bool(last)), int(seen), int(head_bytes), cap,
                                     _ptr(begin, _i64p), _ptr(end, _i64p), _ptr(number, _i64p),
                                     _vp(heads.ctypes.data) if head_bytes and cap else None, C.byref(n), C.byref(consumed), C.byref(seen_out))
        return rc, begin, end, number, heads

    rc, begin, end, number, heads = call(0 if capacity is None else int(capacity))
    if rc == ERR_RANGE and capacity is None:
        rc, begin, end, number, heads = call(n.value)
    check(rc)
    k = n.value
    return {"begin": begin[:k], "end": end[:k], "number": number[:k], "heads": None if heads is None else heads[:k],
            "consumed": consumed.value, "seen": seen_out.value}


class Bed:
    """The SNP-major image of a PLINK .bed file on a context's device (garlic_bed): nrows rows of (nind_total + 3) // 4
    bytes in PLINK's 2-bit codes."""

    def __init__(self, ctx, nrows, nind_total):
        self.ctx = ctx
        self.nrows = int(nrows)
        self.nind_total = int(nind_total)
        self.row_bytes = (self.nind_total + 3) // 4
        self.handle = _vp()
        check(lib().garlic_bed_create(ctx.handle, self.nrows, self.nind_total, C.byref(self.handle)))

    @classmethod
    def create(cls, ctx, nrows, nind_total):
        return cls(ctx, nrows, nind_total)

    def set_rows(self, rows, row_begin=0):
        """rows: uint8 [row_count][row_bytes >= (nind_total + 3) // 4] (host)."""
        rows = np.asarray(rows)
        assert rows.dtype == np.uint8 and rows.ndim == 2 and (rows.shape[1] == 1 or rows.strides[1] == 1)
        check(lib().garlic_bed_set_rows(self.handle, _vp(rows.ctypes.data), rows.strides[0], row_begin, rows.shape[0], HOST))

    def set_rows_device(self, ptr, row_bytes, row_begin, row_count):
        """ptr: device address of row_count rows, row_bytes apart."""
        check(lib().garlic_bed_set_rows(self.handle, _vp(ptr), row_bytes, row_begin, row_count, DEVICE))

    def census(self):
        """(counts int32 [nrows][2] = nalleles, total; counted uint8 [nrows] = 0 A1, 1 A2, 2 none)."""
        counts = np.empty((self.nrows, 2), dtype=np.int32)
        counted = np.empty(self.nrows, dtype=np.uint8)
        check(lib().garlic_bed_census(self.handle, _vp(counts.ctypes.data), _vp(counted.ctypes.data), HOST))
        return counts, counted

    def census_device(self, counts_ptr, counted_ptr):
        check(lib().garlic_bed_census(self.handle, _vp(counts_ptr), _vp(counted_ptr), DEVICE))

    def extract(self, idx):
        """A new Bed on the same context whose individual i is this image's individual idx[i] (any order, repeats allowed):
        one population of a multi-population file.  Independent of this image once made; it needs the context."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        assert idx.ndim == 1
        handle = _vp()
        check(lib().garlic_bed_extract(self.handle, _vp(idx.ctypes.data), idx.shape[0], C.byref(handle)))
        sub = object.__new__(Bed)
        sub.ctx = self.ctx
        sub.nrows = self.nrows
        sub.nind_total = int(idx.shape[0])
        sub.row_bytes = (sub.nind_total + 3) // 4
        sub.handle = handle
        return sub

    def get_rows(self, row_begin=0, row_count=None):
        """uint8 [row_count][(nind_total + 3) // 4]: the image's rows as they stand on the device."""
        row_count = self.nrows - row_begin if row_count is None else row_count
        rows = np.empty((max(row_count, 0), self.row_bytes), dtype=np.uint8)
        check(lib().garlic_bed_get_rows(self.handle, row_begin, row_count, _vp(rows.ctypes.data), self.row_bytes, HOST))
        return rows

    @property
    def order_row_bytes(self):
        return (self.nind_total + 7) // 8

    def set_order_rows(self, rows, row_begin=0):
        """rows: uint8 [row_count][row_bytes >= (nind_total + 7) // 8] (host): the order plane, bit i & 7 of byte i >> 3 of a
        row = "the first allele of individual i's genotype is A2"."""
        rows = np.asarray(rows)
        assert rows.dtype == np.uint8 and rows.ndim == 2 and (rows.shape[1] == 1 or rows.strides[1] == 1)
        check(lib().garlic_bed_set_order_rows(self.handle, _vp(rows.ctypes.data), rows.strides[0], row_begin, rows.shape[0], HOST))

    def set_order_rows_device(self, ptr, row_bytes, row_begin, row_count):
        check(lib().garlic_bed_set_order_rows(self.handle, _vp(ptr), row_bytes, row_begin, row_count, DEVICE))

    def get_order_rows(self, row_begin=0, row_count=None):
        """uint8 [row_count][(nind_total + 7) // 8]: the order plane's rows as they stand on the device."""
        row_count = self.nrows - row_begin if row_count is None else row_count
        rows = np.empty((max(row_count, 0), self.order_row_bytes), dtype=np.uint8)
        check(lib().garlic_bed_get_order_rows(self.handle, row_begin, row_count, _vp(rows.ctypes.data), self.order_row_bytes, HOST))
        return rows

    def set_rows_vcf(self, text, line_begin, row_begin=0, text_bytes=None, where=HOST):
        """Image and order rows [row_begin, row_begin + len(line_begin) - 1) parsed from VCF text on the device
        (garlic_bed_set_rows_vcf).  text: bytes / uint8 array (host), or a device address with text_bytes and where=DEVICE.
        Returns (status int32 [rows][2] = code, sample column; error or None): an offence fills the status and comes back as
        the GarlicError instead of being raised, so that a caller sees both."""
        lb = np.ascontiguousarray(line_begin, dtype=np.int64)
        assert lb.ndim == 1 and lb.shape[0] >= 2
        if where == HOST:
            buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text)
            assert buf.dtype == np.uint8 and buf.ndim == 1 and (buf.shape[0] <= 1 or buf.strides[0] == 1)
            ptr, text_bytes = buf.ctypes.data, buf.shape[0] if text_bytes is None else text_bytes
        else:
            ptr = int(text)
        status = np.zeros((lb.shape[0] - 1, 2), dtype=np.int32)
        rc = lib().garlic_bed_set_rows_vcf(self.handle, _vp(ptr), int(text_bytes), _ptr(lb, _i64p), row_begin, lb.shape[0] - 1,
                                           _vp(status.ctypes.data), where)
        err = None
        if rc != OK:
            err = GarlicError(rc, lib().garlic_hip_last_error().decode())
            if rc != ERR_INVALID or not status[:, 0].any():
                raise err
        return status, err

    def set_rows_tped(self, text, line_begin, row_begin=0, missing=b"0", text_bytes=None, where=HOST):
        """Image rows, order rows and census of rows [row_begin, row_begin + len(line_begin) - 1) parsed from TPED text on the
        device (garlic_bed_set_rows_tped).  text: bytes / uint8 array (host), or a device address with text_bytes and
        where=DEVICE; missing: the --tped-missing character (one byte, or its value).
        Returns (row_allele uint8 [rows], row_status int32 [rows][2] = code, individual).  An offending line raises the
        GarlicError (ERR_INVALID) with both arrays as its row_allele / row_status attributes: the clean rows are written."""
        lb = np.ascontiguousarray(line_begin, dtype=np.int64)
        assert lb.ndim == 1 and lb.shape[0] >= 2
        if where == HOST:
            buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text)
            assert buf.dtype == np.uint8 and buf.ndim == 1 and (buf.shape[0] <= 1 or buf.strides[0] == 1)
            ptr, text_bytes = buf.ctypes.data, buf.shape[0] if text_bytes is None else text_bytes
        else:
            ptr = int(text)
        miss = missing[0] if isinstance(missing, (bytes, bytearray)) else ord(missing) if isinstance(missing, str) else int(missing)
        status = np.zeros((lb.shape[0] - 1, 2), dtype=np.int32)
        allele = np.zeros(lb.shape[0] - 1, dtype=np.uint8)
        rc = lib().garlic_bed_set_rows_tped(self.handle, _vp(ptr), int(text_bytes), _ptr(lb, _i64p), row_begin, lb.shape[0] - 1, miss,
                                            _vp(allele.ctypes.data), _vp(status.ctypes.data), where)
        if rc != OK:
            err = GarlicError(rc, lib().garlic_hip_last_error().decode())
            err.row_allele, err.row_status = allele, status
            raise err
        return allele, status

    def set_census(self, counts, counted):
        """The census the image's source computed (garlic_bed_set_census): counts int32 [nrows][2], counted uint8 [nrows]."""
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        counted = np.ascontiguousarray(counted, dtype=np.uint8)
        assert counts.shape == (self.nrows, 2) and counted.shape == (self.nrows,)
        check(lib().garlic_bed_set_census(self.handle, _vp(counts.ctypes.data), _vp(counted.ctypes.data), HOST))

    def destroy(self):
        if self.handle:
            lib().garlic_bed_destroy(self.handle)
            self.handle = _vp()

    close = destroy

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()


class Tgls:
    """The likelihoods of a --tgls file on a context's device (garlic_tgls): nrows rows of uint16 codes into one dictionary of
    the raw values, parsed from the text on the device.  col_idx: the sample columns kept, in the order kept (None = all)."""

    def __init__(self, ctx, nrows, ncols_total, col_idx=None):
        self.ctx = ctx
        self.nrows = int(nrows)
        self.ncols_total = int(ncols_total)
        idx = None if col_idx is None else np.ascontiguousarray(col_idx, dtype=np.int32)
        self.n_kept = self.ncols_total if idx is None else int(idx.shape[0])
        self.handle = _vp()
        check(lib().garlic_tgls_create(ctx.handle, self.nrows, self.ncols_total, None if idx is None else _ptr(idx, _i32p),
                                       0 if idx is None else idx.shape[0], C.byref(self.handle)))

    def set_rows_text(self, text, line_begin, row_begin=0, text_bytes=None, where=HOST):
        """Rows [row_begin, row_begin + len(line_begin) - 1) parsed from text on the device (garlic_tgls_set_rows_text).  text:
        bytes / uint8 array (host), or a device address with text_bytes and where=DEVICE.  Returns (status int32 [rows][2] =
        code, sample column; error or None): a column-count offence fills the status and comes back as the GarlicError
        instead of being raised, so that a caller sees both.  A deferred row is no error."""
        lb = np.ascontiguousarray(line_begin, dtype=np.int64)
        assert lb.ndim == 1 and lb.shape[0] >= 2
        if where == HOST:
            buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text)
            assert buf.dtype == np.uint8 and buf.ndim == 1 and (buf.shape[0] <= 1 or buf.strides[0] == 1)
            ptr, text_bytes = buf.ctypes.data, buf.shape[0] if text_bytes is None else text_bytes
        else:
            ptr = int(text)
        status = np.zeros((lb.shape[0] - 1, 2), dtype=np.int32)
        rc = lib().garlic_tgls_set_rows_text(self.handle, _vp(ptr), int(text_bytes), _ptr(lb, _i64p), row_begin, lb.shape[0] - 1,
                                             _vp(status.ctypes.data), where)
        err = None
        if rc != OK:
            err = GarlicError(rc, lib().garlic_hip_last_error().decode())
            if rc != ERR_INVALID or not (status[:, 0] >= TGLS_FEW_COLUMNS).any():
                raise err
        return status, err

    def set_rows_vcf(self, text, line_begin, key, missing_raw=None, row_begin=0, text_bytes=None, where=HOST):
        """The same rows from the data lines of a VCF (garlic_tgls_set_rows_vcf): the FORMAT subfield `key` (str or bytes) of
        every sample column.  missing_raw: the raw value a called genotype without a value takes (None: such a line is
        refused).  text, line_begin, the return value and the errors as for set_rows_text."""
        lb = np.ascontiguousarray(line_begin, dtype=np.int64)
        assert lb.ndim == 1 and lb.shape[0] >= 2
        if where == HOST:
            buf = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.asarray(text)
            assert buf.dtype == np.uint8 and buf.ndim == 1 and (buf.shape[0] <= 1 or buf.strides[0] == 1)
            ptr, text_bytes = buf.ctypes.data, buf.shape[0] if text_bytes is None else text_bytes
        else:
            ptr = int(text)
        status = np.zeros((lb.shape[0] - 1, 2), dtype=np.int32)
        miss = None if missing_raw is None else C.byref(C.c_double(float(missing_raw)))
        rc = lib().garlic_tgls_set_rows_vcf(self.handle, _vp(ptr), int(text_bytes), _ptr(lb, _i64p), row_begin, lb.shape[0] - 1,
                                            key.encode() if isinstance(key, str) else bytes(key),
                                            None if miss is None else C.cast(miss, _f64p), _vp(status.ctypes.data), where)
        err = None
        if rc != OK:
            err = GarlicError(rc, lib().garlic_hip_last_error().decode())
            if rc != ERR_INVALID or not (status[:, 0] >= TGLS_FEW_COLUMNS).any():
                raise err
        return status, err

    def set_rows_values(self, raw, row_begin=0):
        """raw: float64 [row_count][n_kept] (host): the rows' raw values as the host parses them."""
        raw = np.ascontiguousarray(raw, dtype=np.float64)
        assert raw.ndim == 2 and raw.shape[1] == self.n_kept
        check(lib().garlic_tgls_set_rows_values(self.handle, _vp(raw.ctypes.data), raw.shape[1], row_begin, raw.shape[0], HOST))

    def get_rows(self, gl_type=TGLS_RAW, row_begin=0, row_count=None):
        """float64 [row_count][n_kept]: the rows' values, raw (TGLS_RAW) or converted (GL_GQ / GL_GL / GL_PL)."""
        row_count = self.nrows - row_begin if row_count is None else row_count
        out = np.empty((max(row_count, 0), self.n_kept), dtype=np.float64)
        check(lib().garlic_tgls_get_rows(self.handle, gl_type, row_begin, row_count, _vp(out.ctypes.data), self.n_kept, HOST))
        return out

    def info(self):
        """(distinct raw values, rows set, rows deferred)"""
        n, rs, rd = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        check(lib().garlic_tgls_info(self.handle, C.byref(n), C.byref(rs), C.byref(rd)))
        return n.value, rs.value, rd.value

    def count_values(self, gl_type=TGLS_RAW, row_begin=0, row_count=None):
        """the number of distinct values, raw or converted, among the rows of the range"""
        n = C.c_int32(0)
        row_count = self.nrows - row_begin if row_count is None else row_count
        check(lib().garlic_tgls_count_values(self.handle, gl_type, row_begin, row_count, C.byref(n)))
        return n.value

    def values(self, gl_type=TGLS_RAW):
        """float64 [n_raw_values]: the dictionary in the order its codes were issued, raw or converted"""
        out = np.empty(self.info()[0], dtype=np.float64)
        check(lib().garlic_tgls_get_values(self.handle, gl_type, _ptr(out, _f64p), out.shape[0]))
        return out

    def destroy(self):
        if self.handle:
            lib().garlic_tgls_destroy(self.handle)
            self.handle = _vp()

    close = destroy

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()


class Panel:
    """Device-resident genotype panel (garlic_panel) for the individuals one context owns."""

    def __init__(self, ctx, chr_nloci, nind):
        self.ctx = ctx
        self.chr_nloci = np.ascontiguousarray(chr_nloci, dtype=np.int32)
        self.nchr = int(self.chr_nloci.shape[0])
        self.nloci = int(self.chr_nloci.sum())
        self.nind = int(nind)
        self.handle = _vp()
        check(lib().garlic_panel_create(ctx.handle, self.nchr, _ptr(self.chr_nloci, _i32p), self.nind,
                                        C.byref(self.handle)))

    def close(self):
        if self.handle:
            lib().garlic_panel_destroy(self.handle)
            self.handle = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_map(self, pos, centro_start, centro_end, gpos=None):
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        cs = np.ascontiguousarray(centro_start, dtype=np.int32)
        ce = np.ascontiguousarray(centro_end, dtype=np.int32)
        assert pos.shape[0] == self.nloci and cs.shape[0] == self.nchr and ce.shape[0] == self.nchr
        if gpos is not None:
            gpos = np.ascontiguousarray(gpos, dtype=np.float64)
            assert gpos.shape[0] == self.nloci
        check(lib().garlic_panel_set_map(self.handle, _ptr(pos, _i32p), _ptr(gpos, _f64p),
                                         _ptr(cs, _i32p), _ptr(ce, _i32p)))

    def set_freq(self, freq):
        freq = np.ascontiguousarray(freq, dtype=np.float64)
        assert freq.shape[0] == self.nloci
        check(lib().garlic_panel_set_freq(self.handle, _ptr(freq, _f64p)))

    def set_genotypes(self, geno, locus_begin=0):
        """geno: int16 numpy array [nloci_chunk][>= nind] (host)."""
        geno = np.asarray(geno)
        assert geno.dtype == np.int16 and geno.ndim == 2 and geno.strides[1] == 2
        ld = geno.strides[0] // 2
        check(lib().garlic_panel_set_genotypes(self.handle, _vp(geno.ctypes.data), ld, locus_begin,
                                               geno.shape[0], HOST))

    def set_genotypes_device(self, ptr, ld, locus_begin, locus_count):
        """ptr: device address of int16 [locus_count][ld] (e.g. torch tensor .data_ptr())."""
        check(lib().garlic_panel_set_genotypes(self.handle, _vp(ptr), ld, locus_begin, locus_count,
                                               DEVICE))

    def set_gl(self, gl, locus_begin=0):
        """gl: float64 numpy array [nloci_chunk][>= nind]: per-genotype error probabilities (TGLS)."""
        gl = np.asarray(gl)
        assert gl.dtype == np.float64 and gl.ndim == 2 and gl.strides[1] == 8
        check(lib().garlic_panel_set_gl(self.handle, _vp(gl.ctypes.data), gl.strides[0] // 8, locus_begin,
                                        gl.shape[0], HOST))

    def set_genotypes_2bit(self, rows, ind_offset=0, locus_begin=0):
        """rows: uint8 [nloci_chunk][row_bytes], 4 genotypes per byte (3 = missing), individuals of the
        whole data set; this panel's individuals start at ind_offset."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        assert rows.ndim == 2
        check(lib().garlic_panel_set_genotypes_2bit(self.handle, _vp(rows.ctypes.data), rows.shape[1], ind_offset,
                                                    locus_begin, rows.shape[0], HOST))

    def set_genotypes_bed(self, bed, dest_locus, ind_offset=0):
        """The rows of a Bed image recoded into the panel: dest_locus[r] = global locus of file row r, -1 = dropped; this
        panel's individuals start at ind_offset of the row."""
        dest = np.ascontiguousarray(dest_locus, dtype=np.int64)
        assert dest.shape == (bed.nrows,)
        check(lib().garlic_panel_set_genotypes_bed(self.handle, bed.handle, ind_offset, _ptr(dest, _i64p)))

    def set_phase_bed(self, bed, dest_locus, ind_offset=0):
        """HapData::firstCopy from a Bed image with an order plane, device to device; arguments as set_genotypes_bed."""
        dest = np.ascontiguousarray(dest_locus, dtype=np.int64)
        assert dest.shape == (bed.nrows,)
        check(lib().garlic_panel_set_phase_bed(self.handle, bed.handle, ind_offset, _ptr(dest, _i64p)))

    def set_gl_tgls(self, tgls, gl_type, dest_locus, ind_offset=0):
        """The likelihoods from a Tgls object, device to device (garlic_panel_set_gl_tgls): row r of the object goes to locus
        dest_locus[r] (-1 = dropped, the others strictly ascending); the panel's individual i is kept column ind_offset + i."""
        dest = np.ascontiguousarray(dest_locus, dtype=np.int64)
        assert dest.shape == (tgls.nrows,)
        check(lib().garlic_panel_set_gl_tgls(self.handle, tgls.handle, gl_type, ind_offset, _ptr(dest, _i64p)))

    def set_gl_codes(self, codes, values, locus_begin=0):
        """codes: uint8 [nloci_chunk][nind] indexing values (float64, <= 256 error probabilities)"""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        values = np.ascontiguousarray(values, dtype=np.float64)
        check(lib().garlic_panel_set_gl_codes(self.handle, _vp(codes.ctypes.data), codes.shape[1], locus_begin,
                                              codes.shape[0], _vp(values.ctypes.data), values.shape[0], HOST))

    def set_gl_codes16(self, codes, values, locus_begin=0):
        """codes: uint16 [nloci_chunk][nind] indexing values (float64, <= 65536 error probabilities); the panel keeps
        2 bytes per genotype (TGLS_DICTIONARY16)"""
        codes = np.ascontiguousarray(codes, dtype=np.uint16)
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert codes.ndim == 2 and values.ndim == 1
        check(lib().garlic_panel_set_gl_codes16(self.handle, _vp(codes.ctypes.data), codes.shape[1], locus_begin,
                                                codes.shape[0], _vp(values.ctypes.data), values.shape[0], HOST))

    feed_order = FEED_ORDER_REFERENCE   # what set_feed_order set last (the library has no getter)

    def set_feed_order(self, order):
        """garlic_panel_set_feed_order: FEED_ORDER_REFERENCE (chromosome -> individual -> locus, the default) or
        FEED_ORDER_SORTED (every feed call returns its values ascending, sorted on the device)"""
        check(lib().garlic_panel_set_feed_order(self.handle, int(order)))
        self.feed_order = int(order)

    def release_scratch(self):
        """free the device scratch the panel keeps between calls (LD buffers, score / feed scratch)"""
        check(lib().garlic_panel_release_scratch(self.handle))

    def set_phase(self, first_copy, locus_begin=0):
        """first_copy: uint8/bool [nloci_chunk][nind], HapData::firstCopy (--phased)."""
        fc = np.ascontiguousarray(first_copy).view(np.uint8) if np.asarray(first_copy).dtype == np.bool_ \
            else np.ascontiguousarray(first_copy, dtype=np.uint8)
        assert fc.ndim == 2 and fc.shape[1] >= self.nind
        check(lib().garlic_panel_set_phase(self.handle, _vp(fc.ctypes.data), fc.shape[1], locus_begin,
                                           fc.shape[0], HOST))

    def set_phase_bits(self, rows, locus_begin=0):
        """rows: uint8 [nloci_chunk][row_bytes], HapData::firstCopy at one bit per genotype -- bit i & 7 of byte i >> 3 of a
        row is individual i (np.packbits(first_copy, axis=1, bitorder="little")); row_bytes >= (nind + 7) / 8."""
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        assert rows.ndim == 2
        check(lib().garlic_panel_set_phase_bits(self.handle, _vp(rows.ctypes.data), rows.shape[1], locus_begin, rows.shape[0], HOST))

    def set_phase_bits_device(self, ptr, row_bytes, locus_begin, locus_count):
        """ptr: device address of such rows"""
        check(lib().garlic_panel_set_phase_bits(self.handle, _vp(ptr), row_bytes, locus_begin, locus_count, DEVICE))

    def ld_form_info(self):
        """(pair kernel LD_PAIR_*, sum kernel LD_SUM_*, fused, phased) of the panel's last LD call"""
        v = [C.c_int32() for _ in range(4)]
        check(lib().garlic_panel_ld_form_info(self.handle, *[C.byref(x) for x in v]))
        return v[0].value, v[1].value, bool(v[2].value), bool(v[3].value)

    def set_gl_device(self, ptr, ld, locus_begin, locus_count):
        """ptr: device address of float64 [locus_count][ld] per-genotype error probabilities."""
        check(lib().garlic_panel_set_gl(self.handle, _vp(ptr), ld, locus_begin, locus_count, DEVICE))

    def set_ld_device(self, winsize, ptr):
        """ptr: device address of float64 [nloci][winsize] LD weights."""
        check(lib().garlic_panel_set_ld(self.handle, winsize, _vp(ptr), DEVICE))

    def wlod_windows_device(self, out_ptr, winsize, error, max_gap, M, mu, ind_begin=0, ind_count=None,
                            pitch_align=32, use_gl=False):
        ind_count = self.nind - ind_begin if ind_count is None else ind_count
        check(lib().garlic_wlod_windows(self.handle, winsize, error, max_gap, int(use_gl), M, mu, ind_begin,
                                        ind_count, pitch_align, _vp(out_ptr), DEVICE))

    def set_ld(self, winsize, ld):
        """ld: float64 [nloci][winsize] LD weights of wLOD (all chromosomes concatenated)."""
        ld = np.ascontiguousarray(ld, dtype=np.float64)
        assert ld.shape == (self.nloci, winsize)
        check(lib().garlic_panel_set_ld(self.handle, winsize, _vp(ld.ctypes.data), HOST))

    @staticmethod
    def _sub(sub_idx):
        """None = every individual; an array = exactly those, an EMPTY array = none of them (a shard
        that holds no member of a panel-wide subsample): the pointer must then still be non-NULL"""
        if sub_idx is None:
            return None, 0
        sub = np.ascontiguousarray(sub_idx, dtype=np.int32)
        n = int(sub.shape[0])
        if n == 0:
            sub = np.zeros(1, dtype=np.int32)
        return sub, n

    def compute_ld(self, winsize, sub_idx=None, want_output=True, phased=False):
        """calcHR2LD (phased: calcR2LD) on the device (sub_idx: the --ld-subsample individuals,
        None = all); installs the weights for wlod_windows and returns them as float64
        [nloci][winsize]."""
        sub, n = self._sub(sub_idx)
        out = np.empty((self.nloci, winsize), dtype=np.float64) if want_output else None
        check(lib().garlic_panel_compute_ld(self.handle, winsize, int(phased), _ptr(sub, _i32p), n,
                                            _vp(out.ctypes.data) if want_output else None, HOST))
        return out

    def ld_counts(self, winsize, sub_idx=None, phased=False):
        """Integer part of the LD weights for this shard's individuals: (locus_counts [nloci][2],
        pair_counts [nloci][winsize][2]) int32; sum over shards, then ld_finish."""
        sub, n = self._sub(sub_idx)
        loc = np.empty((self.nloci, 2), dtype=np.int32)
        pair = np.empty((self.nloci, winsize, 2), dtype=np.int32)
        check(lib().garlic_ld_counts(self.handle, winsize, int(phased), _ptr(sub, _i32p), n, _vp(loc.ctypes.data),
                                     _vp(pair.ctypes.data), HOST))
        return loc, pair

    def ld_finish(self, winsize, locus_counts, pair_counts, want_output=True, phased=False):
        loc = np.ascontiguousarray(locus_counts, dtype=np.int32)
        pair = np.ascontiguousarray(pair_counts, dtype=np.int32)
        assert loc.shape == (self.nloci, 2) and pair.shape == (self.nloci, winsize, 2)
        out = np.empty((self.nloci, winsize), dtype=np.float64) if want_output else None
        check(lib().garlic_ld_finish(self.handle, winsize, int(phased), _vp(loc.ctypes.data), _vp(pair.ctypes.data),
                                     _vp(out.ctypes.data) if want_output else None, HOST))
        return out

    def _ld_multi_outs(self, winsizes, want_output):
        """want_output: True / False for every size, or one flag per listed size"""
        sizes = np.ascontiguousarray(winsizes, dtype=np.int32)
        want = [bool(want_output)] * len(sizes) if isinstance(want_output, (bool, np.bool_)) else [bool(w) for w in want_output]
        assert len(want) == len(sizes)
        outs = [np.empty((self.nloci, int(w)), dtype=np.float64) if k else None for w, k in zip(sizes, want)]
        ptrs = (_vp * len(sizes))(*[o.ctypes.data if o is not None else None for o in outs])
        return sizes, outs, (ptrs if any(want) else None)

    def compute_ld_multi(self, winsizes, sub_idx=None, want_output=True, phased=False):
        """The LD weights of every listed window size from shared passes; installs them all.  Returns one float64
        [nloci][winsize] per listed size (None where no output was wanted)."""
        sub, n = self._sub(sub_idx)
        sizes, outs, ptrs = self._ld_multi_outs(winsizes, want_output)
        check(lib().garlic_panel_compute_ld_multi(self.handle, _ptr(sizes, _i32p), len(sizes), int(phased), _ptr(sub, _i32p), n,
                                                  ptrs, HOST))
        return outs

    def ld_finish_multi(self, winsizes, locus_counts, pair_counts, want_output=True, phased=False):
        """pair_counts: those of ld_counts(max(winsizes)), summed over the shards"""
        sizes, outs, ptrs = self._ld_multi_outs(winsizes, want_output)
        loc = np.ascontiguousarray(locus_counts, dtype=np.int32)
        pair = np.ascontiguousarray(pair_counts, dtype=np.int32)
        assert loc.shape == (self.nloci, 2) and pair.shape == (self.nloci, int(sizes.max()), 2)
        check(lib().garlic_ld_finish_multi(self.handle, _ptr(sizes, _i32p), len(sizes), int(phased), _vp(loc.ctypes.data),
                                           _vp(pair.ctypes.data), ptrs, HOST))
        return outs

    def ld_info(self, cap=64):
        """(installed winsizes ascending, their group of the last multi call, bytes held by the sets, pair stages, sum passes)"""
        w = np.zeros(cap, dtype=np.int32)
        g = np.zeros(cap, dtype=np.int32)
        n, npair, nsum = C.c_int32(), C.c_int32(), C.c_int32()
        nbytes = C.c_int64()
        check(lib().garlic_panel_ld_info(self.handle, cap, _ptr(w, _i32p), _ptr(g, _i32p), C.byref(n), C.byref(nbytes),
                                         C.byref(npair), C.byref(nsum)))
        k = min(n.value, cap)
        return [int(x) for x in w[:k]], [int(x) for x in g[:k]], nbytes.value, npair.value, nsum.value

    def ld_counts_device(self, winsize, locus_ptr, pair_ptr, sub_idx=None, phased=False):
        sub, n = self._sub(sub_idx)
        check(lib().garlic_ld_counts(self.handle, winsize, int(phased), _ptr(sub, _i32p), n, _vp(locus_ptr),
                                     _vp(pair_ptr), DEVICE))

    def ld_finish_device(self, winsize, locus_ptr, pair_ptr, ld_ptr=None, phased=False):
        check(lib().garlic_ld_finish(self.handle, winsize, int(phased), _vp(locus_ptr), _vp(pair_ptr),
                                     _vp(ld_ptr) if ld_ptr else None, DEVICE))

    def out_layout(self, pitch_align=1, nind_out=None):
        nind_out = self.nind if nind_out is None else nind_out
        base = np.empty(self.nchr, dtype=np.int64)
        pitch = np.empty(self.nchr, dtype=np.int64)
        total = C.c_int64()
        check(lib().garlic_lod_out_layout(self.handle, pitch_align, nind_out, _ptr(base, _i64p),
                                          _ptr(pitch, _i64p), C.byref(total)))
        return base, pitch, total.value

    def lod_windows(self, winsize, error, max_gap, ind_begin=0, ind_count=None, pitch_align=1,
                    use_gl=False):
        """Host-output convenience: returns a list of per-chromosome [ind_count][nloci_c] arrays."""
        ind_count = self.nind - ind_begin if ind_count is None else ind_count
        base, pitch, total = self.out_layout(pitch_align, ind_count)
        out = np.empty(total, dtype=np.float64)
        check(lib().garlic_lod_windows(self.handle, winsize, error, max_gap, int(use_gl), ind_begin,
                                       ind_count, pitch_align, _vp(out.ctypes.data), HOST))
        res = []
        for c in range(self.nchr):
            n = int(self.chr_nloci[c])
            blk = out[base[c]: base[c] + ind_count * pitch[c]].reshape(ind_count, pitch[c])
            res.append(blk[:, :n])
        return res

    def wlod_windows(self, winsize, error, max_gap, M, mu, ind_begin=0, ind_count=None, pitch_align=1,
                     use_gl=False):
        ind_count = self.nind - ind_begin if ind_count is None else ind_count
        base, pitch, total = self.out_layout(pitch_align, ind_count)
        out = np.empty(total, dtype=np.float64)
        check(lib().garlic_wlod_windows(self.handle, winsize, error, max_gap, int(use_gl), M, mu, ind_begin,
                                        ind_count, pitch_align, _vp(out.ctypes.data), HOST))
        res = []
        for c in range(self.nchr):
            n = int(self.chr_nloci[c])
            blk = out[base[c]: base[c] + ind_count * pitch[c]].reshape(ind_count, pitch[c])
            res.append(blk[:, :n])
        return res

    def lod_windows_multi(self, winsizes, error, max_gap, pitch_align=1, use_gl=False):
        """Host-output convenience for several window sizes: {W: [per-chromosome [nind][nloci_c] arrays]}."""
        ws = np.ascontiguousarray(winsizes, dtype=np.int32)
        base, pitch, total = self.out_layout(pitch_align, self.nind)
        out = np.empty((len(ws), total), dtype=np.float64)
        check(lib().garlic_lod_windows_multi(self.handle, _ptr(ws, _i32p), len(ws), error, max_gap, int(use_gl), 0,
                                             self.nind, pitch_align, _vp(out.ctypes.data), total, HOST))
        res = {}
        for k, W in enumerate(ws):
            res[int(W)] = [out[k, base[c]: base[c] + self.nind * pitch[c]].reshape(self.nind, pitch[c])[:, :int(self.chr_nloci[c])]
                           for c in range(self.nchr)]
        return res

    def lod_windows_device(self, out_ptr, winsize, error, max_gap, ind_begin=0, ind_count=None,
                           pitch_align=32, use_gl=False):
        ind_count = self.nind - ind_begin if ind_count is None else ind_count
        check(lib().garlic_lod_windows(self.handle, winsize, error, max_gap, int(use_gl), ind_begin,
                                       ind_count, pitch_align, _vp(out_ptr), DEVICE))

    def flatten_device(self, scores_ptr, step, feed_ptr, feed_capacity, pitch_align=32, nind_out=None):
        """KDE feed (convertWinData2DoubleData) of device-resident scores; returns the count."""
        nind_out = self.nind if nind_out is None else nind_out
        n = C.c_int64()
        check(lib().garlic_lod_flatten(self.handle, _vp(scores_ptr), pitch_align, nind_out, step,
                                       _vp(feed_ptr) if feed_ptr else None, feed_capacity, C.byref(n)))
        return n.value

    def lod_feed(self, winsize, error, max_gap, step, use_gl=False, weighted=False, M=7, mu=1e-9, copy=True,
                 ind_idx=None):
        """scores + thinning on the device: returns (feed float64 [count], per-chromosome counts).
        copy=False: the feed is a view of a buffer the panel object reuses for the next call.
        ind_idx: only these individuals, in this order (convertSubsetWinData2DoubleData, --kde-subsample)"""
        idx = None if ind_idx is None else np.ascontiguousarray(ind_idx, dtype=np.int32)
        n_rows = self.nind if idx is None else int(idx.shape[0])
        cap = int(sum((int(n) + step - 1) // step for n in self.chr_nloci)) * n_rows
        if copy:
            feed = np.empty(max(cap, 1), dtype=np.float64)
        else:
            if getattr(self, "_feed_buf", None) is None or self._feed_buf.shape[0] < max(cap, 1):
                self._feed_buf = np.empty(max(cap, 1), dtype=np.float64)
            feed = self._feed_buf
        n = C.c_int64()
        per_chr = np.zeros(self.nchr, dtype=np.int64)
        check(lib().garlic_lod_feed_subset(self.handle, winsize, error, max_gap, int(use_gl), int(weighted), M, mu,
                                           step, _ptr(idx, _i32p), 0 if idx is None else n_rows,
                                           _vp(feed.ctypes.data), cap, C.byref(n), _ptr(per_chr, _i64p)))
        return (feed[: n.value].copy() if copy else feed[: n.value]), per_chr

    def lod_kde(self, winsize, error, max_gap, step, use_gl=False, weighted=False, M=7, mu=1e-9, ind_idx=None):
        """garlic_lod_kde: lod_feed's arguments; the feed is sorted and reduced to its KDE on the device.  Returns
        (the dict of Context.feed_kde, per-chromosome counts)."""
        idx = None if ind_idx is None else np.ascontiguousarray(ind_idx, dtype=np.int32)
        k = Kde()
        per_chr = np.zeros(self.nchr, dtype=np.int64)
        check(lib().garlic_lod_kde(self.handle, winsize, error, max_gap, int(use_gl), int(weighted), M, mu, step,
                                   _ptr(idx, _i32p), 0 if idx is None else int(idx.shape[0]), C.byref(k), _ptr(per_chr, _i64p)))
        return k.as_dict(), per_chr

    def lod_kde_multi(self, winsizes, error, max_gap, steps=None, use_gl=False, ind_idx=None, strict=False, outs=None):
        """garlic_lod_kde_multi: the KDEs of several window sizes' feeds in one call (unweighted scores; steps default to the
        window sizes).  Returns ([lod_kde's dict, or None for a refused size], [status per size], per-chromosome counts
        [n_sizes, nchr]).  strict and outs as Context.feed_kde_multi."""
        sizes = np.ascontiguousarray(winsizes, dtype=np.int32)
        st = sizes.copy() if steps is None else np.ascontiguousarray(steps, dtype=np.int32)
        idx = None if ind_idx is None else np.ascontiguousarray(ind_idx, dtype=np.int32)
        m = int(sizes.shape[0])
        per_chr = np.zeros((max(m, 1), self.nchr), dtype=np.int64)
        got = _kde_multi_result(lambda ks, status: lib().garlic_lod_kde_multi(
            self.handle, _ptr(sizes, _i32p), _ptr(st, _i32p), m, error, max_gap, int(use_gl), _ptr(idx, _i32p),
            0 if idx is None else int(idx.shape[0]), ks, status, _ptr(per_chr, _i64p)), m, strict, outs)
        return got + (per_chr[:m],)

    def lod_kde_part(self, winsize, error, max_gap, step, use_gl=False, weighted=False, M=7, mu=1e-9, ind_idx=None):
        """garlic_lod_kde_part: lod_kde's arguments; the sorted device feed becomes an abi.KdePart that borrows the panel's
        scratch (stale after the panel's next score or feed call).  Returns (the part, per-chromosome counts)."""
        idx = None if ind_idx is None else np.ascontiguousarray(ind_idx, dtype=np.int32)
        h = _vp()
        per_chr = np.zeros(self.nchr, dtype=np.int64)
        check(lib().garlic_lod_kde_part(self.handle, winsize, error, max_gap, int(use_gl), int(weighted), M, mu, step,
                                        _ptr(idx, _i32p), 0 if idx is None else int(idx.shape[0]), C.byref(h), _ptr(per_chr, _i64p)))
        return KdePart(h), per_chr

    def lod_kde_part_set(self, winsizes, error, max_gap, steps=None, use_gl=False, ind_idx=None):
        """garlic_lod_kde_part_set: lod_kde_multi's arguments; the sizes' sorted device feeds become an abi.KdePartSet that
        borrows the panel's feed slots (stale after the panel's next score or feed call).  Returns (the set, per-chromosome
        counts [n_sizes, nchr])."""
        sizes = np.ascontiguousarray(winsizes, dtype=np.int32)
        st = sizes.copy() if steps is None else np.ascontiguousarray(steps, dtype=np.int32)
        idx = None if ind_idx is None else np.ascontiguousarray(ind_idx, dtype=np.int32)
        m = int(sizes.shape[0])
        h = _vp()
        per_chr = np.zeros((max(m, 1), self.nchr), dtype=np.int64)
        check(lib().garlic_lod_kde_part_set(self.handle, _ptr(sizes, _i32p), _ptr(st, _i32p), m, error, max_gap, int(use_gl),
                                            _ptr(idx, _i32p), 0 if idx is None else int(idx.shape[0]), C.byref(h), _ptr(per_chr, _i64p)))
        return KdePartSet(h, m), per_chr[:m]

    def lod_feed_multi(self, winsizes, error, max_gap, steps=None, ind_idx=None, copy=True):
        """garlic_lod_feed_multi: the feeds of several window sizes in one call (unweighted --error scores; steps
        default to the window sizes).  Returns ([feed per size], per-chromosome counts [n_sizes, nchr]).
        copy=False: the feeds are views of buffers the panel object reuses for the next call."""
        sizes = np.ascontiguousarray(winsizes, dtype=np.int32)
        st = sizes.copy() if steps is None else np.ascontiguousarray(steps, dtype=np.int32)
        idx = None if ind_idx is None else np.ascontiguousarray(ind_idx, dtype=np.int32)
        n_rows = self.nind if idx is None else int(idx.shape[0])
        caps = np.array([max(1, int(sum((int(n) + int(s) - 1) // int(s) for n in self.chr_nloci)) * n_rows) for s in st],
                        dtype=np.int64)
        if copy:
            bufs = [np.empty(int(c), dtype=np.float64) for c in caps]
        else:
            old = getattr(self, "_feed_multi", [])
            bufs = [old[i] if i < len(old) and old[i].shape[0] >= int(c) else np.empty(int(c), dtype=np.float64)
                    for i, c in enumerate(caps)]
            self._feed_multi = bufs
        ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
        counts = np.zeros(len(bufs), dtype=np.int64)
        per_chr = np.zeros((len(bufs), self.nchr), dtype=np.int64)
        check(lib().garlic_lod_feed_multi(self.handle, _ptr(sizes, _i32p), _ptr(st, _i32p), len(bufs), error, max_gap,
                                          _ptr(idx, _i32p), 0 if idx is None else n_rows, ptrs, _ptr(caps, _i64p),
                                          _ptr(counts, _i64p), _ptr(per_chr, _i64p)))
        return [b[: int(n)] for b, n in zip(bufs, counts)], per_chr

    def lod_feed_multi_tgls(self, winsizes, max_gap, steps=None, ind_idx=None, copy=True):
        """garlic_lod_feed_multi_tgls: lod_feed_multi for per-genotype likelihoods (use_gl, unweighted); the sizes that
        take the thinned ring chain share one pass over the term matrix in groups (garlic_hip.h).  Returns and copy as there."""
        sizes = np.ascontiguousarray(winsizes, dtype=np.int32)
        st = sizes.copy() if steps is None else np.ascontiguousarray(steps, dtype=np.int32)
        idx = None if ind_idx is None else np.ascontiguousarray(ind_idx, dtype=np.int32)
        n_rows = self.nind if idx is None else int(idx.shape[0])
        caps = np.array([max(1, int(sum((int(n) + int(s) - 1) // int(s) for n in self.chr_nloci)) * n_rows) for s in st],
                        dtype=np.int64)
        if copy:
            bufs = [np.empty(int(c), dtype=np.float64) for c in caps]
        else:
            old = getattr(self, "_feed_multi", [])
            bufs = [old[i] if i < len(old) and old[i].shape[0] >= int(c) else np.empty(int(c), dtype=np.float64)
                    for i, c in enumerate(caps)]
            self._feed_multi = bufs
        ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs])
        counts = np.zeros(len(bufs), dtype=np.int64)
        per_chr = np.zeros((len(bufs), self.nchr), dtype=np.int64)
        check(lib().garlic_lod_feed_multi_tgls(self.handle, _ptr(sizes, _i32p), _ptr(st, _i32p), len(bufs), max_gap,
                                               _ptr(idx, _i32p), 0 if idx is None else n_rows, ptrs, _ptr(caps, _i64p),
                                               _ptr(counts, _i64p), _ptr(per_chr, _i64p)))
        return [b[: int(n)] for b, n in zip(bufs, counts)], per_chr

    def feed_multi_info(self, n):
        """garlic_lod_feed_multi_info for the first n sizes of the last lod_feed_multi_tgls call: {"forms": [..], "groups": [..],
        "n_chain_launches": int, "n_term_builds": int}"""
        forms, groups = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32)
        launches, builds = C.c_int32(), C.c_int32()
        check(lib().garlic_lod_feed_multi_info(self.handle, n, _ptr(forms, _i32p), _ptr(groups, _i32p), C.byref(launches),
                                               C.byref(builds)))
        return {"forms": [int(x) for x in forms[:n]], "groups": [int(x) for x in groups[:n]],
                "n_chain_launches": launches.value, "n_term_builds": builds.value}

    def alloc_scores(self, winsize, error, max_gap, pitch_align=32, nind_out=None, candidates=0):
        """garlic_panel_alloc_scores: score memory in the chain kernel's fast placement (the real kernel timed into
        `candidates` buffers, the fastest kept).  Returns (DeviceBuffer, [kernel ms per candidate])."""
        nind_out = self.nind if nind_out is None else nind_out
        n = candidates if candidates > 0 else 4
        ms = (C.c_float * n)()
        ptr = _vp()
        check(lib().garlic_panel_alloc_scores(self.handle, pitch_align, nind_out, winsize, error, max_gap, candidates,
                                              C.byref(ptr), ms))
        _, _, total = self.out_layout(pitch_align, nind_out)
        return DeviceBuffer(self.ctx, int(total) * 8, ptr=ptr.value), [float(x) for x in ms]

    def alloc_scores_info(self):
        """garlic_panel_alloc_scores_info: what the last alloc_scores on this panel drew"""
        drawn, rounds, reached = C.c_int32(), C.c_int32(), C.c_int32()
        best, med, worst, target = C.c_float(), C.c_float(), C.c_float(), C.c_float()
        check(lib().garlic_panel_alloc_scores_info(self.handle, C.byref(drawn), C.byref(rounds), C.byref(best), C.byref(med),
                                                   C.byref(worst), C.byref(target), C.byref(reached)))
        return {"candidates_drawn": drawn.value, "rounds": rounds.value, "best_ms": best.value, "median_ms": med.value,
                "worst_ms": worst.value, "target_ms_at_0.74_of_hbm": target.value, "reached_target": bool(reached.value)}

    def feed_info(self):
        """(form, score_doubles) of the last lod_feed / lod_feed_multi call: FEED_FROM_SCORES, FEED_CHAIN,
        FEED_SAMPLED_WLOD or FEED_TGLS_CHAIN, and the doubles of score scratch it needed (garlic_hip.h)"""
        form, n = C.c_int32(), C.c_int64()
        check(lib().garlic_lod_feed_info(self.handle, C.byref(form), C.byref(n)))
        return form.value, n.value

    def chain_kind(self):
        """0 tuned chain, 1 tuned chain + scan for the value -9999.0 (none found), 2 by-value chain (garlic_hip.h)"""
        k = C.c_int32()
        check(lib().garlic_panel_chain_kind(self.handle, C.byref(k)))
        return k.value

    def tgls_mode(self):
        """(mode, terms_by): mode 0 none / 1 dictionary codes / 2 continuous values; terms_by 0 tabulated or
        nothing yet / 1 device log10 / 2 host libm"""
        mode, by = C.c_int32(), C.c_int32()
        check(lib().garlic_panel_tgls_mode(self.handle, C.byref(mode), C.byref(by)))
        return mode.value, by.value

    def set_tgls_term_budget(self, nbytes):
        """garlic_panel_set_tgls_term_budget: 0 the whole term matrix or none (the default), > 0 an upper bound in bytes for the
        term buffers (a larger matrix is built and read slab by slab), -1 whole if it fits, else slabs from the free memory"""
        check(lib().garlic_panel_set_tgls_term_budget(self.handle, int(nbytes)))

    def tgls_terms_info(self):
        """{whole_bytes, resident_bytes, slab_blocks, n_slabs}: what the full term matrix needs, what the panel holds now, and
        the slabs of the last unweighted use_gl call (n_slabs 0: it read a whole matrix or looked its terms up)"""
        whole, res = C.c_int64(), C.c_int64()
        sb, ns = C.c_int32(), C.c_int32()
        check(lib().garlic_panel_tgls_terms_info(self.handle, C.byref(whole), C.byref(res), C.byref(sb), C.byref(ns)))
        return {"whole_bytes": whole.value, "resident_bytes": res.value, "slab_blocks": sb.value, "n_slabs": ns.value}

    def roh_coverage(self, scores_ptr, winsize, cutoff, pitch_align=32, nind_out=None, inwin_pitch_align=1):
        """assembleROHWindows' coverage counts of device-resident scores: list of per-chromosome int16
        [nind_out][pitch_c] host arrays (pitch_c = nloci_c rounded up to inwin_pitch_align; a multiple of 8 lets the kernel
        store 16 bytes at a time)."""
        nind_out = self.nind if nind_out is None else nind_out
        base, pitch, total = self.out_layout(inwin_pitch_align, nind_out)
        out = np.empty(total, dtype=np.int16)
        check(lib().garlic_roh_coverage(self.handle, _vp(scores_ptr), pitch_align, nind_out, winsize, cutoff,
                                        _vp(out.ctypes.data), inwin_pitch_align, HOST))
        return [out[base[c]: base[c] + nind_out * pitch[c]].reshape(nind_out, pitch[c])
                for c in range(self.nchr)]

    def roh_coverage_fused(self, winsize, error, max_gap, cutoff, pitch_align=1, use_gl=False, weighted=False, M=7, mu=1e-9):
        """coverage counts without computing the score matrix (unweighted --error scores, or --weighted with or without
        likelihoods): list of per-chromosome int16 [nind][pitch_c] host arrays (pitch_c = nloci_c rounded up to pitch_align)"""
        base, pitch, total = self.out_layout(pitch_align, self.nind)
        out = np.empty(total, dtype=np.int16)
        check(lib().garlic_roh_coverage_fused(self.handle, winsize, error, max_gap, int(use_gl), int(weighted), M, mu, cutoff,
                                              _vp(out.ctypes.data), pitch_align, HOST))
        return [out[base[c]: base[c] + self.nind * pitch[c]].reshape(self.nind, pitch[c]) for c in range(self.nchr)]

    def roh_segments(self, winsize, error, max_gap, cutoff, overlap_frac, use_gl=False, weighted=False, M=7, mu=1e-9, capacity=None):
        """garlic_roh_segments: the ROH segments of assembleROHWindows without scores or counts in memory -> int32 array
        [n][4] of (individual, chromosome, first SNP, last SNP), in the reference's order.  capacity None: room for 64 per
        individual, once more with the number found if that was too little."""
        n = C.c_int64()
        args = (self.handle, winsize, error, max_gap, int(use_gl), int(weighted), M, mu, cutoff, overlap_frac)
        cap = max(1024, 64 * self.nind) if capacity is None else int(capacity)
        for _ in range(2):
            out = np.empty((max(cap, 1), 4), dtype=np.int32)
            check(lib().garlic_roh_segments(*args, _vp(out.ctypes.data), cap, C.byref(n)))
            if n.value <= cap or capacity is not None:
                break
            cap = n.value           # (nothing usable was written: once more, with room)
        if n.value > cap:
            raise GarlicError(1, f"garlic_roh_segments: {n.value} segments, room for {cap}")
        return out[:n.value].copy()

    def roh_coverage_fused_device(self, winsize, error, max_gap, cutoff, out_ptr, pitch_align=8, use_gl=False, weighted=False,
                                  M=7, mu=1e-9):
        """the same counts into device memory (int16 rows: out_layout(pitch_align, nind))"""
        check(lib().garlic_roh_coverage_fused(self.handle, winsize, error, max_gap, int(use_gl), int(weighted), M, mu, cutoff,
                                              _vp(out_ptr), pitch_align, DEVICE))

    def roh_coverage_device(self, scores_ptr, winsize, cutoff, out_ptr, pitch_align=32, nind_out=None, inwin_pitch_align=1):
        """the same counts into device memory (int16 rows: out_layout(inwin_pitch_align, nind_out))"""
        nind_out = self.nind if nind_out is None else nind_out
        check(lib().garlic_roh_coverage(self.handle, _vp(scores_ptr), pitch_align, nind_out, winsize, cutoff,
                                        _vp(out_ptr), inwin_pitch_align, DEVICE))

    def stats(self):
        st = CallStats()
        check(lib().garlic_last_call_stats(self.handle, C.byref(st)))
        return {k: getattr(st, k) for k, _ in CallStats._fields_}
