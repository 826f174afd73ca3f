"""ctypes binding of libgvamp.so (include/gvamp.h) -- what tests/ and bench.py drive.

This module is plumbing only: every method forwards to one C-ABI entry point.  It never computes on the
CPU and never imports oracle/.  If the library or a GPU is missing it raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgvamp.so")
_LIB = None

SPACE_M, SPACE_N = 0, 1
ABI_VERSION = 4          # GV_ABI_VERSION of include/gvamp.h this module's ctypes structs were written against

EXPORTS = [
    "gv_abi_version", "gv_create", "gv_destroy", "gv_last_error", "gv_synchronize", "gv_set_dims", "gv_mbytes",
    "gv_upload_bed", "gv_upload_bed_file", "gv_synth_bed", "gv_synth_bed_ld", "gv_download_bed", "gv_set_mask", "gv_marker_stats", "gv_get_marker_stats",
    "gv_ax", "gv_atx", "gv_set_layout", "gv_get_layout", "gv_set_kernel_mode", "gv_get_kernel_mode", "gv_vec_alloc", "gv_vec_free", "gv_vec_len",
    "gv_vec_upload", "gv_vec_download", "gv_vec_fill", "gv_vec_copy", "gv_vec_axpby", "gv_vec_mul", "gv_vec_dot", "gv_vec_dots", "gv_vec_dots_ex",
    "gv_ax_dev", "gv_atx_dev", "gv_ax2_dev", "gv_atx2_dev", "gv_set_phen", "gv_lmmse_mult", "gv_cg_solve", "gv_cg_solve2", "gv_cg_solve2x",
    "gv_denoise", "gv_prior_estep", "gv_denoise_global", "gv_prior_estep_global",
    "gv_probit_denoise", "gv_probit_denoise_cov", "gv_people_stats", "gv_cg_solve_aat", "gv_cg_solve_aat2", "gv_cg_solve_aat2w", "gv_cg_solve2w", "gv_pvals_loo", "gv_pvals_loco", "gv_pvals_loco_pred", "gv_allreduce_host", "gv_comm_unique_id", "gv_comm_init", "gv_comm_init_local", "gv_comm_init_callback", "gv_comm_share", "gv_set_overlap", "gv_debug_force_multi", "gv_comm_rank", "gv_comm_size", "gv_bind_host_numa", "gv_set_timing",
    "gv_get_counters", "gv_reset_counters", "gv_get_decomp", "gv_set_decomp", "gv_tune_info", "gv_ingest_info", "gv_ingest_info2", "gv_set_expected_passes", "gv_copy_bandwidth", "gv_read_bandwidth",
    "gv_upload_meth", "gv_upload_meth_file", "gv_synth_meth", "gv_upload_dosage", "gv_upload_dosage_file", "gv_synth_dosage",
    "gv_huber_denoise", "gv_huber_delta",
    "gv_set_cg_precond", "gv_precond_info", "gv_precond_window_gram", "gv_precond_apply",
    "gv_assoc_loo", "gv_assoc_loco",
    "gv_set_dosage_missing", "gv_synth_dosage_na", "gv_dosage_info", "gv_marker_counts",
    "gv_set_dosage_route", "gv_get_dosage_route",
    "gv_ld_scores", "gv_ld_band", "gv_ld_info", "gv_ld_scores_pos", "gv_ld_last_passes",
    "gv_ld_clump", "gv_ld_clump_last", "gv_ld_clump_seconds",
    "gv_set_ld_dosage", "gv_get_ld_dosage",
    "gv_synth_dosage_ld",
    "gv_score_dev", "gv_score", "gv_score_info",
    "gv_atxm_dev", "gv_atxm", "gv_atxm_info", "gv_screen_dev",
    "gv_pca_dev", "gv_pca_loadings_dev", "gv_pca_info",
    "gv_king_block", "gv_king_pairs", "gv_king_info",
    "gv_grm_weights", "gv_grm_block", "gv_grm_pairs", "gv_grm_info", "gv_grm_apply", "gv_grm_he",
    "gv_screen_cov_set", "gv_screen_cov_dev", "gv_screen_cov_info",
    "gv_set_screen_dosage", "gv_get_screen_dosage",
]


class GvError(RuntimeError):
    pass


class DotSpec(C.Structure):            # gv_dot_spec (include/gvamp.h)
    _fields_ = [("xa", C.c_void_p), ("xb", C.c_void_p), ("ya", C.c_void_p), ("yb", C.c_void_p), ("sync", C.c_int)]


class AssocOut(C.Structure):           # gv_assoc_out
    _fields_ = [("beta", C.POINTER(C.c_double)), ("se", C.POINTER(C.c_double)), ("t", C.POINTER(C.c_double)),
                ("p", C.POINTER(C.c_double))]


class DosageStats(C.Structure):        # gv_dosage_stats
    _fields_ = [("scale", C.c_double), ("reserved", C.c_uint64), ("bits", C.c_int), ("missing", C.c_int), ("na_kernels", C.c_int),
                ("pad_", C.c_int)]


class ScoreStats(C.Structure):         # gv_score_stats
    _fields_ = [("path", C.c_int), ("cols_per_pass", C.c_int), ("ksegs", C.c_int), ("min_cols", C.c_int), ("columns", C.c_int64),
                ("passes", C.c_int64), ("scratch_bytes", C.c_uint64), ("seconds", C.c_double)]


SCORE_PATH_KERNEL, SCORE_PATH_FALLBACK = 1, 2


class AtxmStats(C.Structure):          # gv_atxm_stats
    _fields_ = [("path", C.c_int), ("cols_per_pass", C.c_int), ("ksegs", C.c_int), ("min_cols", C.c_int), ("columns", C.c_int64),
                ("passes", C.c_int64), ("scratch_bytes", C.c_uint64), ("seconds", C.c_double)]


ATXM_PATH_KERNEL, ATXM_PATH_FALLBACK = 1, 2


class PcaStats(C.Structure):           # gv_pca_stats
    _fields_ = [("iterations", C.c_int), ("converged", C.c_int), ("block", C.c_int), ("pad_", C.c_int), ("cols_atxm", C.c_int64),
                ("cols_score", C.c_int64), ("scratch_bytes", C.c_uint64), ("seconds_products", C.c_double),
                ("seconds_panel", C.c_double), ("seconds", C.c_double)]


PCA_MAX_BLOCK = 32


class KingStats(C.Structure):          # gv_king_stats
    _fields_ = [("seconds", C.c_double), ("block_pairs", C.c_int64), ("used_markers", C.c_int64), ("pairs", C.c_int64),
                ("useful_macs", C.c_double), ("scratch_bytes", C.c_double)]


class GrmStats(C.Structure):           # gv_grm_stats
    _fields_ = [("seconds", C.c_double), ("block_pairs", C.c_int64), ("counting_markers", C.c_int64), ("dropped_markers", C.c_int64),
                ("pairs", C.c_int64), ("useful_macs", C.c_double), ("scratch_bytes", C.c_double), ("passes", C.c_int64),
                ("blocks_computed", C.c_int64)]


GRM_APPLY_MAX_COLS = 32


class HeResult(C.Structure):           # gv_he_result
    _fields_ = [("n_ind", C.c_int64), ("n_pairs", C.c_int64), ("sum_a", C.c_double), ("sum_aa", C.c_double), ("h2", C.c_double),
                ("intercept", C.c_double), ("se_ols", C.c_double), ("se_jack", C.c_double)]


HE_DTYPE = np.dtype([("n_ind", np.int64), ("n_pairs", np.int64), ("sum_a", np.float64), ("sum_aa", np.float64), ("h2", np.float64),
                     ("intercept", np.float64), ("se_ols", np.float64), ("se_jack", np.float64)])


class ScreenCovStats(C.Structure):     # gv_screen_cov_stats
    _fields_ = [("K", C.c_int), ("pad_", C.c_int), ("nu", C.c_int64), ("cached_bytes", C.c_uint64),
                ("set_seconds_products", C.c_double), ("set_seconds_panel", C.c_double), ("set_seconds", C.c_double),
                ("columns", C.c_int64), ("call_seconds_products", C.c_double), ("call_seconds_panel", C.c_double),
                ("call_seconds", C.c_double)]


class CgStats(C.Structure):
    _fields_ = [("iters", C.c_int), ("converged", C.c_int), ("rel_res", C.c_double), ("onsager", C.c_double),
                ("n_ax", C.c_int), ("n_atx", C.c_int), ("n_relres", C.c_int)]


class CgExtras(C.Structure):
    _fields_ = [("ride_x", C.c_void_p), ("ride_out", C.c_void_p), ("a_mu_a", C.c_void_p), ("ata_mu_b", C.c_void_p)]


class CgWarm(C.Structure):
    _fields_ = [("ata_mu_start_a", C.c_void_p), ("a_mu_start_a", C.c_void_p), ("ata_mu_a", C.c_void_p),
                ("ata_v_b", C.c_void_p), ("have_ata_v_b", C.c_int)]


class AatWarm(C.Structure):
    _fields_ = [("aat_mu_start_a", C.c_void_p), ("at_mu_start_a", C.c_void_p), ("accumulate_at_mu_a", C.c_int),
                ("ata_v_b", C.c_void_p), ("have_ata_v_b", C.c_int), ("pre_x", C.c_void_p), ("pre_out", C.c_void_p),
                ("ride_x", C.c_void_p), ("ride_out", C.c_void_p), ("pre_scale", C.c_double)]


class Counters(C.Structure):
    _fields_ = [("n_ax", C.c_int64), ("n_atx", C.c_int64), ("ms_ax", C.c_double), ("ms_atx", C.c_double),
                ("ms_allreduce", C.c_double), ("n_ax_kernel", C.c_int64), ("n_atx_kernel", C.c_int64),
                ("ms_ax_kernel", C.c_double), ("ms_atx_kernel", C.c_double), ("n_ax_pass", C.c_int64),
                ("n_atx_pass", C.c_int64), ("n_allreduce", C.c_int64)]


class IngestStats(C.Structure):      # gv_ingest_stats
    _fields_ = [("alloc_seconds", C.c_double), ("fill_seconds", C.c_double), ("overlap_seconds", C.c_double),
                ("resident_bytes", C.c_double), ("layout", C.c_int), ("expected_passes", C.c_int64)]


class DecompInfo(C.Structure):
    _fields_ = [("ks", C.c_int), ("balanced_cells", C.c_int64), ("prio", C.c_int), ("taper", C.c_float), ("tuned", C.c_int),
                ("whole_quads", C.c_int64), ("geo", C.c_float), ("wgs_per_cu", C.c_int), ("xcd_skew", C.c_float)]


class PrecondStats(C.Structure):     # gv_precond_stats
    _fields_ = [("kind", C.c_int), ("window", C.c_int), ("windows", C.c_int64 * 2), ("first_window", C.c_int64 * 2),
                ("resident_bytes", C.c_double), ("build_seconds", C.c_double), ("factorisations", C.c_int64),
                ("fallback_windows", C.c_int64), ("last_tau", C.c_double), ("last_gam2", C.c_double)]


class LdStats(C.Structure):          # gv_ld_stats
    _fields_ = [("seconds", C.c_double), ("block_pairs", C.c_int64), ("useful_macs", C.c_double), ("scratch_bytes", C.c_double)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_size_t)


def bind_host_numa(device):
    """gv_bind_host_numa: this process onto the CPUs next to its GPU; returns the NUMA node or -1 (nothing changed)"""
    L = load()
    node = C.c_int(-1)
    if L.gv_bind_host_numa(int(device), C.byref(node)):
        raise GvError(L.gv_last_error(None).decode())
    return node.value


def load():
    """dlopen libgvamp.so.  Raises if it has not been built (python gvamp_amd/build.py)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise GvError("libgvamp.so is not built: run `python gvamp_amd/build.py` (needs hipcc)")
    L = C.CDLL(LIB_PATH)
    if L.gv_abi_version() != ABI_VERSION:
        raise GvError("libgvamp.so speaks ABI %d, this binding %d: rebuild (python gvamp_amd/build.py --force)" % (L.gv_abi_version(), ABI_VERSION))
    vp, dp, up = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    i64 = C.c_int64
    L.gv_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.gv_destroy.argtypes = [vp]
    L.gv_destroy.restype = None
    L.gv_last_error.argtypes = [vp]
    L.gv_last_error.restype = C.c_char_p
    L.gv_synchronize.argtypes = [vp]
    L.gv_set_dims.argtypes = [vp, i64, i64, i64, i64]
    L.gv_mbytes.argtypes = [vp]
    L.gv_mbytes.restype = i64
    L.gv_upload_bed.argtypes = [vp, up, C.c_size_t]
    L.gv_synth_bed.argtypes = [vp, C.c_uint64, C.c_uint32]
    L.gv_synth_bed_ld.argtypes = [vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32]
    L.gv_upload_bed_file.argtypes = [vp, C.c_char_p, i64]
    L.gv_download_bed.argtypes = [vp, up, C.c_size_t]
    L.gv_upload_meth.argtypes = [vp, dp, C.c_size_t]
    L.gv_upload_meth_file.argtypes = [vp, C.c_char_p, i64]
    L.gv_synth_meth.argtypes = [vp, C.c_uint64]
    L.gv_upload_dosage.argtypes = [vp, C.c_void_p, C.c_size_t, C.c_int, C.c_double]
    L.gv_upload_dosage_file.argtypes = [vp, C.c_char_p, i64, C.c_int, C.c_double]
    L.gv_synth_dosage.argtypes = [vp, C.c_uint64, C.c_int]
    L.gv_set_dosage_missing.argtypes = [vp, C.c_int]
    L.gv_synth_dosage_na.argtypes = [vp, C.c_uint64, C.c_int, C.c_uint32]
    L.gv_synth_dosage_ld.argtypes = [vp, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]
    L.gv_dosage_info.argtypes = [vp, C.POINTER(DosageStats)]
    L.gv_marker_counts.argtypes = [vp, dp]
    L.gv_set_dosage_route.argtypes = [vp, C.c_int]
    L.gv_get_dosage_route.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.gv_set_mask.argtypes = [vp, up, i64]
    L.gv_marker_stats.argtypes = [vp, C.c_double]
    L.gv_get_marker_stats.argtypes = [vp, dp, dp]
    L.gv_ax.argtypes = [vp, dp, dp]
    L.gv_atx.argtypes = [vp, dp, dp]
    L.gv_set_kernel_mode.argtypes = [vp, C.c_int]
    L.gv_set_layout.argtypes = [vp, C.c_int, C.c_int]
    L.gv_get_layout.argtypes = [vp]
    L.gv_get_kernel_mode.argtypes = [vp]
    L.gv_vec_alloc.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.gv_vec_free.argtypes = [vp, vp]
    L.gv_vec_free.restype = None
    L.gv_vec_len.argtypes = [vp]
    L.gv_vec_len.restype = i64
    L.gv_vec_upload.argtypes = [vp, vp, dp]
    L.gv_vec_download.argtypes = [vp, vp, dp]
    L.gv_vec_fill.argtypes = [vp, vp, C.c_double]
    L.gv_vec_copy.argtypes = [vp, vp, vp]
    L.gv_vec_axpby.argtypes = [vp, vp, C.c_double, vp, C.c_double, vp]
    L.gv_vec_mul.argtypes = [vp, vp, vp, vp]
    L.gv_vec_dot.argtypes = [vp, vp, vp, C.c_int, dp]
    L.gv_vec_dots.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), C.c_int, dp]
    L.gv_vec_dots_ex.argtypes = [vp, C.c_int, C.POINTER(DotSpec), dp]
    L.gv_ax_dev.argtypes = [vp, vp, vp]
    L.gv_atx_dev.argtypes = [vp, vp, vp]
    L.gv_ax2_dev.argtypes = [vp, vp, vp, vp, vp]
    L.gv_atx2_dev.argtypes = [vp, vp, vp, vp, vp]
    L.gv_cg_solve2.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, vp, C.POINTER(CgStats),
                               C.POINTER(CgStats), dp, dp]
    L.gv_cg_solve2x.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, vp, C.POINTER(CgStats),
                                C.POINTER(CgStats), dp, dp, C.POINTER(CgExtras)]
    L.gv_cg_solve2w.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, vp, C.POINTER(CgStats),
                                C.POINTER(CgStats), dp, dp, C.POINTER(CgExtras), C.POINTER(CgWarm)]
    L.gv_set_phen.argtypes = [vp, vp, dp]
    L.gv_lmmse_mult.argtypes = [vp, vp, C.c_double, C.c_double, vp]
    L.gv_cg_solve.argtypes = [vp, vp, vp, C.c_double, C.c_double, C.c_int, C.c_int, vp, C.POINTER(CgStats), dp]
    L.gv_denoise.argtypes = [vp, vp, C.c_double, dp, dp, C.c_int, vp, vp, dp]
    L.gv_prior_estep.argtypes = [vp, vp, C.c_double, C.c_double, dp, dp, C.c_int, dp]
    L.gv_allreduce_host.argtypes = [vp, dp, C.c_int]
    L.gv_probit_denoise.argtypes = [vp, vp, vp, C.c_double, C.c_double, vp, dp]
    L.gv_probit_denoise_cov.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, vp, dp]
    L.gv_huber_denoise.argtypes = [vp, vp, vp, C.c_double, C.c_double, vp, dp]
    L.gv_huber_delta.argtypes = [vp, vp, vp, C.c_double, dp, C.c_int, dp]
    L.gv_set_cg_precond.argtypes = [vp, C.c_int, C.c_int]
    L.gv_precond_info.argtypes = [vp, C.POINTER(PrecondStats)]
    L.gv_precond_window_gram.argtypes = [vp, C.c_int, i64, dp]
    L.gv_precond_apply.argtypes = [vp, C.c_double, C.c_double, vp, vp]
    L.gv_ld_scores.argtypes = [vp, i64, C.POINTER(C.c_int), C.c_int, dp, dp]
    L.gv_ld_band.argtypes = [vp, i64, C.POINTER(C.c_int), i64, i64, dp]
    L.gv_ld_info.argtypes = [vp, C.POINTER(LdStats)]
    i32p = C.POINTER(C.c_int32)
    L.gv_king_block.argtypes = [vp, up, i64, i64, i64, i64, dp, i32p]
    L.gv_king_pairs.argtypes = [vp, up, C.c_double, i64, i32p, i32p, dp, i32p, C.POINTER(i64)]
    L.gv_king_info.argtypes = [vp, C.POINTER(KingStats)]
    L.gv_grm_weights.argtypes = [vp, up, dp, dp, C.POINTER(i64)]
    L.gv_grm_block.argtypes = [vp, up, i64, i64, i64, i64, dp, i32p]
    L.gv_grm_pairs.argtypes = [vp, up, C.c_double, i64, i32p, i32p, dp, i32p, dp, i32p, C.POINTER(i64)]
    L.gv_grm_info.argtypes = [vp, C.POINTER(GrmStats)]
    L.gv_grm_apply.argtypes = [vp, up, C.c_int, dp, dp, dp, dp]
    L.gv_grm_he.argtypes = [vp, up, i64, dp, C.POINTER(HeResult)]
    L.gv_ld_scores_pos.argtypes = [vp, dp, C.c_double, C.POINTER(C.c_int), C.c_int, dp, C.c_int, dp, dp]
    L.gv_ld_last_passes.argtypes = [vp, C.POINTER(C.c_int)]
    L.gv_ld_clump.argtypes = [vp, dp, C.c_double, C.POINTER(C.c_int), dp, C.c_double, C.c_double, C.c_double, C.POINTER(i64), C.POINTER(i64)]
    L.gv_ld_clump_last.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(i64), C.POINTER(i64)]
    L.gv_ld_clump_seconds.argtypes = [vp, dp, dp]
    L.gv_score_dev.argtypes = [vp, i64, C.POINTER(vp), C.POINTER(vp)]
    L.gv_score.argtypes = [vp, i64, dp, dp]
    L.gv_score_info.argtypes = [vp, C.POINTER(ScoreStats)]
    L.gv_atxm_dev.argtypes = [vp, i64, C.POINTER(vp), C.POINTER(vp)]
    L.gv_atxm.argtypes = [vp, i64, dp, dp]
    L.gv_atxm_info.argtypes = [vp, C.POINTER(AtxmStats)]
    L.gv_screen_dev.argtypes = [vp, i64, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.gv_pca_dev.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp), C.c_double, C.c_int, C.POINTER(vp), dp, dp]
    L.gv_pca_loadings_dev.argtypes = [vp, C.c_int, C.POINTER(vp), dp, C.POINTER(vp)]
    L.gv_pca_info.argtypes = [vp, C.POINTER(PcaStats)]
    L.gv_screen_cov_set.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.gv_screen_cov_dev.argtypes = [vp, i64, C.POINTER(vp), C.c_double] + [C.POINTER(vp)] * 5
    L.gv_screen_cov_info.argtypes = [vp, C.POINTER(ScreenCovStats)]
    L.gv_set_ld_dosage.argtypes = [vp, C.c_int]
    L.gv_get_ld_dosage.argtypes = [vp, C.POINTER(C.c_int)]
    L.gv_set_screen_dosage.argtypes = [vp, C.c_int]
    L.gv_get_screen_dosage.argtypes = [vp, C.POINTER(C.c_int)]
    L.gv_people_stats.argtypes = [vp, dp, dp, dp]
    L.gv_cg_solve_aat.argtypes = [vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, C.POINTER(CgStats), dp]
    L.gv_cg_solve_aat2.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, vp, vp, C.POINTER(CgStats),
                                   C.POINTER(CgStats), dp, dp, vp, vp]
    L.gv_cg_solve_aat2w.argtypes = [vp, vp, vp, vp, C.c_double, C.c_double, C.c_int, vp, vp, vp, C.POINTER(CgStats),
                                    C.POINTER(CgStats), dp, dp, vp, vp, C.POINTER(AatWarm)]
    L.gv_pvals_loo.argtypes = [vp, vp, vp, vp, dp]
    L.gv_pvals_loco.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int), dp]
    L.gv_pvals_loco_pred.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int), dp, dp]
    L.gv_assoc_loo.argtypes = [vp, vp, vp, vp, C.POINTER(AssocOut)]
    L.gv_assoc_loco.argtypes = [vp, vp, vp, vp, C.POINTER(C.c_int), C.POINTER(AssocOut), dp]
    L.gv_comm_unique_id.argtypes = [C.c_void_p]
    L.gv_comm_init.argtypes = [vp, C.c_int, C.c_int, C.c_void_p]
    L.gv_comm_init_local.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.gv_comm_init_callback.argtypes = [vp, C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p]
    L.gv_comm_share.argtypes = [vp, vp]
    L.gv_set_overlap.argtypes = [vp, C.c_int]
    L.gv_comm_rank.argtypes = [vp]
    L.gv_comm_size.argtypes = [vp]
    L.gv_set_timing.argtypes = [vp, C.c_int]
    L.gv_get_counters.argtypes = [vp, C.POINTER(Counters)]
    L.gv_reset_counters.argtypes = [vp]
    L.gv_get_decomp.argtypes = [vp, C.POINTER(DecompInfo)]
    L.gv_set_decomp.argtypes = [vp, C.c_int, C.POINTER(DecompInfo)]
    L.gv_tune_info.argtypes = [vp, dp, C.POINTER(C.c_int)]
    L.gv_ingest_info.argtypes = [vp, dp, dp]
    L.gv_ingest_info2.argtypes = [vp, C.POINTER(IngestStats)]
    L.gv_set_expected_passes.argtypes = [vp, C.c_int64]
    L.gv_debug_force_multi.argtypes = [vp, C.c_int, C.c_int]
    L.gv_bind_host_numa.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.gv_copy_bandwidth.argtypes = [vp, C.c_size_t, C.c_int, dp]
    L.gv_read_bandwidth.argtypes = [vp, C.c_size_t, C.c_int, dp]
    _LIB = L
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_ubyte))


def comm_unique_id():
    buf = (C.c_ubyte * 128)()
    if load().gv_comm_unique_id(buf):
        raise GvError(load().gv_last_error(None).decode())
    return bytes(buf)


class Vec:
    """Device-resident fp64 vector (gv_vec)."""

    def __init__(self, shard, space):
        self.shard = shard
        h = C.c_void_p()
        shard._ck(shard.L.gv_vec_alloc(shard.h, space, C.byref(h)))
        self.h = h
        self.space = space
        self.n = shard.L.gv_vec_len(h)

    def upload(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        assert a.size == self.n, (a.size, self.n)
        self.shard._ck(self.shard.L.gv_vec_upload(self.shard.h, self.h, _dp(a)))
        return self

    def download(self):
        out = np.empty(self.n)
        self.shard._ck(self.shard.L.gv_vec_download(self.shard.h, self.h, _dp(out)))
        return out

    def fill(self, v):
        self.shard._ck(self.shard.L.gv_vec_fill(self.shard.h, self.h, float(v)))
        return self

    def free(self):
        if self.h:
            self.shard.L.gv_vec_free(self.shard.h, self.h)
            self.h = None


class Shard:
    """One marker shard resident on one GPU: the device side of the reference's `class data`
    (data.hpp:93-140).  Method names follow the reference (Ax, ATx, compute_markers_statistics...)."""

    def __init__(self, N, M, Mt=None, S=0, device=0, anchor=False):
        """Nothing but gv_create + gv_set_dims: the context keeps the C ABI's defaults (kernel mode 1, no raw rows, layout
        picked at ingest).  anchor=True opts into the parity-anchor set-up of the tests that compare the two kernel families or
        read the rows back: raw rows + two stripe sets resident, fp64 VALU family selected (gv_set_layout(1, 1),
        gv_set_kernel_mode(0))."""
        self.L = load()
        h = C.c_void_p()
        if self.L.gv_create(device, C.byref(h)):
            raise GvError(self.L.gv_last_error(None).decode())
        self.h = h
        self.N, self.M, self.Mt, self.S = N, M, (M if Mt is None else Mt), S
        self._ck(self.L.gv_set_dims(h, N, M, self.Mt, S))
        self.mbytes = self.L.gv_mbytes(h)
        self._present = None              # the mask as set_mask left it (None: everyone has a phenotype); read by screen()
        if anchor:
            self.set_layout(True, 1)
            self.set_kernel_mode(0)

    def _ck(self, rc):
        if rc:
            raise GvError(self.L.gv_last_error(self.h).decode())

    def set_dims(self, N, M, Mt=None, S=0):
        """gv_set_dims on a live context: the data set, the mask (everyone present again) and the statistics go; vectors allocated
        before do not outlive the call (every entry point refuses them) -- free them and allocate new ones"""
        Mt = M if Mt is None else Mt
        self._ck(self.L.gv_set_dims(self.h, N, M, Mt, S))
        self.N, self.M, self.Mt, self.S = N, M, Mt, S
        self.mbytes = self.L.gv_mbytes(self.h)
        self._present = None

    def close(self):
        if self.h:
            self.L.gv_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- dataset -------------------------------------------------------------------------------------
    def upload_bed(self, bed):
        bed = np.ascontiguousarray(bed, dtype=np.uint8)
        self._ck(self.L.gv_upload_bed(self.h, _up(bed), bed.size))

    def upload_bed_file(self, path, offset=None):
        off = 3 + self.S * self.mbytes if offset is None else offset
        self._ck(self.L.gv_upload_bed_file(self.h, path.encode(), off))

    def synth_bed(self, seed, miss_ppm=5000, ld_block=0, ld_ppm=0):
        if ld_block:
            self._ck(self.L.gv_synth_bed_ld(self.h, seed, miss_ppm, ld_block, ld_ppm))
        else:
            self._ck(self.L.gv_synth_bed(self.h, seed, miss_ppm))

    def upload_meth(self, x):
        """methylation data (type_data == "meth"): M x N doubles of this shard, marker-major"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.M * self.N, (x.size, self.M, self.N)
        self._ck(self.L.gv_upload_meth(self.h, _dp(x), x.size))

    def upload_meth_file(self, path, offset=None):
        """M x N doubles at byte offset (default S * N * 8, data.cpp:259) of a file of raw doubles"""
        off = self.S * self.N * 8 if offset is None else offset
        self._ck(self.L.gv_upload_meth_file(self.h, path.encode(), off))

    def synth_meth(self, seed):
        """the device-generated methylation matrix that synth.synth_meth(N, M, seed, S) reproduces on the host"""
        self._ck(self.L.gv_synth_meth(self.h, seed))

    def upload_dosage(self, codes, scale, missing=False):
        """compact dense data: M x N unsigned codes of this shard, marker-major, X = scale * codes; codes.dtype (uint8 / uint16)
        selects the width.  missing: the all-ones code (255 / 65535) is a missing entry (gv_set_dosage_missing)"""
        codes = np.ascontiguousarray(codes)
        if codes.dtype not in (np.uint8, np.uint16):
            raise GvError("upload_dosage: codes must be uint8 or uint16, not %s" % codes.dtype)
        assert codes.size == self.M * self.N, (codes.size, self.M, self.N)
        self.set_dosage_missing(missing)
        self._ck(self.L.gv_upload_dosage(self.h, codes.ctypes.data_as(C.c_void_p), codes.size, 8 * codes.dtype.itemsize, scale))

    def upload_dosage_file(self, path, bits, scale, offset=None, missing=False):
        """M x N codes of `bits` bits at byte offset (default S * N * bits / 8) of a file of raw codes; missing as upload_dosage"""
        off = self.S * self.N * (bits // 8) if offset is None else offset
        self.set_dosage_missing(missing)
        self._ck(self.L.gv_upload_dosage_file(self.h, path.encode(), off, bits, scale))

    def synth_dosage(self, seed, bits):
        """the device-generated codes that synth.synth_dosage(N, M, seed, bits, S) reproduces on the host (scale 1/127, 1/16384)"""
        self._ck(self.L.gv_synth_dosage(self.h, seed, bits))

    def set_dosage_missing(self, on):
        """gv_set_dosage_missing: read by the next upload of codes; refused while codes uploaded with the other setting are resident"""
        self._ck(self.L.gv_set_dosage_missing(self.h, int(bool(on))))

    def synth_dosage_na(self, seed, bits, miss_ppm):
        """the device-generated codes with missing entries that synth.synth_dosage_na(N, M, seed, bits, miss_ppm, S) reproduces on the
        host; turns the missing option on"""
        self._ck(self.L.gv_synth_dosage_na(self.h, seed, bits, miss_ppm))

    def synth_dosage_ld(self, seed, bits, ld_block, ld_ppm, miss_ppm=0):
        """the device-generated block-correlated codes that synth.synth_dosage_ld(N, M, seed, bits, ld_block, ld_ppm, miss_ppm, S)
        reproduces on the host; miss_ppm > 0 turns the missing option on"""
        self._ck(self.L.gv_synth_dosage_ld(self.h, seed, bits, miss_ppm, ld_block, ld_ppm))

    def dosage_info(self):
        """gv_dosage_info as a dict: bits, scale, missing (option on), reserved (codes counted at ingest), na_kernels (in use)"""
        st = DosageStats()
        self._ck(self.L.gv_dosage_info(self.h, C.byref(st)))
        return dict(bits=st.bits, scale=st.scale, missing=bool(st.missing), reserved=int(st.reserved), na_kernels=bool(st.na_kernels))

    def set_dosage_route(self, route):
        """gv_set_dosage_route: 0 = the VALU kernels of the dosage kind (default), 1 = fixed-point i8 MFMA (8-bit codes without missing
        entries; a request, kept where it does not apply)"""
        self._ck(self.L.gv_set_dosage_route(self.h, int(route)))

    def dosage_route(self):
        """gv_get_dosage_route: (requested, in_force)"""
        req, inf = C.c_int(0), C.c_int(0)
        self._ck(self.L.gv_get_dosage_route(self.h, C.byref(req), C.byref(inf)))
        return req.value, inf.value

    def marker_counts(self):
        """gv_marker_counts: the M per-marker counts sum b na after compute_markers_statistics (dosage data)"""
        cnt = np.empty(self.M)
        self._ck(self.L.gv_marker_counts(self.h, _dp(cnt)))
        return cnt

    def download_bed(self):
        out = np.empty(self.M * self.mbytes, dtype=np.uint8)
        self._ck(self.L.gv_download_bed(self.h, _up(out), out.size))
        return out

    def set_mask(self, mask4, nonas):
        m = np.ascontiguousarray(mask4, dtype=np.uint8)
        assert m.size == self.mbytes
        self._ck(self.L.gv_set_mask(self.h, _up(m), nonas))
        self._present = (((m.reshape(-1)[:, None] >> np.arange(4, dtype=np.uint8)) & 1).reshape(-1)[:self.N]).astype(bool)

    def compute_markers_statistics(self, alpha_scale=1.0):
        self._ck(self.L.gv_marker_stats(self.h, alpha_scale))

    def marker_stats(self):
        mave, msig = np.empty(self.M), np.empty(self.M)
        self._ck(self.L.gv_get_marker_stats(self.h, _dp(mave), _dp(msig)))
        return mave, msig

    def set_layout(self, raw_rows=True, stripes=True):
        self._ck(self.L.gv_set_layout(self.h, int(raw_rows), int(stripes)))

    def get_layout(self):
        return self.L.gv_get_layout(self.h)

    def set_kernel_mode(self, mode):
        self._ck(self.L.gv_set_kernel_mode(self.h, mode))

    def get_kernel_mode(self):
        return self.L.gv_get_kernel_mode(self.h)

    # ---- host-signature matvecs (data::Ax / data::ATx) ---------------------------------------------------
    def Ax(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.M
        out = np.empty(4 * self.mbytes)
        self._ck(self.L.gv_ax(self.h, _dp(x), _dp(out)))
        return out

    def ATx(self, p):
        p = np.ascontiguousarray(p, dtype=np.float64)
        assert p.size == 4 * self.mbytes
        out = np.empty(self.M)
        self._ck(self.L.gv_atx(self.h, _dp(p), _dp(out)))
        return out

    # ---- device vectors -------------------------------------------------------------------------------
    def vec(self, space, data=None):
        v = Vec(self, space)
        if data is not None:
            v.upload(data)
        return v

    def vecM(self, data=None):
        return self.vec(SPACE_M, data)

    def vecN(self, data=None):
        return self.vec(SPACE_N, data)

    def set_phen(self, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        assert y.size == self.N
        v = Vec(self, SPACE_N)
        self._ck(self.L.gv_set_phen(self.h, v.h, _dp(y)))
        return v

    def ax_dev(self, x, out):
        self._ck(self.L.gv_ax_dev(self.h, x.h, out.h))

    def atx_dev(self, p, out):
        self._ck(self.L.gv_atx_dev(self.h, p.h, out.h))

    def axpby(self, out, a, x, b=0.0, y=None):
        self._ck(self.L.gv_vec_axpby(self.h, out.h, a, x.h, b, y.h if y is not None else None))

    def copy(self, dst, src):
        self._ck(self.L.gv_vec_copy(self.h, dst.h, src.h))

    def dot(self, x, y, sync=1):
        out = C.c_double()
        self._ck(self.L.gv_vec_dot(self.h, x.h, y.h, sync, C.byref(out)))
        return out.value

    def dots(self, pairs, sync=1):
        n = len(pairs)
        xs = (C.c_void_p * n)(*[p[0].h for p in pairs])
        ys = (C.c_void_p * n)(*[p[1].h for p in pairs])
        out = np.empty(n)
        self._ck(self.L.gv_vec_dots(self.h, n, xs, ys, sync, _dp(out)))
        return out

    def dots_ex(self, specs):
        """specs: (xa, xb, ya, yb, sync) tuples, xb / yb may be None: <xa - xb, ya - yb> in one launch and one read-back"""
        n = len(specs)
        arr = (DotSpec * n)()
        for k, (xa, xb, ya, yb, sync) in enumerate(specs):
            arr[k] = DotSpec(xa.h, xb.h if xb is not None else None, ya.h, yb.h if yb is not None else None, int(sync))
        out = np.empty(n)
        self._ck(self.L.gv_vec_dots_ex(self.h, n, arr, _dp(out)))
        return out

    def lmmse_mult(self, v, tau, gam2, out):
        self._ck(self.L.gv_lmmse_mult(self.h, v.h, tau, gam2, out.h))

    def cg_solve(self, v, mu_start, tau, gam2, denoiser, max_iter, mu_out):
        st = CgStats()
        rr = np.zeros(max(max_iter, 1))
        self._ck(self.L.gv_cg_solve(self.h, v.h, mu_start.h if mu_start is not None else None, tau, gam2, denoiser,
                                    max_iter, mu_out.h, C.byref(st), _dp(rr)))
        return st, rr[:st.n_relres].copy()

    def set_cg_precond(self, kind, window=128):
        """gv_set_cg_precond: 0 / "scalar" (the default) or 1 / "ld" with windows of 32, 64 or 128 markers"""
        k = {"scalar": 0, "ld": 1}.get(kind, kind)
        self._ck(self.L.gv_set_cg_precond(self.h, int(k), int(window)))

    def precond_info(self):
        st = PrecondStats()
        self._ck(self.L.gv_precond_info(self.h, C.byref(st)))
        return {"kind": st.kind, "window": st.window, "windows": list(st.windows), "first_window": list(st.first_window),
                "resident_bytes": st.resident_bytes, "build_seconds": st.build_seconds, "factorisations": st.factorisations,
                "fallback_windows": st.fallback_windows, "last_tau": st.last_tau, "last_gam2": st.last_gam2}

    def precond_window_gram(self, grid, k):
        """W x W Gram of window k of grid 0 / 1, clipped to the shard (zero past its clipped length)"""
        W = self.precond_info()["window"]
        out = np.empty(W * W)
        self._ck(self.L.gv_precond_window_gram(self.h, int(grid), int(k), _dp(out)))
        return out.reshape(W, W)

    def precond_apply(self, tau, gam2, r, z):
        self._ck(self.L.gv_precond_apply(self.h, tau, gam2, r.h, z.h))

    def _chrom(self, chrom):
        if chrom is None:
            return None, None
        ch = np.ascontiguousarray(chrom, dtype=np.int32)
        assert ch.size == self.M
        return ch, ch.ctypes.data_as(C.POINTER(C.c_int))

    def ld_scores(self, window, chrom=None, adjusted=False):
        """gv_ld_scores: (l2[M], npairs[M]) -- l_j = 1 + sum of f(r_jk^2) over the band of `window` markers on each side (clipped
        to the shard and, with chrom, to the chromosome), NaN / 0 for a monomorphic marker; adjusted: the LDSC estimator"""
        l2, n = np.zeros(max(self.M, 1)), np.zeros(max(self.M, 1))
        ch, chp = self._chrom(chrom)
        self._ck(self.L.gv_ld_scores(self.h, int(window), chp, int(bool(adjusted)), _dp(l2), _dp(n)))
        return l2[:self.M].copy(), n[:self.M].copy()

    def ld_scores_pos(self, pos, radius, chrom=None, adjusted=False, annot=None):
        """gv_ld_scores_pos: (l2, npairs[M]) over the band |pos_k - pos_j| <= radius on the same chromosome; l2 has shape (M,) without
        annot and (M, C) with the M x C annotation matrix: l(j, c) = a_jc + sum of f(r_jk^2) a_kc.  pos=None passes NULL (refused)."""
        M = self.M
        p = None if pos is None else np.ascontiguousarray(pos, dtype=np.float64)
        assert p is None or p.size == M
        C_ = 1
        an = None
        if annot is not None:
            an = np.ascontiguousarray(annot, dtype=np.float64)
            assert an.ndim == 2 and an.shape[0] == M
            C_ = an.shape[1]
        l2, n = np.zeros(max(M, 1) * max(C_, 1)), np.zeros(max(M, 1))
        ch, chp = self._chrom(chrom)
        self._ck(self.L.gv_ld_scores_pos(self.h, None if p is None else _dp(p), float(radius), chp, int(bool(adjusted)),
                                         None if an is None else _dp(an), C_, _dp(l2), _dp(n)))
        l2 = l2[:M * C_].copy()
        return (l2 if annot is None else l2.reshape(M, C_)), n[:M].copy()

    def ld_last_passes(self):
        """gv_ld_last_passes: the passes over row groups the last LD call took (more than 1 only for ld_scores_pos over its budget)"""
        k = C.c_int(0)
        self._ck(self.L.gv_ld_last_passes(self.h, C.byref(k)))
        return k.value

    def ld_clump(self, pos, radius, p, p1, p2, r2, chrom=None):
        """gv_ld_clump: (index_of int64[M], n_index) -- the index marker of every marker's clump (itself for an index marker, -1 for a
        marker in no clump) over the band |pos_k - pos_j| <= radius on the same chromosome: index candidates p <= p1, members p <= p2,
        adjacency r^2 >= r2.  pos=None / p=None pass NULL (refused)."""
        M = self.M
        ps = None if pos is None else np.ascontiguousarray(pos, dtype=np.float64)
        pv = None if p is None else np.ascontiguousarray(p, dtype=np.float64)
        assert (ps is None or ps.size == M) and (pv is None or pv.size == M)
        out = np.full(max(M, 1), -1, dtype=np.int64)
        n = C.c_int64(0)
        ch, chp = self._chrom(chrom)
        self._ck(self.L.gv_ld_clump(self.h, None if ps is None else _dp(ps), float(radius), chp, None if pv is None else _dp(pv), float(p1),
                                    float(p2), float(r2), out.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n)))
        return out[:M].copy(), n.value

    def ld_clump_last(self):
        """gv_ld_clump_last and gv_ld_clump_seconds of the last ld_clump: the rounds of the selection, |E1|, |E2|, and the seconds of the
        block pass and of the selection"""
        k, n1, n2 = C.c_int(0), C.c_int64(0), C.c_int64(0)
        self._ck(self.L.gv_ld_clump_last(self.h, C.byref(k), C.byref(n1), C.byref(n2)))
        tb, ts = C.c_double(0.0), C.c_double(0.0)
        self._ck(self.L.gv_ld_clump_seconds(self.h, C.byref(tb), C.byref(ts)))
        return {"rounds": k.value, "n_e1": n1.value, "n_e2": n2.value, "block_seconds": tb.value, "select_seconds": ts.value}

    def ld_band(self, window, j0, nj, chrom=None):
        """gv_ld_band: nj x (2 * window + 1) correlations of the local markers [j0, j0 + nj); column window + d is r[j][j + d],
        0 outside the band"""
        nj_ = int(nj)
        out = np.zeros((max(nj_, 1), 2 * int(window) + 1))
        ch, chp = self._chrom(chrom)
        self._ck(self.L.gv_ld_band(self.h, int(window), chp, int(j0), nj_, _dp(out)))
        return out[:max(nj_, 0)]

    def set_ld_dosage(self, on):
        """gv_set_ld_dosage: 1 = ld_scores / ld_band / ld_info accept resident 8-bit dosage codes with the mask set (default 0)"""
        self._ck(self.L.gv_set_ld_dosage(self.h, int(on)))

    def get_ld_dosage(self):
        on = C.c_int(0)
        self._ck(self.L.gv_get_ld_dosage(self.h, C.byref(on)))
        return on.value

    def ld_info(self):
        st = LdStats()
        self._ck(self.L.gv_ld_info(self.h, C.byref(st)))
        return {"seconds": st.seconds, "block_pairs": st.block_pairs, "useful_macs": st.useful_macs, "scratch_bytes": st.scratch_bytes}

    def score_dev(self, xs, outs):
        """gv_score_dev: outs[j] = data::Ax(xs[j]) for every column, many columns per pass over the genotypes (xs M-space, outs N-space
        vectors; None in place of a list passes a NULL array)"""
        n = len(xs) if xs is not None else len(outs)

        def arr(vs):
            if vs is None:
                return None
            return (C.c_void_p * max(len(vs), 1))(*[None if v is None else v.h for v in vs])
        self._ck(self.L.gv_score_dev(self.h, n, arr(xs), arr(outs)))

    def score(self, W):
        """gv_score: W of shape (C, M) or (M,) on the host -> (C, 4 * mbytes), row j = data::Ax(W[j])"""
        W = np.ascontiguousarray(W, dtype=np.float64)
        if W.ndim == 1:
            W = W[None, :]
        assert W.ndim == 2 and W.shape[1] == self.M, (W.shape, self.M)
        out = np.empty((W.shape[0], 4 * self.mbytes))
        self._ck(self.L.gv_score(self.h, W.shape[0], _dp(W), _dp(out)))
        return out

    def score_info(self):
        """gv_score_info of the last score_dev / score as a dict; path is "kernel", "fallback" or None"""
        st = ScoreStats()
        self._ck(self.L.gv_score_info(self.h, C.byref(st)))
        return dict(path={SCORE_PATH_KERNEL: "kernel", SCORE_PATH_FALLBACK: "fallback"}.get(st.path), cols_per_pass=st.cols_per_pass,
                    ksegs=st.ksegs, min_cols=st.min_cols, columns=st.columns, passes=st.passes, scratch_bytes=int(st.scratch_bytes),
                    seconds=st.seconds)

    @staticmethod
    def _handles(vs):
        if vs is None:
            return None
        return (C.c_void_p * max(len(vs), 1))(*[None if v is None else v.h for v in vs])

    def atxm_dev(self, ps, outs):
        """gv_atxm_dev: outs[j] = data::ATx(ps[j]) for every column, many columns per pass over the genotypes (ps N-space, outs M-space
        vectors; None in place of a list passes a NULL array)"""
        n = len(ps) if ps is not None else len(outs)
        self._ck(self.L.gv_atxm_dev(self.h, n, self._handles(ps), self._handles(outs)))

    def atxm(self, Y):
        """gv_atxm: Y of shape (C, 4 * mbytes) or (4 * mbytes,) on the host -> (C, M), row j = data::ATx(Y[j])"""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[None, :]
        assert Y.ndim == 2 and Y.shape[1] == 4 * self.mbytes, (Y.shape, self.mbytes)
        out = np.empty((Y.shape[0], self.M))
        self._ck(self.L.gv_atxm(self.h, Y.shape[0], _dp(Y), _dp(out)))
        return out

    def atxm_info(self):
        """gv_atxm_info of the last atxm_dev / atxm / screen as a dict; path is "kernel", "fallback" or None"""
        st = AtxmStats()
        self._ck(self.L.gv_atxm_info(self.h, C.byref(st)))
        return dict(path={ATXM_PATH_KERNEL: "kernel", ATXM_PATH_FALLBACK: "fallback"}.get(st.path), cols_per_pass=st.cols_per_pass,
                    ksegs=st.ksegs, min_cols=st.min_cols, columns=st.columns, passes=st.passes, scratch_bytes=int(st.scratch_bytes),
                    seconds=st.seconds)

    def screen_dev(self, us, rs, ts=None, ps=None):
        """gv_screen_dev: prepared phenotype columns us (N-space) -> r, t, p per marker (M-space; ts and ps may be None)"""
        n = len(us) if us is not None else len(rs)
        self._ck(self.L.gv_screen_dev(self.h, n, self._handles(us), self._handles(rs), self._handles(ts), self._handles(ps)))

    def set_screen_dosage(self, on):
        """gv_set_screen_dosage: 1 = screen / screen_dev / screen_cov_set / screen_cov_dev / screen_cov accept resident dosage codes
        (8 or 16 bits, with or without missing entries, either route).  Default 0; it outlives the dataset"""
        self._ck(self.L.gv_set_screen_dosage(self.h, int(on)))

    def get_screen_dosage(self):
        on = C.c_int(0)
        self._ck(self.L.gv_get_screen_dosage(self.h, C.byref(on)))
        return on.value

    def screen_prepare(self, Y):
        """the prepared columns u of gv_screen_dev from raw phenotype columns Y of shape (C, N), NaN for NA: zero at the individuals the
        context's mask leaves out and at pad slots, centred over the phenotyped, scaled by sqrt((n - 1) / sum (y - mean)^2).  A NaN at
        an individual the mask keeps is refused: the NA pattern of every column must lie inside the mask."""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[None, :]
        assert Y.ndim == 2 and Y.shape[1] == self.N, (Y.shape, self.N)
        pres = np.ones(self.N, dtype=bool) if self._present is None else self._present
        n = int(pres.sum())
        if n < 3:
            raise GvError("screen: fewer than 3 individuals with a phenotype")
        U = np.zeros((Y.shape[0], 4 * self.mbytes))
        for c, y in enumerate(Y):
            if np.any(np.isnan(y[pres])):
                raise GvError("screen: column %d is NA at an individual the context's mask keeps (set the merged mask first)" % c)
            d = y[pres] - y[pres].sum() / n
            ss = float((d * d).sum())
            if not ss > 0:
                raise GvError("screen: column %d has no variance over the phenotyped individuals" % c)
            U[c, np.nonzero(pres)[0]] = d * np.sqrt((n - 1) / ss)
        return U

    def screen(self, Y, cols_per_call=64):
        """the marginal association screen of raw phenotype columns Y (C, N): (r, t, p), each of shape (C, M)"""
        U = self.screen_prepare(Y)
        out = [np.empty((U.shape[0], self.M)) for _ in range(3)]
        for j0 in range(0, U.shape[0], cols_per_call):
            blk = U[j0:j0 + cols_per_call]
            us = [self.vecN(u) for u in blk]
            res = [[self.vecM() for _ in blk] for _ in range(3)]
            try:
                self.screen_dev(us, *res)
                for k in range(3):
                    for j, v in enumerate(res[k]):
                        out[k][j0 + j] = v.download()
            finally:
                for v in us + res[0] + res[1] + res[2]:
                    v.free()
        return tuple(out)

    # ---- the covariate-adjusted screen (gv_screen_cov_*) -----------------------------------
    def screen_cov_set(self, Cov, K=None):
        """gv_screen_cov_set: Cov is a list of N-space vectors (used as they are) or raw covariate columns of shape (K, N) / (N,) on the
        host (uploaded, the call made, freed); None or an empty list is K = 0, the intercept alone.  K overrides the count the list
        implies (None in place of a list passes a NULL array)"""
        if Cov is None or (isinstance(Cov, (list, tuple)) and all(v is None or isinstance(v, Vec) for v in Cov)):
            k = (0 if Cov is None else len(Cov)) if K is None else K
            self._ck(self.L.gv_screen_cov_set(self.h, int(k), self._handles(Cov)))
            return
        A = np.ascontiguousarray(Cov, dtype=np.float64)
        if A.ndim == 1:
            A = A[None, :]
        assert A.ndim == 2 and A.shape[1] == self.N, (A.shape, self.N)
        vs = [self.vecN(self._padN(a)) for a in A]
        try:
            self._ck(self.L.gv_screen_cov_set(self.h, len(vs) if K is None else int(K), self._handles(vs)))
        finally:
            for v in vs:
                v.free()

    def _padN(self, a):
        out = np.zeros(4 * self.mbytes)
        out[:self.N] = a
        return out

    def screen_cov_dev(self, ys, rs, ts=None, ps=None, betas=None, ses=None, vif=50.0):
        """gv_screen_cov_dev: raw phenotype columns ys (N-space vectors) -> r, t, p, beta, se per marker (M-space vectors; all but rs may
        be None)"""
        n = len(ys) if ys is not None else len(rs)
        self._ck(self.L.gv_screen_cov_dev(self.h, n, self._handles(ys), float(vif), self._handles(rs), self._handles(ts), self._handles(ps),
                                          self._handles(betas), self._handles(ses)))

    def screen_cov(self, Y, Cov, vif=50.0, cols_per_call=64):
        """the covariate-adjusted screen of raw phenotype columns Y (C, N) given raw covariate columns Cov (K, N), or None for the
        intercept alone: dict r, t, p, beta, se, each of shape (C, M).  Values at the individuals the context's mask leaves out are
        ignored (NaN there is fine); Cov=False keeps the covariates of the last screen_cov_set"""
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim == 1:
            Y = Y[None, :]
        assert Y.ndim == 2 and Y.shape[1] == self.N, (Y.shape, self.N)
        if Cov is not False:
            self.screen_cov_set(Cov)
        names = ("r", "t", "p", "beta", "se")
        out = {k: np.empty((Y.shape[0], self.M)) for k in names}
        for j0 in range(0, Y.shape[0], cols_per_call):
            blk = Y[j0:j0 + cols_per_call]
            ys = [self.vecN(self._padN(y)) for y in blk]
            res = [[self.vecM() for _ in blk] for _ in names]
            try:
                self.screen_cov_dev(ys, *res, vif=vif)
                for k, name in enumerate(names):
                    for j, v in enumerate(res[k]):
                        out[name][j0 + j] = v.download()
            finally:
                for v in ys + [v for vs in res for v in vs]:
                    v.free()
        return out

    def screen_cov_info(self):
        """gv_screen_cov_info as a dict; K is None when no covariate state is cached"""
        st = ScreenCovStats()
        self._ck(self.L.gv_screen_cov_info(self.h, C.byref(st)))
        return dict(K=None if st.K < 0 else st.K, nu=st.nu, cached_bytes=int(st.cached_bytes), set_seconds_products=st.set_seconds_products,
                    set_seconds_panel=st.set_seconds_panel, set_seconds=st.set_seconds, columns=st.columns,
                    call_seconds_products=st.call_seconds_products, call_seconds_panel=st.call_seconds_panel,
                    call_seconds=st.call_seconds)

    def pca_dev(self, q0, us, tol, max_iter, k=None, L=None):
        """gv_pca_dev: the len(us) largest eigenpairs of the relationship matrix from the starting block q0 (N-space vectors, not
        modified) into us (N-space vectors).  Returns (eval, resid); k / L override the counts the lists imply (None in place of a
        list passes a NULL array)"""
        k = len(us) if k is None else k
        L = len(q0) if L is None else L
        ev, rs = np.full(max(k, 1), np.nan), np.full(max(k, 1), np.nan)
        self._ck(self.L.gv_pca_dev(self.h, int(k), int(L), self._handles(q0), float(tol), int(max_iter), self._handles(us), _dp(ev), _dp(rs)))
        return ev[:k], rs[:k]

    def pca_loadings_dev(self, us, ev, vs):
        """gv_pca_loadings_dev: vs[i] = c_i * ATx(us[i]), the right singular vectors of this rank's markers (M-space vectors)"""
        ev = np.ascontiguousarray(ev, dtype=np.float64)
        assert ev.size == len(us) == len(vs)
        self._ck(self.L.gv_pca_loadings_dev(self.h, len(us), self._handles(us), _dp(ev), self._handles(vs)))

    # ---- pairwise kinship (gv_king_*) ------------------------------------------------
    def _use(self, use):
        if use is None:
            return None, None
        u = np.ascontiguousarray(use, dtype=np.uint8)
        assert u.size == self.M, (u.size, self.M)
        return u, _up(u)

    def king_block(self, i0, ni, j0, nj, use=None):
        """gv_king_block: (kin[ni, nj] float64, counts[ni, nj, 5] int32 = nsnp, hethet, ibs0, het_i, het_j) of the individuals
        [i0, i0 + ni) x [j0, j0 + nj); use: M bytes, non-zero = the marker counts (None: every marker)"""
        ni_, nj_ = int(ni), int(nj)
        kin = np.zeros((max(ni_, 0), max(nj_, 0)))
        cnt = np.zeros((max(ni_, 0), max(nj_, 0), 5), dtype=np.int32)
        u, upt = self._use(use)
        self._ck(self.L.gv_king_block(self.h, upt, int(i0), ni_, int(j0), nj_, _dp(kin) if kin.size else None,
                                      cnt.ctypes.data_as(C.POINTER(C.c_int32)) if cnt.size else None))
        return kin, cnt

    def king_pairs_raw(self, cutoff, cap, use=None):
        """gv_king_pairs with the caller's cap: (n_found, i, j, kin, counts); the arrays hold the pairs only when n_found <= cap"""
        cap_ = int(cap)
        n = max(cap_, 1)
        pi, pj = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        kin, cnt = np.zeros(n), np.zeros((n, 5), dtype=np.int32)
        found = C.c_int64(-1)
        u, upt = self._use(use)
        i32p = C.POINTER(C.c_int32)
        self._ck(self.L.gv_king_pairs(self.h, upt, float(cutoff), cap_, pi.ctypes.data_as(i32p), pj.ctypes.data_as(i32p), _dp(kin),
                                      cnt.ctypes.data_as(i32p), C.byref(found)))
        return found.value, pi, pj, kin, cnt

    def king_pairs(self, cutoff, use=None, cap=None):
        """every pair i < j with kin >= cutoff in ascending (i, j): (i, j, kin, counts[., 5]).  cap: the first call's slots (default
        65536); one more call with the number found when they did not suffice"""
        cap_ = 65536 if cap is None else int(cap)
        found, pi, pj, kin, cnt = self.king_pairs_raw(cutoff, cap_, use)
        if found > cap_:
            cap_ = found
            found, pi, pj, kin, cnt = self.king_pairs_raw(cutoff, cap_, use)
            if found > cap_:
                raise GvError("king_pairs: %d pairs found with room for %d on the second call" % (found, cap_))
        return pi[:found].copy(), pj[:found].copy(), kin[:found].copy(), cnt[:found].copy()

    def king_info(self):
        """gv_king_info of the last king_block / king_pairs call as a dict"""
        st = KingStats()
        self._ck(self.L.gv_king_info(self.h, C.byref(st)))
        return dict(seconds=st.seconds, block_pairs=st.block_pairs, used_markers=st.used_markers, pairs=st.pairs,
                    useful_macs=st.useful_macs, scratch_bytes=st.scratch_bytes)

    # ---- standardised genetic relationship matrix (gv_grm_*) -------------------------
    def grm_weights(self, use=None):
        """gv_grm_weights: (mu[M], rs[M], n_used) of the pre-pass; a marker that does not count has mu = rs = 0"""
        mu, rs = np.zeros(max(self.M, 1)), np.zeros(max(self.M, 1))
        n = C.c_int64(-1)
        u, upt = self._use(use)
        self._ck(self.L.gv_grm_weights(self.h, upt, _dp(mu), _dp(rs), C.byref(n)))
        return mu[:self.M], rs[:self.M], n.value

    def grm_block(self, i0, ni, j0, nj, use=None):
        """gv_grm_block: (a[ni, nj] float64, m_common[ni, nj] int32) of the individuals [i0, i0 + ni) x [j0, j0 + nj); use: M bytes,
        non-zero = the marker is selected (None: every marker)"""
        ni_, nj_ = int(ni), int(nj)
        a = np.zeros((max(ni_, 0), max(nj_, 0)))
        mc = np.zeros((max(ni_, 0), max(nj_, 0)), dtype=np.int32)
        u, upt = self._use(use)
        self._ck(self.L.gv_grm_block(self.h, upt, int(i0), ni_, int(j0), nj_, _dp(a) if a.size else None,
                                     mc.ctypes.data_as(C.POINTER(C.c_int32)) if mc.size else None))
        return a, mc

    def grm_pairs_raw(self, cutoff, cap, use=None, diag=True):
        """gv_grm_pairs with the caller's cap: (n_found, i, j, a, m_common, diag, diag_m); the pair arrays hold the pairs only when
        n_found <= cap; diag and diag_m are None without diag"""
        cap_ = int(cap)
        n = max(cap_, 1)
        pi, pj = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        a, mc = np.zeros(n), np.zeros(n, dtype=np.int32)
        d, dm = (np.zeros(self.N), np.zeros(self.N, dtype=np.int32)) if diag else (None, None)
        found = C.c_int64(-1)
        u, upt = self._use(use)
        i32p = C.POINTER(C.c_int32)
        self._ck(self.L.gv_grm_pairs(self.h, upt, float(cutoff), cap_, pi.ctypes.data_as(i32p), pj.ctypes.data_as(i32p), _dp(a),
                                     mc.ctypes.data_as(i32p), _dp(d) if diag else None, dm.ctypes.data_as(i32p) if diag else None,
                                     C.byref(found)))
        return found.value, pi, pj, a, mc, d, dm

    def grm_pairs(self, cutoff, use=None, cap=None, diag=True):
        """every pair i < j with A_ij >= cutoff in ascending (i, j): (i, j, a, m_common, diag, diag_m).  cap: the first call's slots
        (default 65536); one more call with the number found when they did not suffice"""
        cap_ = 65536 if cap is None else int(cap)
        found, pi, pj, a, mc, d, dm = self.grm_pairs_raw(cutoff, cap_, use, diag)
        if found > cap_:
            cap_ = found
            found, pi, pj, a, mc, d, dm = self.grm_pairs_raw(cutoff, cap_, use, diag)
            if found > cap_:
                raise GvError("grm_pairs: %d pairs found with room for %d on the second call" % (found, cap_))
        return pi[:found].copy(), pj[:found].copy(), a[:found].copy(), mc[:found].copy(), d, dm

    def grm_info(self):
        """gv_grm_info of the last grm_weights / grm_block / grm_pairs call as a dict"""
        st = GrmStats()
        self._ck(self.L.gv_grm_info(self.h, C.byref(st)))
        return dict(seconds=st.seconds, block_pairs=st.block_pairs, counting_markers=st.counting_markers,
                    dropped_markers=st.dropped_markers, pairs=st.pairs, useful_macs=st.useful_macs, scratch_bytes=st.scratch_bytes,
                    passes=st.passes, blocks_computed=st.blocks_computed)

    # ---- GRM-times-panel product and Haseman-Elston regression (gv_grm_apply / gv_grm_he) ----
    def grm_apply(self, w, use=None, want=(True, True, True)):
        """gv_grm_apply: (g0, g1, g2), each N x C float64 (None where `want` is false), of the panel w (N x C, or N values: one
        column): gp = Gp w with G0 = 1, G1 = A, G2 = fl(A^2) off the diagonal and where M_ij > 0, 0 elsewhere"""
        w_ = np.ascontiguousarray(w, dtype=np.float64)
        if w_.ndim == 1:
            w_ = w_.reshape(-1, 1)
        if w_.ndim != 2 or w_.shape[0] != self.N:
            raise GvError("grm_apply: w must be N x C (N = %d), not %s" % (self.N, w_.shape))
        ncol = w_.shape[1]
        out = [np.zeros((self.N, max(ncol, 1))) if k else None for k in want]
        u, upt = self._use(use)
        self._ck(self.L.gv_grm_apply(self.h, upt, ncol, _dp(w_), *[_dp(o) if o is not None else None for o in out]))
        return tuple(out)

    def grm_he(self, y, use=None):
        """gv_grm_he: a record array (HE_DTYPE), one record per column of y (N x C, or N values: one trait; NaN = missing)"""
        y_ = np.ascontiguousarray(y, dtype=np.float64)
        if y_.ndim == 1:
            y_ = y_.reshape(-1, 1)
        if y_.ndim != 2 or y_.shape[0] != self.N:
            raise GvError("grm_he: y must be N x C (N = %d), not %s" % (self.N, y_.shape))
        ncol = y_.shape[1]
        res = (HeResult * max(ncol, 1))()
        u, upt = self._use(use)
        self._ck(self.L.gv_grm_he(self.h, upt, ncol, _dp(y_), res))
        return np.frombuffer(res, dtype=HE_DTYPE, count=ncol).copy()

    def pca_info(self):
        """gv_pca_info of the last pca_dev / pca as a dict"""
        st = PcaStats()
        self._ck(self.L.gv_pca_info(self.h, C.byref(st)))
        return dict(iterations=st.iterations, converged=st.converged, block=st.block, cols_atxm=st.cols_atxm, cols_score=st.cols_score,
                    scratch_bytes=int(st.scratch_bytes), seconds_products=st.seconds_products, seconds_panel=st.seconds_panel,
                    seconds=st.seconds)

    def pca(self, k, block=None, tol=1e-8, max_iter=100, seed=0, loadings=False, strict=True):
        """the k leading principal components of the resident genotypes: dict eval (k,), evec (k, N), resid (k,), info and, with
        loadings, loadings (k, M).  The starting block is `block` columns (default min(32, k + max(8, k))) of standard normals from
        numpy.random.default_rng(seed); an unconverged result raises GvError unless strict is false."""
        L = min(PCA_MAX_BLOCK, k + max(8, k)) if block is None else int(block)
        if k < 1 or L < k or L > PCA_MAX_BLOCK:
            raise GvError("pca: need 1 <= k <= block <= %d (k = %d, block = %d)" % (PCA_MAX_BLOCK, k, L))
        Q0 = np.zeros((L, 4 * self.mbytes))
        Q0[:, :self.N] = np.random.default_rng(seed).standard_normal((L, self.N))
        q0, us, vs = [self.vecN(q) for q in Q0], [self.vecN() for _ in range(k)], []
        try:
            ev, rs = self.pca_dev(q0, us, tol, max_iter)
            info = self.pca_info()
            if strict and not info["converged"]:
                raise GvError("pca: not converged after %d iterations (largest r / theta = %.3g, tol = %.3g)"
                              % (info["iterations"], float(np.max(rs / ev)), tol))
            out = dict(eval=ev, resid=rs, info=info, evec=np.stack([u.download()[:self.N] for u in us]))
            if loadings:
                vs = [self.vecM() for _ in range(k)]
                self.pca_loadings_dev(us, ev, vs)
                out["loadings"] = np.stack([v.download() for v in vs])
            return out
        finally:
            for v in q0 + us + vs:
                v.free()

    def ax2_dev(self, xa, xb, outa, outb):
        self._ck(self.L.gv_ax2_dev(self.h, xa.h, xb.h, outa.h, outb.h))

    def atx2_dev(self, pa, pb, outa, outb):
        self._ck(self.L.gv_atx2_dev(self.h, pa.h, pb.h, outa.h, outb.h))

    def cg_solve2(self, v_a, mu_start_a, v_b, tau, gam2, max_iter, mu_a, mu_b):
        """LMMSE solve (a) and Onsager probe solve (b) in lock-step; returns ((stats_a, relres_a), (stats_b, relres_b))."""
        sa, sb = CgStats(), CgStats()
        ra, rb = np.zeros(max(max_iter, 1)), np.zeros(max(max_iter, 1))
        self._ck(self.L.gv_cg_solve2(self.h, v_a.h, mu_start_a.h if mu_start_a is not None else None, v_b.h, tau, gam2,
                                     max_iter, mu_a.h, mu_b.h, C.byref(sa), C.byref(sb), _dp(ra), _dp(rb)))
        return (sa, ra[:sa.n_relres].copy()), (sb, rb[:sb.n_relres].copy())

    def cg_solve2x(self, v_a, mu_start_a, v_b, tau, gam2, max_iter, mu_a, mu_b, ride_x=None, ride_out=None, a_mu_a=None,
                   ata_mu_b=None, ata_mu_start_a=None, a_mu_start_a=None, ata_mu_a=None, ata_v_b=None, have_ata_v_b=False):
        """gv_cg_solve2 plus its pass-free by-products (include/gvamp.h: gv_cg_extras) and, when one of the last three
        arguments is given, the warm start whose initial residual costs no pass (gv_cg_warm, gv_cg_solve2w)."""
        sa, sb = CgStats(), CgStats()
        ra, rb = np.zeros(max(max_iter, 1)), np.zeros(max(max_iter, 1))
        ex = CgExtras(*[v.h if v is not None else None for v in (ride_x, ride_out, a_mu_a, ata_mu_b)])
        ms = mu_start_a.h if mu_start_a is not None else None
        if ata_mu_start_a is None and a_mu_start_a is None and ata_mu_a is None and ata_v_b is None:
            self._ck(self.L.gv_cg_solve2x(self.h, v_a.h, ms, v_b.h, tau, gam2, max_iter, mu_a.h, mu_b.h, C.byref(sa),
                                          C.byref(sb), _dp(ra), _dp(rb), C.byref(ex)))
        else:
            wm = CgWarm(*[v.h if v is not None else None for v in (ata_mu_start_a, a_mu_start_a, ata_mu_a, ata_v_b)],
                        int(bool(have_ata_v_b)))
            self._ck(self.L.gv_cg_solve2w(self.h, v_a.h, ms, v_b.h, tau, gam2, max_iter, mu_a.h, mu_b.h, C.byref(sa),
                                          C.byref(sb), _dp(ra), _dp(rb), C.byref(ex), C.byref(wm)))
        return (sa, ra[:sa.n_relres].copy()), (sb, rb[:sb.n_relres].copy())

    def denoise(self, r1, gam1, probs, vars_scaled, x1_out, d_out=None):
        probs = np.ascontiguousarray(probs, dtype=np.float64)
        vs = np.ascontiguousarray(vars_scaled, dtype=np.float64)
        sums = np.empty(2)
        self._ck(self.L.gv_denoise(self.h, r1.h, gam1, _dp(probs), _dp(vs), probs.size, x1_out.h,
                                   d_out.h if d_out is not None else None, _dp(sums)))
        return sums

    def prior_estep(self, r1, gam1, lam, omegas, vars_scaled):
        om = np.ascontiguousarray(omegas, dtype=np.float64)
        vs = np.ascontiguousarray(vars_scaled, dtype=np.float64)
        sums = np.empty(1 + 2 * (om.size - 1))
        self._ck(self.L.gv_prior_estep(self.h, r1.h, gam1, lam, _dp(om), _dp(vs), om.size, _dp(sums)))
        return sums

    def probit_denoise(self, p1, y, tau1, probit_var, z1_out, m_cov=None):
        sums = np.empty(2)
        if m_cov is None:
            self._ck(self.L.gv_probit_denoise(self.h, p1.h, y.h, tau1, probit_var, z1_out.h, _dp(sums)))
        else:
            self._ck(self.L.gv_probit_denoise_cov(self.h, p1.h, y.h, m_cov.h, tau1, probit_var, z1_out.h, _dp(sums)))
        return sums

    def huber_denoise(self, p1, y, tau1, deltaH, z1_out):
        """g1_Huber over the N individuals (--model robust): z1_out, and [sum dz1/dp1, sum (z1 - p1)^2]"""
        sums = np.empty(2)
        self._ck(self.L.gv_huber_denoise(self.h, p1.h, y.h, tau1, deltaH, z1_out.h, _dp(sums)))
        return sums

    def huber_delta(self, p1, y, tau1, grid):
        """the delta_H objective per grid value: mean expected Huber loss + log Z (--model robust)"""
        g = np.ascontiguousarray(grid, dtype=np.float64)
        obj = np.empty(g.size)
        self._ck(self.L.gv_huber_delta(self.h, p1.h, y.h, tau1, _dp(g), g.size, _dp(obj)))
        return obj

    def compute_people_statistics(self):
        """data::compute_people_statistics: (mave_people, msig_people, numb_people), 4*mbytes each."""
        n4 = 4 * self.mbytes
        a, b, c = np.empty(n4), np.empty(n4), np.empty(n4)
        self._ck(self.L.gv_people_stats(self.h, _dp(a), _dp(b), _dp(c)))
        return a, b, c

    def cg_solve_aat(self, v, mu_start, tau, gam2, max_iter, mu_out):
        st = CgStats()
        rr = np.zeros(max(max_iter, 1))
        self._ck(self.L.gv_cg_solve_aat(self.h, v.h, mu_start.h if mu_start is not None else None, tau, gam2, max_iter,
                                        mu_out.h, C.byref(st), _dp(rr)))
        return st, rr[:st.n_relres].copy()

    def cg_solve_aat2(self, v_a, mu_start_a, v_b, tau, gam2, max_iter, mu_a, at_mu_a, mu_b, aat_mu_a=None, ata_mu_b=None,
                      aat_mu_start_a=None, at_mu_start_a=None, accumulate_at_mu_a=False, ata_v_b=None, have_ata_v_b=False,
                      pre_x=None, pre_out=None, ride_x=None, ride_out=None, pre_scale=0.0):
        """gv_cg_solve_aat (system a, N-space) and the Onsager gv_cg_solve (system b, M-space) on shared passes; the last three
        arguments are gv_aat_warm (gv_cg_solve_aat2w): A A^T mu_start_a / A^T mu_start_a known from the previous call, and
        A^T mu_a accumulated inside the solve instead of by a closing pass."""
        sa, sb = CgStats(), CgStats()
        ra, rb = np.zeros(max(max_iter, 1)), np.zeros(max(max_iter, 1))
        wm = AatWarm(aat_mu_start_a.h if aat_mu_start_a is not None else None,
                     at_mu_start_a.h if at_mu_start_a is not None else None, int(bool(accumulate_at_mu_a)),
                     ata_v_b.h if ata_v_b is not None else None, int(bool(have_ata_v_b)),
                     *[q.h if q is not None else None for q in (pre_x, pre_out, ride_x, ride_out)], float(pre_scale))
        self._ck(self.L.gv_cg_solve_aat2w(self.h, v_a.h, mu_start_a.h if mu_start_a is not None else None, v_b.h, tau, gam2,
                                          max_iter, mu_a.h, at_mu_a.h, mu_b.h, C.byref(sa), C.byref(sb), _dp(ra), _dp(rb),
                                          aat_mu_a.h if aat_mu_a is not None else None,
                                          ata_mu_b.h if ata_mu_b is not None else None, C.byref(wm)))
        return (sa, ra[:sa.n_relres].copy()), (sb, rb[:sb.n_relres].copy())

    def pvals_calc_loco_pred(self, z1, y, x1_hat, chrom):
        """gv_pvals_loco_pred: (pvals[M], predictors[23, 4*mbytes])"""
        out = np.zeros(max(self.M, 1))
        pred = np.zeros((23, 4 * self.mbytes))
        ch = np.ascontiguousarray(chrom, dtype=np.int32)
        assert ch.size == self.M
        self._ck(self.L.gv_pvals_loco_pred(self.h, z1.h, y.h, x1_hat.h, ch.ctypes.data_as(C.POINTER(C.c_int)), _dp(out), _dp(pred)))
        return out[:self.M].copy(), pred

    def pvals_calc(self, z1, y, x1_hat, chrom=None):
        """data::pvals_calc (chrom None) / data::pvals_calc_LOCO on device handles; returns pvals[M]."""
        out = np.zeros(max(self.M, 1))
        if chrom is None:
            self._ck(self.L.gv_pvals_loo(self.h, z1.h, y.h, x1_hat.h, _dp(out)))
        else:
            ch = np.ascontiguousarray(chrom, dtype=np.int32)
            assert ch.size == self.M
            self._ck(self.L.gv_pvals_loco(self.h, z1.h, y.h, x1_hat.h, ch.ctypes.data_as(C.POINTER(C.c_int)), _dp(out)))
        return out[:self.M].copy()

    def assoc_calc(self, z1, y, x1_hat, chrom=None, want_pred=False):
        """gv_assoc_loo (chrom None) / gv_assoc_loco on device handles: the whole per-marker test, a dict of beta, se, t, p (M
        each); beta is the effect per unit of the standardised column.  want_pred (LOCO): also the predictors[23, 4*mbytes]."""
        res = {k: np.zeros(max(self.M, 1)) for k in ("beta", "se", "t", "p")}
        out = AssocOut(*[_dp(res[k]) for k in ("beta", "se", "t", "p")])
        if chrom is None:
            assert not want_pred, "the chromosome predictors belong to the LOCO test"
            self._ck(self.L.gv_assoc_loo(self.h, z1.h, y.h, x1_hat.h, C.byref(out)))
            return {k: v[:self.M].copy() for k, v in res.items()}
        ch = np.ascontiguousarray(chrom, dtype=np.int32)
        assert ch.size == self.M
        pred = np.zeros((23, 4 * self.mbytes)) if want_pred else None
        self._ck(self.L.gv_assoc_loco(self.h, z1.h, y.h, x1_hat.h, ch.ctypes.data_as(C.POINTER(C.c_int)), C.byref(out),
                                      _dp(pred) if want_pred else None))
        res = {k: v[:self.M].copy() for k, v in res.items()}
        return (res, pred) if want_pred else res

    def allreduce_host(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        self._ck(self.L.gv_allreduce_host(self.h, _dp(a), a.size))
        return a

    # ---- communicator / instrumentation --------------------------------------------------------------------
    def comm_init(self, nranks, rank, uid):
        buf = (C.c_ubyte * 128).from_buffer_copy(uid) if uid is not None else None
        self._ck(self.L.gv_comm_init(self.h, nranks, rank, buf))

    def comm_init_local(self, group, nranks, rank):
        self._ck(self.L.gv_comm_init_local(self.h, group, nranks, rank))

    def comm_init_callback(self, nranks, rank, allreduce):
        """gv_comm_init_callback: `allreduce(a)` sums the float64 numpy array `a` in place over the ranks (e.g.
        torch.distributed.all_reduce over gloo on torch.from_numpy(a))."""
        def _cb(_user, buf, n):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(n,)))
                return 0
            except Exception:          # no exception may cross the C ABI
                import traceback
                traceback.print_exc()
                return 1
        self._cb_keep = ALLREDUCE_FN(_cb)          # keep the trampoline alive as long as the context
        self._ck(self.L.gv_comm_init_callback(self.h, nranks, rank, self._cb_keep, None))

    def comm_share(self, owner):
        """gv_comm_share: join the communicator another Shard of this process already holds"""
        self._ck(self.L.gv_comm_share(self.h, owner.h))
        if getattr(owner, "_cb_keep", None) is not None:
            self._cb_keep = owner._cb_keep

    def set_overlap(self, tiles):
        self._ck(self.L.gv_set_overlap(self.h, tiles))

    def force_multi(self, transport=1, delay_us=0):
        """gv_debug_force_multi (test hook): this one-rank shard takes the sharded branches over an in-stream exchange
        (1 loop-back with poisoning, 2 the 1-rank RCCL communicator, 3 both; 0 = off)."""
        self._ck(self.L.gv_debug_force_multi(self.h, transport, delay_us))

    def set_timing(self, on):
        self._ck(self.L.gv_set_timing(self.h, int(on)))

    def counters(self, reset=False):
        c = Counters()
        self._ck(self.L.gv_get_counters(self.h, C.byref(c)))
        if reset:
            self._ck(self.L.gv_reset_counters(self.h))
        return dict(n_ax=c.n_ax, n_atx=c.n_atx, ms_ax=c.ms_ax, ms_atx=c.ms_atx, ms_allreduce=c.ms_allreduce,
                    n_ax_kernel=c.n_ax_kernel, n_atx_kernel=c.n_atx_kernel, ms_ax_kernel=c.ms_ax_kernel,
                    ms_atx_kernel=c.ms_atx_kernel, n_ax_pass=c.n_ax_pass, n_atx_pass=c.n_atx_pass,
                    n_allreduce=c.n_allreduce)

    def ingest_info(self):
        """(seconds allocating the resident layouts, seconds filling them) of the last ingest"""
        a, f = C.c_double(), C.c_double()
        self._ck(self.L.gv_ingest_info(self.h, C.byref(a), C.byref(f)))
        return a.value, f.value

    def ingest_stats(self):
        """gv_ingest_info2 of the last ingest as a dict"""
        st = IngestStats()
        self._ck(self.L.gv_ingest_info2(self.h, C.byref(st)))
        return {"alloc_s": st.alloc_seconds, "fill_s": st.fill_seconds, "overlap_s": st.overlap_seconds,
                "resident_GB": st.resident_bytes / 1e9, "layout": st.layout, "expected_passes": st.expected_passes}

    def set_expected_passes(self, passes):
        self._ck(self.L.gv_set_expected_passes(self.h, int(passes)))

    def tune_info(self):
        """(seconds spent picking the decompositions, source: 'pending' / 'model' / 'measured' / 'cache' / 'fixed' / 'builtin')"""
        sec, src = C.c_double(), C.c_int()
        self._ck(self.L.gv_tune_info(self.h, C.byref(sec), C.byref(src)))
        return sec.value, {-1: "pending", 0: "model", 1: "measured", 2: "cache", 3: "fixed", 4: "builtin"}[src.value]

    def decomp(self):
        """work decomposition per streaming-kernel class (gv_get_decomp)"""
        d = (DecompInfo * 4)()
        self._ck(self.L.gv_get_decomp(self.h, d))
        names = ("atx", "atx2", "ax", "ax2")
        return {n: (({"balanced_cells": int(x.balanced_cells)} | ({"whole_quads": int(x.whole_quads)} if x.whole_quads > 0 else {}))
                    if x.balanced_cells > 0 else ({"ks": x.ks, "taper": round(float(x.taper), 2)} | ({"geo": round(float(x.geo), 2)} if x.geo > 0 else {})))
                | ({"wgs_per_cu": 2} if x.wgs_per_cu == 2 else {}) | ({"xcd_skew": round(float(x.xcd_skew), 3)} if x.xcd_skew != 0 else {})
                | {"prio": x.prio, "tuned": bool(x.tuned)}
                for n, x in zip(names, d)}

    def set_decomp(self, cls, ks=1, balanced_cells=0, whole_quads=0, prio=0, taper=0.0, geo=0.0, wgs_per_cu=0, xcd_skew=0.0):
        """pins the decomposition of one streaming-kernel class (gv_set_decomp); cls: 0 atx, 1 atx2, 2 ax, 3 ax2 or its name"""
        if isinstance(cls, str):
            cls = ("atx", "atx2", "ax", "ax2").index(cls)
        d = DecompInfo(ks, balanced_cells, prio, taper, 0, whole_quads, geo, wgs_per_cu, xcd_skew)
        self._ck(self.L.gv_set_decomp(self.h, cls, C.byref(d)))

    def synchronize(self):
        self._ck(self.L.gv_synchronize(self.h))

    def copy_bandwidth(self, nbytes=1 << 30, reps=10):
        out = C.c_double()
        self._ck(self.L.gv_copy_bandwidth(self.h, nbytes, reps, C.byref(out)))
        return out.value

    def read_bandwidth(self, nbytes=1 << 30, reps=5):
        """read-only stream probe over the resident stripes (or a scratch buffer): GB/s"""
        out = C.c_double()
        self._ck(self.L.gv_read_bandwidth(self.h, nbytes, reps, C.byref(out)))
        return out.value
