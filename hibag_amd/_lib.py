"""ctypes binding of ``libhibag_hip.so`` (C ABI: ``include/hibag_hip.h``).

The library is the product; this module only declares its prototypes and turns
its error codes into exceptions.  There is no fallback: if the shared object is
missing, or there is no MI355X, compute entry points raise.
"""

from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# HIBAG_HIP_LIBRARY selects another build of the same library (tuning experiments)
LIB_PATH = os.environ.get("HIBAG_HIP_LIBRARY") or os.path.join(CSRC, "libhibag_hip.so")

K_PACK, K_TOTAL, K_ACCUM, K_FINISH, K_COUNT = 0, 1, 2, 3, 4
KERNEL_NAMES = {K_PACK: "pack", K_TOTAL: "total", K_ACCUM: "accum", K_FINISH: "finish"}

EXPORTS = [
    "hibag_hip_abi_version", "hibag_hip_last_error", "hibag_hip_device_count", "hibag_hip_set_device", "hibag_hip_get_device",
    "hibag_hip_set_kernel_target", "hibag_hip_model_new", "hibag_hip_model_add_classifier",
    "hibag_hip_model_add_classifier_packed", "hibag_hip_model_finalize", "hibag_hip_model_free",
    "hibag_hip_model_n_hla", "hibag_hip_model_n_snp", "hibag_hip_model_n_classifier",
    "hibag_hip_model_pair_evals", "hibag_hip_model_stored_cells", "hibag_hip_model_second_pass_pairs", "hibag_hip_model_mutation_table", "hibag_hip_predict",
    "hibag_hip_predict_device", "hibag_hip_model_set_snp_weights", "hibag_hip_predict_partial_device",
    "hibag_hip_finish_device", "hibag_hip_set_timing", "hibag_hip_get_timing", "hibag_hip_reset_timing",
    "hibag_hip_gpu_ext_proc", "hibag_hip_bed_flag", "hibag_hip_conv_bed", "hibag_hip_predict_bed", "hibag_hip_predict_mapped", "hibag_hip_predict_mapped_device",
    "hibag_hip_predict_snp_major", "hibag_hip_predict_snp_major_device",
    "hibag_hip_trainer_new", "hibag_hip_trainer_free", "hibag_hip_trainer_set_rng", "hibag_hip_trainer_set_seed",
    "hibag_hip_trainer_new_classifiers", "hibag_hip_trainer_n_classifier", "hibag_hip_trainer_classifier_dims",
    "hibag_hip_trainer_classifier_get", "hibag_hip_trainer_set_threads", "hibag_hip_trainer_threads", "hibag_hip_trainer_set_em_mode",
    "hibag_hip_trainer_set_shared", "hibag_hip_train_set_thread_budget", "hibag_hip_train_combine_stats", "hibag_hip_train_combine_times",
    "hibag_hip_model_status", "hibag_hip_model_clear_status", "hibag_hip_model_handover_faults",
    "hibag_hip_test_inject_handover_fault", "hibag_hip_model_engine", "hibag_hip_model_replicate",
    "hibag_hip_multi_slice", "hibag_hip_predict_multi", "hibag_hip_model_device",
    "hibag_hip_shard_bounds", "hibag_hip_model_shard", "hibag_hip_model_batch_limit", "hibag_hip_shard_group_new",
    "hibag_hip_shard_group_free", "hibag_hip_shard_group_ranks", "hibag_hip_shard_group_allreduces", "hibag_hip_rccl_version",
    "hibag_hip_shard_group_predict", "hibag_hip_predict_multi_sharded", "hibag_hip_measure_issue_costs",
    "hibag_hip_test_time_avg_prob", "hibag_hip_test_read_diag", "hibag_hip_plugin_degraded_calls", "hibag_hip_predict_oob",
    "hibag_hip_ld_geno_new", "hibag_hip_ld_geno_free", "hibag_hip_ld_snp_counts", "hibag_hip_ld_matrix", "hibag_hip_ld_gram_ms",
    "hibag_hip_ld_hla", "hibag_hip_model_distance", "hibag_hip_model_distance_ms",
    "hibag_hip_merge_plan_new", "hibag_hip_merge_plan_free", "hibag_hip_merge_device", "hibag_hip_predict_merge",
    "hibag_hip_predict_merge_bed", "hibag_hip_predict_prefix", "hibag_hip_predict_prefix_ms",
    "hibag_hip_predict_topk", "hibag_hip_predict_topk_device", "hibag_hip_predict_topk_mapped",
    "hibag_hip_predict_topk_snp_major", "hibag_hip_predict_topk_bed",
    "hibag_hip_cohort_new", "hibag_hip_cohort_from_bed", "hibag_hip_cohort_free", "hibag_hip_cohort_device",
    "hibag_hip_cohort_n_samp", "hibag_hip_cohort_n_snp", "hibag_hip_cohort_bytes", "hibag_hip_cohort_snp_counts",
    "hibag_hip_predict_cohort", "hibag_hip_predict_topk_cohort", "hibag_hip_predict_masked",
    "hibag_hip_test_build_eval_batch", "hibag_hip_test_em_fit", "hibag_hip_test_em_layout", "hibag_hip_trainer_em_counts",
    "hibag_hip_predict_draw", "hibag_hip_predict_draw_device", "hibag_hip_predict_draw_mapped",
    "hibag_hip_predict_draw_snp_major", "hibag_hip_predict_draw_bed", "hibag_hip_predict_draw_cohort",
    "hibag_hip_groups_create", "hibag_hip_groups_free", "hibag_hip_groups_levels", "hibag_hip_groups_tile",
    "hibag_hip_predict_groups", "hibag_hip_predict_groups_device", "hibag_hip_predict_groups_mapped",
    "hibag_hip_predict_groups_snp_major", "hibag_hip_predict_groups_bed", "hibag_hip_predict_groups_cohort",
    "hibag_hip_predict_given", "hibag_hip_predict_given_device", "hibag_hip_predict_given_mapped",
    "hibag_hip_predict_given_snp_major", "hibag_hip_predict_given_bed", "hibag_hip_predict_given_cohort",
    "hibag_hip_predict_family", "hibag_hip_predict_family_device", "hibag_hip_predict_family_mapped",
    "hibag_hip_predict_family_snp_major",
    "hibag_hip_assoc_new", "hibag_hip_assoc_free", "hibag_hip_assoc_n_tests", "hibag_hip_assoc_observed",
    "hibag_hip_assoc_permute", "hibag_hip_assoc_labels",
    "hibag_hip_assoc_n_kept", "hibag_hip_assoc_feature_rows", "hibag_hip_assoc_glm",
    "hibag_hip_assoc_glm_sets", "hibag_hip_assoc_row_sums",
    "hibag_hip_assoc_glm_terms", "hibag_hip_assoc_row_gram",
    "hibag_hip_assoc_cox", "hibag_hip_assoc_cox_segment",
    "hibag_hip_assoc_quant_new", "hibag_hip_assoc_quant_free", "hibag_hip_assoc_quant_classes", "hibag_hip_assoc_quant_observed",
    "hibag_hip_assoc_quant_permute", "hibag_hip_assoc_quant_perm_rows", "hibag_hip_assoc_quant_gram_ms",
    "hibag_hip_assoc_score_new", "hibag_hip_assoc_score_free", "hibag_hip_assoc_score_base", "hibag_hip_assoc_score_sets",
    "hibag_hip_assoc_score_observed", "hibag_hip_assoc_score_n_df", "hibag_hip_assoc_score_resample", "hibag_hip_assoc_score_signs",
    "hibag_hip_assoc_score_ms", "hibag_hip_assoc_rscore_sets",
    "hibag_hip_haplo_new", "hibag_hip_haplo_free", "hibag_hip_haplo_dims", "hibag_hip_haplo_fit", "hibag_hip_haplo_calls",
    "hibag_hip_haplo_dosage",
    "hibag_hip_oob_knock_variants", "hibag_hip_oob_knock",
    "hibag_hip_test_layout_plan", "hibag_hip_test_layout_count", "hibag_hip_test_layout_get", "hibag_hip_test_layout_free",
    "hibag_hip_test_set_chunking", "hibag_hip_test_last_launch", "hibag_hip_test_plan_total", "hibag_hip_test_plan_accum",
]
TOPK_MAX = 16      # HIBAG_HIP_TOPK_MAX of include/hibag_hip.h
DRAW_MAX = 64      # HIBAG_HIP_DRAW_MAX
GROUPS_MAX_PART = 512        # HIBAG_HIP_GROUPS_MAX_PART
GROUPS_MAX_LEVELS = 4096     # HIBAG_HIP_GROUPS_MAX_LEVELS


class LaunchInfo(C.Structure):
    """``hibag_hip_launch_info`` of include/hibag_hip.h: what passes 1 and 2 launched, or would launch."""
    _fields_ = [(name, C.c_int32) for name in (
        "p1_launches", "p1_kernel", "p1_n", "p1_slots", "p1_k", "p1_n_whole", "p1_rest", "p1_stride", "p1_grid", "p1_many",
        "p1_walk", "p1_store", "p1_vote", "p2_launches", "p2_kernel", "p2_nx", "p2_sx", "p2_k", "p2_n_whole", "p2_grid")]

    def as_dict(self) -> dict:
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class HibagHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(message or f"libhibag_hip error {code}")
        self.code = code


def build(force: bool = False) -> str:
    """Compile the HIP library for gfx950 (``make -C hibag_amd/csrc``)."""
    cmd = ["make", "-C", CSRC, "-s", "-j2"] + (["-B"] if force else [])
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    """Load the library; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C hibag_amd/csrc`.  hibag_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, dbl = C.c_void_p, C.c_int, C.c_int64, C.c_double
    L.hibag_hip_abi_version.restype = i32
    L.hibag_hip_last_error.restype = C.c_char_p
    L.hibag_hip_device_count.restype = i32
    L.hibag_hip_set_device.argtypes = [i32]
    L.hibag_hip_set_kernel_target.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
    L.hibag_hip_model_new.argtypes = [i32, i32]
    L.hibag_hip_model_new.restype = vp
    L.hibag_hip_model_add_classifier.argtypes = [vp, i32, vp, i32, vp, vp, C.POINTER(C.c_char_p)]
    L.hibag_hip_model_add_classifier_packed.argtypes = [vp, i32, vp, i32, vp, vp, vp]
    L.hibag_hip_model_set_snp_weights.argtypes = [vp, vp]
    L.hibag_hip_model_finalize.argtypes = [vp]
    L.hibag_hip_model_free.argtypes = [vp]
    L.hibag_hip_model_free.restype = None
    for f in (L.hibag_hip_model_n_hla, L.hibag_hip_model_n_snp, L.hibag_hip_model_n_classifier, L.hibag_hip_model_device):
        f.argtypes = [vp]
        f.restype = i32
    L.hibag_hip_model_pair_evals.argtypes = [vp]
    L.hibag_hip_model_pair_evals.restype = i64
    L.hibag_hip_model_stored_cells.argtypes = [vp]
    L.hibag_hip_model_stored_cells.restype = i64
    L.hibag_hip_model_second_pass_pairs.argtypes = [vp]
    L.hibag_hip_model_second_pass_pairs.restype = i64
    L.hibag_hip_model_mutation_table.argtypes = [vp, vp]
    L.hibag_hip_predict.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_predict_oob.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    if hasattr(L, "hibag_hip_predict_masked"):        # (absent from an older build selected with HIBAG_HIP_LIBRARY, as below)
        L.hibag_hip_predict_masked.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "hibag_hip_oob_knock"):             # (likewise)
        L.hibag_hip_oob_knock_variants.argtypes = [vp, C.POINTER(i32)]
        L.hibag_hip_oob_knock.argtypes = [vp, vp, i32, vp, vp, dbl, vp, vp, vp, vp]
    L.hibag_hip_predict_prefix.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp]
    L.hibag_hip_predict_prefix_ms.argtypes = [vp, C.POINTER(dbl)]
    L.hibag_hip_predict_topk.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
    L.hibag_hip_predict_topk_device.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
    L.hibag_hip_predict_topk_mapped.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp]
    L.hibag_hip_predict_topk_snp_major.argtypes = [vp, vp, C.c_size_t, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp]
    L.hibag_hip_predict_topk_bed.argtypes = [vp, C.c_char_p, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp]
    if hasattr(L, "hibag_hip_predict_draw"):          # (absent from an older build selected with HIBAG_HIP_LIBRARY)
        u64 = C.c_uint64
        L.hibag_hip_predict_draw.argtypes = [vp, vp, i32, i32, i32, u64, i64, vp, vp, vp, vp]
        L.hibag_hip_predict_draw_device.argtypes = [vp, vp, i32, i32, i32, u64, i64, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_draw_mapped.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, u64, i64, vp, vp, vp, vp]
        L.hibag_hip_predict_draw_snp_major.argtypes = [vp, vp, C.c_size_t, i32, i32, vp, vp, i32, i32, u64, i64, vp, vp, vp, vp]
        L.hibag_hip_predict_draw_bed.argtypes = [vp, C.c_char_p, i32, i32, vp, vp, i32, i32, u64, i64, vp, vp, vp, vp]
        L.hibag_hip_predict_draw_cohort.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, u64, i64, vp, vp, vp, vp]
    if hasattr(L, "hibag_hip_groups_create"):         # (absent from an older build selected with HIBAG_HIP_LIBRARY)
        L.hibag_hip_groups_create.argtypes = [vp, i32, vp, C.POINTER(vp)]
        L.hibag_hip_groups_free.argtypes = [vp]
        L.hibag_hip_groups_free.restype = None
        L.hibag_hip_groups_levels.argtypes = [vp, vp]
        L.hibag_hip_groups_tile.argtypes = [vp, C.POINTER(i32)]
        L.hibag_hip_predict_groups.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_groups_device.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_groups_mapped.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_groups_snp_major.argtypes = [vp, vp, C.c_size_t, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_groups_bed.argtypes = [vp, C.c_char_p, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_groups_cohort.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "hibag_hip_predict_given"):         # (absent from an older build selected with HIBAG_HIP_LIBRARY)
        L.hibag_hip_predict_given.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_given_device.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_given_mapped.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_given_snp_major.argtypes = [vp, vp, C.c_size_t, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_given_bed.argtypes = [vp, C.c_char_p, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_given_cohort.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "hibag_hip_predict_family"):        # (absent from an older build selected with HIBAG_HIP_LIBRARY)
        L.hibag_hip_predict_family.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_family_device.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_family_mapped.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_family_snp_major.argtypes = [vp, vp, C.c_size_t, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "hibag_hip_assoc_new"):             # (absent from an older build selected with HIBAG_HIP_LIBRARY)
        L.hibag_hip_assoc_new.argtypes = [vp, vp, vp, i32, i32, vp, i32, i32]
        L.hibag_hip_assoc_new.restype = vp
        L.hibag_hip_assoc_free.argtypes = [vp]
        L.hibag_hip_assoc_free.restype = None
        L.hibag_hip_assoc_n_tests.argtypes = [vp]
        L.hibag_hip_assoc_observed.argtypes = [vp, vp, vp]
        L.hibag_hip_assoc_permute.argtypes = [vp, C.c_uint64, C.c_uint64, i64, vp, vp]
        L.hibag_hip_assoc_labels.argtypes = [vp, C.c_uint64, C.c_uint64, i32, vp]
    if hasattr(L, "hibag_hip_assoc_glm"):
        L.hibag_hip_assoc_n_kept.argtypes = [vp]
        L.hibag_hip_assoc_feature_rows.argtypes = [vp, i32, i32, vp]
        L.hibag_hip_assoc_glm.argtypes = [vp, vp, i32, vp, i32, C.c_double, vp, vp, vp, vp, vp]
    if hasattr(L, "hibag_hip_assoc_glm_sets"):
        L.hibag_hip_assoc_glm_sets.argtypes = [vp, vp, vp, i32, vp, i32, vp, i32, C.c_double, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_assoc_row_sums.argtypes = [vp, vp]
    if hasattr(L, "hibag_hip_assoc_glm_terms"):
        L.hibag_hip_assoc_glm_terms.argtypes = [vp, vp, i32, vp, i32, vp, i32, C.c_double, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_assoc_row_gram.argtypes = [vp, i32, i32, vp]
    if hasattr(L, "hibag_hip_assoc_cox"):
        L.hibag_hip_assoc_cox.argtypes = [vp, vp, vp, i32, i32, i32, C.c_double, vp, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_assoc_cox_segment.argtypes = [i32, C.POINTER(i32), C.POINTER(i32)]
    if hasattr(L, "hibag_hip_assoc_quant_new"):
        L.hibag_hip_assoc_quant_new.argtypes = [vp, vp, vp, i32]
        L.hibag_hip_assoc_quant_new.restype = vp
        L.hibag_hip_assoc_quant_free.argtypes = [vp]
        L.hibag_hip_assoc_quant_free.restype = None
        L.hibag_hip_assoc_quant_classes.argtypes = [vp, vp, vp, vp, vp]
        L.hibag_hip_assoc_quant_observed.argtypes = [vp, vp, vp, vp, vp, vp]
        L.hibag_hip_assoc_quant_permute.argtypes = [vp, C.c_uint64, C.c_uint64, i64, vp, vp]
        L.hibag_hip_assoc_quant_perm_rows.argtypes = [vp, C.c_uint64, C.c_uint64, i32, vp]
        L.hibag_hip_assoc_quant_gram_ms.argtypes = [vp, C.POINTER(dbl)]
    if hasattr(L, "hibag_hip_assoc_score_new"):
        L.hibag_hip_assoc_score_new.argtypes = [vp, vp, i32, vp, i32, C.c_double]
        L.hibag_hip_assoc_score_new.restype = vp
        L.hibag_hip_assoc_score_free.argtypes = [vp]
        L.hibag_hip_assoc_score_free.restype = None
        L.hibag_hip_assoc_score_base.argtypes = [vp, vp, vp, vp, vp, vp]
        L.hibag_hip_assoc_score_sets.argtypes = [vp, vp, vp, i32, vp, vp, vp]
        L.hibag_hip_assoc_score_observed.argtypes = [vp, vp, vp, vp, vp]
        L.hibag_hip_assoc_score_n_df.argtypes = [vp]
        L.hibag_hip_assoc_score_resample.argtypes = [vp, C.c_uint64, C.c_uint64, i64, vp, vp]
        L.hibag_hip_assoc_score_signs.argtypes = [vp, C.c_uint64, C.c_uint64, i32, vp]
        L.hibag_hip_assoc_score_ms.argtypes = [vp, vp]
    if hasattr(L, "hibag_hip_assoc_rscore_sets"):
        L.hibag_hip_assoc_rscore_sets.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp]
    if hasattr(L, "hibag_hip_haplo_new"):
        L.hibag_hip_haplo_new.argtypes = [i32, i32, i32, vp, vp, vp, i32, i32]
        L.hibag_hip_haplo_new.restype = vp
        L.hibag_hip_haplo_free.argtypes = [vp]
        L.hibag_hip_haplo_free.restype = None
        L.hibag_hip_haplo_dims.argtypes = [vp, vp, vp, vp, vp, vp]
        L.hibag_hip_haplo_fit.argtypes = [vp, i32, dbl, vp, vp, vp, vp, vp]
        L.hibag_hip_haplo_calls.argtypes = [vp, vp, vp, vp, vp]
    if hasattr(L, "hibag_hip_haplo_dosage"):
        L.hibag_hip_haplo_dosage.argtypes = [vp, vp, i32, vp]
    if hasattr(L, "hibag_hip_cohort_new"):
        # (an older build selected with HIBAG_HIP_LIBRARY, e.g. the parent commit's for a baseline timing, lacks the cohort
        # entries: everything else still binds, and a call that needs them fails with AttributeError)
        L.hibag_hip_cohort_new.argtypes = [vp, i32, C.c_size_t, i32, i32, vp, i32]
        L.hibag_hip_cohort_new.restype = vp
        L.hibag_hip_cohort_from_bed.argtypes = [C.c_char_p, i32, i32, vp, i32]
        L.hibag_hip_cohort_from_bed.restype = vp
        L.hibag_hip_cohort_free.argtypes = [vp]
        L.hibag_hip_cohort_free.restype = None
        for f in (L.hibag_hip_cohort_device, L.hibag_hip_cohort_n_samp, L.hibag_hip_cohort_n_snp):
            f.argtypes = [vp]
            f.restype = i32
        L.hibag_hip_cohort_bytes.argtypes = [vp]
        L.hibag_hip_cohort_bytes.restype = i64
        L.hibag_hip_cohort_snp_counts.argtypes = [vp, vp, vp]
        L.hibag_hip_predict_cohort.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_predict_topk_cohort.argtypes = [vp, vp, i32, i32, vp, vp, i32, i32, vp, vp, vp, vp]
    L.hibag_hip_ld_geno_new.argtypes = [vp, i32, i32, i32]
    L.hibag_hip_ld_geno_new.restype = vp
    L.hibag_hip_ld_geno_free.argtypes = [vp]
    L.hibag_hip_ld_geno_free.restype = None
    L.hibag_hip_ld_snp_counts.argtypes = [vp, vp, vp]
    L.hibag_hip_ld_matrix.argtypes = [vp, vp, i32, vp, C.POINTER(i32)]
    L.hibag_hip_ld_gram_ms.argtypes = [vp, C.POINTER(dbl)]
    L.hibag_hip_ld_hla.argtypes = [vp, vp, vp, i32, vp, vp]
    L.hibag_hip_model_distance.argtypes = [vp, vp, vp]
    L.hibag_hip_model_distance_ms.argtypes = [vp, C.POINTER(dbl)]
    L.hibag_hip_merge_plan_new.argtypes = [i32, vp, C.POINTER(vp), i32, i32]
    L.hibag_hip_merge_plan_new.restype = vp
    L.hibag_hip_merge_plan_free.argtypes = [vp]
    L.hibag_hip_merge_plan_free.restype = None
    L.hibag_hip_merge_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), vp, i32, i32, vp, vp, vp, vp, vp, vp, C.c_size_t, vp]
    L.hibag_hip_predict_merge.argtypes = [vp, C.POINTER(vp), vp, i32, C.c_size_t, i32, i32, C.POINTER(vp), C.POINTER(vp), i32,
                                          vp, i32, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_predict_merge_bed.argtypes = [vp, C.POINTER(vp), C.c_char_p, i32, i32, C.POINTER(vp), C.POINTER(vp), i32,
                                              vp, i32, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_predict_device.argtypes = [vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_predict_partial_device.argtypes = [vp, vp, i32, vp, vp]
    L.hibag_hip_finish_device.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_set_timing.argtypes = [vp, i32]
    L.hibag_hip_get_timing.argtypes = [vp, i32, C.POINTER(dbl), C.POINTER(i64)]
    L.hibag_hip_reset_timing.argtypes = [vp]
    L.hibag_hip_gpu_ext_proc.restype = vp
    L.hibag_hip_trainer_new.argtypes = [i32, i32, vp, i32, vp, vp]
    L.hibag_hip_trainer_new.restype = vp
    L.hibag_hip_trainer_free.argtypes = [vp]
    L.hibag_hip_trainer_free.restype = None
    L.hibag_hip_trainer_set_rng.argtypes = [vp, vp, vp]
    L.hibag_hip_trainer_set_seed.argtypes = [vp, C.c_uint32]
    L.hibag_hip_trainer_new_classifiers.argtypes = [vp, i32, i32, i32, i32, i32]
    L.hibag_hip_trainer_n_classifier.argtypes = [vp]
    L.hibag_hip_trainer_set_threads.argtypes = [vp, i32]
    L.hibag_hip_trainer_threads.argtypes = [vp]
    L.hibag_hip_trainer_set_em_mode.argtypes = [vp, i32]
    L.hibag_hip_trainer_set_shared.argtypes = [vp, i32]
    L.hibag_hip_train_set_thread_budget.argtypes = [i32]
    L.hibag_hip_train_combine_stats.argtypes = [C.POINTER(i64), C.POINTER(i64), i32]
    L.hibag_hip_train_combine_times.argtypes = [C.POINTER(dbl), i32]
    L.hibag_hip_trainer_classifier_dims.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.hibag_hip_trainer_classifier_get.argtypes = [vp, i32, vp, vp, vp, vp, vp, C.POINTER(dbl)]
    L.hibag_hip_bed_flag.argtypes = [C.c_char_p]
    L.hibag_hip_conv_bed.argtypes = [C.c_char_p, i32, i32, i32, vp, vp]
    L.hibag_hip_predict_bed.argtypes = [vp, C.c_char_p, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_predict_mapped.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_predict_mapped_device.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_predict_snp_major.argtypes = [vp, vp, C.c_size_t, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_predict_snp_major_device.argtypes = [vp, vp, C.c_size_t, i32, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_model_status.argtypes = [vp]
    L.hibag_hip_model_clear_status.argtypes = [vp]
    L.hibag_hip_model_handover_faults.argtypes = [vp]
    L.hibag_hip_model_handover_faults.restype = i64
    L.hibag_hip_test_inject_handover_fault.argtypes = [vp, i32]
    L.hibag_hip_model_engine.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(i32)]
    L.hibag_hip_model_replicate.argtypes = [vp, i32]
    L.hibag_hip_model_replicate.restype = vp
    L.hibag_hip_multi_slice.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.hibag_hip_predict_multi.argtypes = [C.POINTER(vp), i32, vp, i32, i32, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_shard_bounds.argtypes = [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.hibag_hip_model_shard.argtypes = [vp, i32, i32, i32]
    L.hibag_hip_model_shard.restype = vp
    L.hibag_hip_model_batch_limit.argtypes = [vp]
    L.hibag_hip_shard_group_new.argtypes = [C.POINTER(vp), i32]
    L.hibag_hip_shard_group_new.restype = vp
    L.hibag_hip_shard_group_free.argtypes = [vp]
    L.hibag_hip_shard_group_free.restype = None
    L.hibag_hip_shard_group_ranks.argtypes = [vp]
    L.hibag_hip_shard_group_allreduces.argtypes = [vp]
    L.hibag_hip_shard_group_allreduces.restype = i64
    L.hibag_hip_rccl_version.restype = i32
    L.hibag_hip_shard_group_predict.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_predict_multi_sharded.argtypes = [C.POINTER(vp), i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.hibag_hip_measure_issue_costs.argtypes = [C.POINTER(dbl)] * 4
    L.hibag_hip_test_time_avg_prob.argtypes = [vp, vp, i32, i32, i32, vp, vp, C.POINTER(dbl)]
    if hasattr(L, "hibag_hip_test_build_eval_batch"):     # (absent from an older build selected with HIBAG_HIP_LIBRARY)
        L.hibag_hip_test_build_eval_batch.argtypes = [i32, i32, vp, vp, i32, i32, vp, vp, vp, vp, i32, vp, i32, vp, vp]
    if hasattr(L, "hibag_hip_test_em_fit"):               # (likewise)
        L.hibag_hip_test_em_fit.argtypes = [i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
        L.hibag_hip_test_em_layout.argtypes = [i32, i32, i32]
        L.hibag_hip_trainer_em_counts.argtypes = [vp, C.POINTER(C.c_longlong)]
    if hasattr(L, "hibag_hip_test_layout_plan"):          # (likewise)
        L.hibag_hip_test_layout_plan.argtypes = [vp]
        L.hibag_hip_test_layout_plan.restype = vp
        L.hibag_hip_test_layout_count.argtypes = [vp]
        L.hibag_hip_test_layout_get.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(i32)]
        L.hibag_hip_test_layout_free.argtypes = [vp]
        L.hibag_hip_test_layout_free.restype = None
    if hasattr(L, "hibag_hip_test_set_chunking"):         # (likewise)
        L.hibag_hip_test_set_chunking.argtypes = [vp, i32, i32, i32]
        L.hibag_hip_test_last_launch.argtypes = [vp, C.POINTER(LaunchInfo)]
        L.hibag_hip_test_plan_total.argtypes = [i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(LaunchInfo)]
        L.hibag_hip_test_plan_accum.argtypes = [i32, i32, i32, C.POINTER(LaunchInfo)]
    if hasattr(L, "hibag_hip_test_read_diag"):
        L.hibag_hip_test_read_diag.argtypes = [vp, vp, i32]
        L.hibag_hip_plugin_degraded_calls.restype = i64
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        raise HibagHipError(rc, lib().hibag_hip_last_error().decode("utf-8", "replace"))
