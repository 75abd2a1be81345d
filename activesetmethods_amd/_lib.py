"""ctypes binding of libasmhip.so (include/asm_hip.h).  The HIP library is the product: loading fails
loudly when it is missing - there is no CPU fallback."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, os.environ.get("ASM_HIP_LIB", "libasmhip.so"))      # ASM_HIP_LIB: another build in the package directory (A/B timing in one GPU call)

OPTIMAL, INFEASIBLE, DUAL_INFEASIBLE, OTHER = 1, 2, 3, 4
K_NAMES = ("assemble", "scale", "gemv", "syrk", "chol", "trsv", "syrk_kernel", "panel_kernel")


class SolveStats(C.Structure):
    _fields_ = [("path", C.c_int32), ("polished", C.c_int32), ("ipm_iters", C.c_int32), ("nfact", C.c_int32),
                ("eqp", C.c_int32), ("M", C.c_int32), ("n", C.c_int32), ("ns", C.c_int32), ("col_iters", C.c_int32),
                ("ns_iters", C.c_int32), ("ns_dim", C.c_int32), ("ns_cold", C.c_int32), ("restored", C.c_int32),
                ("ns_path", C.c_int32), ("ipm_pinf", C.c_double), ("ipm_dinf", C.c_double), ("ipm_gap", C.c_double),
                ("kkt_pr", C.c_double), ("kkt_du", C.c_double), ("wall_ms", C.c_double)]


class KernelStats(C.Structure):
    _fields_ = [("ms", C.c_double * 8), ("calls", C.c_int64 * 8), ("flops", C.c_double * 8), ("bytes", C.c_double * 8)]


class SlpParams(C.Structure):
    """asm_slp_params (src/parameters.jl:17-28)."""
    _fields_ = [("max_iter", C.c_int32), ("max_lp_solves", C.c_int32), ("tol_direction", C.c_double), ("tol_residual", C.c_double),
                ("tol_infeas", C.c_double), ("eta", C.c_double), ("tau", C.c_double), ("min_alpha", C.c_double)]


class SlpResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("iter", C.c_int32), ("lp_solves", C.c_int32), ("restoration_solves", C.c_int32),
                ("ls_trials", C.c_int32), ("slot", C.c_int32), ("paths", C.c_int32 * 12), ("ipm_iters", C.c_int32), ("ns_cold", C.c_int32),
                ("obj_val", C.c_double), ("prim_infeas", C.c_double), ("dual_infeas", C.c_double), ("compl_", C.c_double)]


class SlpTrInfo(C.Structure):
    """asm_slp_tr_info: final radius; steps with rho >= 0 / < 0; radius decreases / increases."""
    _fields_ = [("delta", C.c_double), ("accepted", C.c_int32), ("rejected", C.c_int32), ("shrunk", C.c_int32), ("expanded", C.c_int32)]


class IpmStage(C.Structure):
    """asm_ipm_stage: one stage of asm_test_ipm_stages (include/asm_hip.h)."""
    _fields_ = [("kind", C.c_int32), ("mode", C.c_int32), ("spec", C.c_int32), ("sexp", C.c_int32), ("origin", C.c_int32), ("dir", C.c_int32),
                ("with_e", C.c_int32), ("D", C.c_int32), ("B", C.c_int32), ("pub", C.c_uint32),
                ("tp", C.c_double), ("td", C.c_double), ("res", C.c_double), ("crel", C.c_double), ("floor_", C.c_double), ("rho_p", C.c_double),
                ("mu_factor", C.c_double), ("al", C.c_double), ("be", C.c_double), ("fixed", C.c_double),
                ("x", C.c_int64 * 4), ("ix", C.c_int64 * 2), ("len", C.c_int64 * 3)]


class AsStage(C.Structure):
    """asm_as_stage: one stage of asm_test_as_stages (include/asm_hip.h)."""
    _fields_ = [("kind", C.c_int32), ("with_y", C.c_int32), ("accumulate", C.c_int32), ("check_only", C.c_int32), ("have_prev", C.c_int32),
                ("rperm", C.c_int32), ("fam", C.c_int32), ("k", C.c_int32), ("set", C.c_int32 * 3), ("pad_", C.c_int32), ("e", C.c_int64),
                ("tol_p", C.c_double), ("tol_d", C.c_double), ("tol_m", C.c_double), ("x", C.c_int64 * 4)]


class NsStage(C.Structure):
    """asm_ns_stage: one stage of asm_test_ns_stages (include/asm_hip.h)."""
    _fields_ = [("kind", C.c_int32), ("mode", C.c_int32), ("add", C.c_int32), ("D", C.c_int32), ("B", C.c_int32), ("pub", C.c_uint32),
                ("rho_p", C.c_double), ("res", C.c_double), ("al", C.c_double), ("be", C.c_double), ("es", C.c_double), ("eta", C.c_double),
                ("rerr", C.c_double), ("scale", C.c_double), ("val", C.c_double), ("x", C.c_int64 * 4), ("len", C.c_int64)]


class NssStage(C.Structure):
    """asm_nss_stage: one stage of asm_test_ns_setup_stages (include/asm_hip.h)."""
    _fields_ = [("kind", C.c_int32), ("flag", C.c_int32), ("thr", C.c_double)]


class KktStage(C.Structure):
    """asm_kkt_stage: one stage of asm_test_kkt_stages (include/asm_hip.h)."""
    _fields_ = [("kind", C.c_int32), ("flag", C.c_int32 * 3), ("pub", C.c_uint32), ("pad_", C.c_int32), ("s", C.c_double * 2), ("len", C.c_int64 * 3),
                ("x", C.c_int64 * 7), ("ix", C.c_int64 * 7), ("lx", C.c_int64 * 3)]


class BatchStats(C.Structure):
    _fields_ = [("rounds", C.c_int64), ("ops", C.c_int64), ("launches", C.c_int64), ("releases", C.c_int64), ("blob_bytes", C.c_int64),
                ("emit_ms", C.c_double), ("wait_ms", C.c_double), ("host_ms", C.c_double), ("wall_ms", C.c_double),
                ("panel_ms", C.c_double), ("panel_launches", C.c_int64), ("panel_ops", C.c_int64), ("panel_flops", C.c_double), ("panel_bytes", C.c_double),
                ("panel_grid_max", C.c_int64)]


class BatchKernelRow(C.Structure):
    """asm_batch_kernel_row: one row of asm_test_batch_kernel_table (include/asm_hip.h)."""
    _fields_ = [("name", C.c_char * 256), ("operations", C.c_int64), ("launches", C.c_int64), ("nb_max", C.c_int32), ("gz", C.c_int32)]


class KktParams(C.Structure):
    """asm_kkt_params."""
    _fields_ = [("max_iter", C.c_int32), ("rtol", C.c_double)]


class KktInfo(C.Structure):
    """asm_kkt_info: status 0 solved, 1 iteration limit, 2 reduced Hessian not positive definite, 3 dependent working rows."""
    _fields_ = [("status", C.c_int32), ("cg_iters", C.c_int32), ("n_free", C.c_int32), ("n_rows", C.c_int32), ("dropped_pivots", C.c_int32),
                ("res_stat", C.c_double), ("res_feas", C.c_double)]


class KktStepParams(C.Structure):
    """asm_kkt_step_params."""
    _fields_ = [("max_iter", C.c_int32), ("rtol", C.c_double), ("normal_share", C.c_double)]


class KktStepInfo(C.Structure):
    """asm_kkt_step_info: asm_kkt_info's fields; boundary 0 inside the region, 1 reached on positive curvature, 2 reached along
    p'Hp <= 0; theta, the norms of the normal step and of the step, the model value."""
    _fields_ = [("status", C.c_int32), ("cg_iters", C.c_int32), ("n_free", C.c_int32), ("n_rows", C.c_int32), ("dropped_pivots", C.c_int32),
                ("boundary", C.c_int32), ("res_stat", C.c_double), ("res_feas", C.c_double), ("theta", C.c_double),
                ("norm_normal", C.c_double), ("norm_step", C.c_double), ("model", C.c_double)]


class KktFormInfo(C.Structure):
    """asm_kkt_form_info: the form asked for and used by the last KKT call (0 dense, 1 sparse), the bandwidth and structural pairs of S in
    the order used, whether the order came from the cache, the device bytes of each form's own buffers, host milliseconds of the ordering."""
    _fields_ = [("form_requested", C.c_int32), ("form_used", C.c_int32), ("band", C.c_int32), ("order_reused", C.c_int32),
                ("n_pairs", C.c_int64), ("dense_bytes", C.c_int64), ("sparse_bytes", C.c_int64), ("order_ms", C.c_double)]


class RangeInfo(C.Structure):
    """asm_range_info: the range [t_lo, t_hi] of a sensitivity column and what blocks at either end - position (row i, or m + variable
    j; -1 none) and kind (sensitivity.RANGE_KINDS)."""
    _fields_ = [("t_lo", C.c_double), ("t_hi", C.c_double), ("pos_lo", C.c_int32), ("kind_lo", C.c_int32), ("pos_hi", C.c_int32), ("kind_hi", C.c_int32)]


KKT_FORMS = {"dense": 0, "sparse": 1}


class KktOrderInfo(C.Structure):
    """asm_kkt_order_info: the row order of the sparse form asked for and used by the last KKT call (0 working-set, 1 static), the band and
    the structural pairs of S over all m rows in the static order (0 before the first sparse call)."""
    _fields_ = [("order_requested", C.c_int32), ("order_used", C.c_int32), ("all_band", C.c_int64), ("all_pairs", C.c_int64)]


KKT_ORDERS = {"working-set": 0, "static": 1}


class EqpInfo(C.Structure):
    """asm_eqp_info: asm_kkt_step_info's fields; skipped 0 none, 1 more working rows than free variables, 2 dependent working rows,
    3 zero step; t, the norms of d = t dx, the merit function at x and at x + d."""
    _fields_ = [("status", C.c_int32), ("cg_iters", C.c_int32), ("n_free", C.c_int32), ("n_rows", C.c_int32), ("dropped_pivots", C.c_int32),
                ("boundary", C.c_int32), ("res_stat", C.c_double), ("res_feas", C.c_double), ("theta", C.c_double),
                ("norm_normal", C.c_double), ("norm_step", C.c_double), ("model", C.c_double), ("skipped", C.c_int32), ("t", C.c_double),
                ("norm_d", C.c_double), ("norm_d_inf", C.c_double), ("phi0", C.c_double), ("phi1", C.c_double)]


class SlpEqpParams(C.Structure):
    """asm_slp_eqp_params."""
    _fields_ = [("radius0", C.c_double), ("radius_max", C.c_double), ("tol_active", C.c_double), ("enabled", C.c_int32)]


class SlpEqpInfo(C.Structure):
    """asm_slp_eqp_info: final radius of the EQP step and the trial counts of a native SLP-EQP run."""
    _fields_ = [("radius", C.c_double), ("attempts", C.c_int32), ("accepted", C.c_int32), ("rejected", C.c_int32), ("skipped_rows", C.c_int32),
                ("skipped_dependent", C.c_int32), ("skipped_zero", C.c_int32), ("cg_iters", C.c_int32), ("boundary", C.c_int32)]


class LmInfo(C.Structure):
    """asm_lm_info: the handle's Hessian type (0 exact, 1 limited-memory) and the limited-memory store - its memory, the pairs it holds,
    whether a begin waits for its end, the pairs offered and refused since it was cleared, sigma, its device bytes."""
    _fields_ = [("type", C.c_int32), ("memory", C.c_int32), ("pairs", C.c_int32), ("pending", C.c_int32), ("pushed", C.c_int64),
                ("skipped_zero", C.c_int64), ("skipped_curvature", C.c_int64), ("sigma", C.c_double), ("bytes", C.c_int64)]


HESSIAN_TYPES = {"exact": 0, "limited-memory": 1}
LM_MAX = 32

_P = C.c_void_p
_D = C.POINTER(C.c_double)
_I64 = C.POINTER(C.c_int64)
_I32 = C.POINTER(C.c_int32)
_U8 = C.POINTER(C.c_uint8)

PROTOTYPES = {
    "asm_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "asm_destroy": (C.c_int, [_P]),
    "asm_last_error": (C.c_char_p, [_P]),
    "asm_sublp_setup": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _I64, _I64, _D, _D, _D, _D]),
    "asm_sublp_set_bounds": (C.c_int, [_P, _D, _D, _D, _D]),
    "asm_sublp_solve": (C.c_int, [_P, _D, _D, C.c_double, _D, _D, C.c_double, C.c_int, _D, _D, _D, _D, _D, _I32]),
    "asm_lp_solve": (C.c_int, [_P, _D, _D, _D, _D, _D, C.c_int, _D, _D, _D, _D, _D, _D, _I32, _I32]),
    "asm_sublp_upload": (C.c_int, [_P, _D, _D, C.c_double, _D, _D]),
    "asm_sublp_solve_resident": (C.c_int, [_P, C.c_double, C.c_int, _D, _D, _D, _D, _D, _I32]),
    "asm_sublp_active_set": (C.c_int, [_P, _I32, _I32, _I32, _I64, _I64]),
    "asm_sublp_reset_warm": (C.c_int, [_P]),
    "asm_sublp_ns_basis": (C.c_int, [_P, _I32, _I64]),
    "asm_sublp_row_order": (C.c_int, [_P, _I32, _I64, _I32, _I64, _I64]),
    "asm_sublp_last_stats": (C.c_int, [_P, C.POINTER(SolveStats)]),
    "asm_kernel_stats_get": (C.c_int, [_P, C.POINTER(KernelStats)]),
    "asm_kernel_stats_reset": (C.c_int, [_P]),
    "asm_kernel_timing": (C.c_int, [_P, C.c_int]),
    "asm_kt_residuals": (C.c_int, [_P, _D, _D, _D, _D, _D]),
    "asm_jac_row_norms": (C.c_int, [_P, _D]),
    "asm_eval_setup": (C.c_int, [_P, C.c_int64, _I64, _I64, _D, _I64, _I64, _I64, _D, _D, _I64, _I64, _I64, _D, _I64, C.c_double, C.c_int,
                                 C.c_int64, C.c_int64, _I64, C.c_int64, _D, C.c_int64]),
    "asm_eval_functions": (C.c_int, [_P, _D, _D, _D, _D]),
    "asm_eval_constraints": (C.c_int, [_P, _D, _D, _D]),
    "asm_eval_jacobian_values": (C.c_int, [_P, _D]),
    "asm_eval_set_data": (C.c_int, [_P, C.c_int64, C.c_int64, _D]),
    "asm_eval_data_gradient": (C.c_int, [_P, _D, _D, _D]),
    "asm_eval_data_cross": (C.c_int, [_P, _D, _D, _D, _D, _D]),
    "asm_kkt_solve": (C.c_int, [_P, _D, _D, _I32, _I32, _D, _D, C.POINTER(KktParams), _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_solution_sensitivity": (C.c_int, [_P, _D, _D, _I32, _I32, _D, C.POINTER(KktParams), _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_kkt_solve_multi": (C.c_int, [_P, _D, _D, _I32, _I32, C.c_int32, _D, _D, C.POINTER(KktParams), _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_solution_sensitivity_multi": (C.c_int, [_P, _D, _D, _I32, _I32, C.c_int32, _D, C.POINTER(KktParams), _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_bound_sensitivity_multi": (C.c_int, [_P, _D, _D, _I32, _I32, C.c_int32, _I32, _D, C.POINTER(KktParams), _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_eval_data_cross_t": (C.c_int, [_P, _D, _D, _D, _D, _D]),
    "asm_solution_adjoint": (C.c_int, [_P, _D, _D, _I32, _I32, _D, _D, C.POINTER(KktParams), _D, _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_solution_adjoint_multi": (C.c_int, [_P, _D, _D, _I32, _I32, C.c_int32, _D, _D, C.POINTER(KktParams), _D, _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_var_bound_sensitivity_multi": (C.c_int, [_P, _D, _D, _I32, _I32, C.c_int32, _I32, _D, C.POINTER(KktParams), _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_sensitivity_range_multi": (C.c_int, [_P, _D, _D, _D, _I32, _I32, C.c_int32, _D, _D, _D, C.POINTER(RangeInfo)]),
    "asm_solution_adjoint_z": (C.c_int, [_P, _D, _D, _I32, _I32, _D, _D, _D, C.POINTER(KktParams), _D, _D, _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_solution_adjoint_z_multi": (C.c_int, [_P, _D, _D, _I32, _I32, C.c_int32, _D, _D, _D, C.POINTER(KktParams), _D, _D, _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_kkt_step": (C.c_int, [_P, _D, _D, _I32, _I32, _D, _D, C.c_double, C.POINTER(KktStepParams), _D, _D, _D, C.POINTER(KktStepInfo)]),
    "asm_kkt_step_multi": (C.c_int, [_P, _D, _D, _I32, _I32, C.c_int32, _D, _D, _D, C.POINTER(KktStepParams), _D, _D, _D, C.POINTER(KktStepInfo)]),
    "asm_kkt_set_form": (C.c_int, [_P, C.c_int32]),
    "asm_kkt_form_info": (C.c_int, [_P, C.POINTER(KktFormInfo)]),
    "asm_kkt_set_order": (C.c_int, [_P, C.c_int32]),
    "asm_kkt_order_info": (C.c_int, [_P, C.POINTER(KktOrderInfo)]),
    "asm_kkt_row_order": (C.c_int, [_P, _I32, _I64]),
    "asm_eval_hessian_structure": (C.c_int, [_P, _I64, _I64, _I64]),
    "asm_eval_hessian_lagrangian": (C.c_int, [_P, _D, C.c_double, _D, _D]),
    "asm_eval_hessian_product": (C.c_int, [_P, _D, C.c_double, _D, _D, _D]),
    "asm_slp_norms": (C.c_int, [_P, _D, _D, _D, _D]),
    "asm_slp_merit": (C.c_int, [_P, C.c_int, C.c_double, _D, _D, _D, C.c_int, C.c_double, _D]),
    "asm_slp_line_search": (C.c_int, [_P, _D, _D, _D, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _D, _D,
                                      C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "asm_slp_step_quality": (C.c_int, [_P, _D, _D, _D, C.c_int, C.c_double, _D]),
    "asm_sublp_set_ns_basis": (C.c_int, [_P, _I32, C.c_int64]),
    "asm_slp_run": (C.c_int, [_P, C.POINTER(SlpParams), _D, _D, _D, _D, _D, _D, C.POINTER(SlpResult)]),
    "asm_slp_run_tr": (C.c_int, [_P, C.POINTER(SlpParams), C.c_double, _D, _D, _D, _D, _D, _D, C.POINTER(SlpResult), C.POINTER(SlpTrInfo)]),
    "asm_eqp_trial": (C.c_int, [_P, _D, _D, _I32, _I32, C.c_double, _D, C.c_double, C.POINTER(KktStepParams), _D, _D, _D, _D, _I32, _I32, C.POINTER(EqpInfo)]),
    "asm_slp_run_eqp": (C.c_int, [_P, C.POINTER(SlpParams), C.c_double, C.POINTER(SlpEqpParams), _D, _D, _D, _D, _D, _D, C.POINTER(SlpResult),
                                  C.POINTER(SlpTrInfo), C.POINTER(SlpEqpInfo)]),
    "asm_hessian_set_type": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "asm_lm_reset": (C.c_int, [_P]),
    "asm_lm_push_pair": (C.c_int, [_P, _D, _D]),
    "asm_lm_begin": (C.c_int, [_P, _D]),
    "asm_lm_end": (C.c_int, [_P, _D]),
    "asm_lm_product": (C.c_int, [_P, _D, C.c_int32, _D]),
    "asm_lm_info": (C.c_int, [_P, C.POINTER(LmInfo)]),
    "asm_batch_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_P)]),
    "asm_batch_destroy": (C.c_int, [_P]),
    "asm_batch_last_error": (C.c_char_p, [_P]),
    "asm_batch_slots": (C.c_int, [_P]),
    "asm_batch_set_groups": (C.c_int, [_P, C.c_int]),
    "asm_batch_groups": (C.c_int, [_P]),
    "asm_batch_handle": (_P, [_P, C.c_int]),
    "asm_batch_setup": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _I64, _I64, _D, _D, _D, _D]),
    "asm_batch_eval_setup": (C.c_int, [_P, C.c_int64, _I64, _I64, _D, _I64, _I64, _I64, _D, _D, _I64, _I64, _I64, _D, _I64, C.c_double, C.c_int,
                                       C.c_int64, C.c_int64, _I64, C.c_int64, _D, C.c_int64]),
    "asm_batch_set_ns_basis": (C.c_int, [_P, _I32, C.c_int64]),
    "asm_batch_set_scenario_data": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _D]),
    "asm_batch_data_gradient": (C.c_int, [_P, C.c_int64, _D, _D, _D]),
    "asm_batch_hessian_structure": (C.c_int, [_P, _I64, _I64, _I64]),
    "asm_batch_hessian_lagrangian": (C.c_int, [_P, C.c_int64, _D, _D, _D, _D]),
    "asm_batch_hessian_product": (C.c_int, [_P, C.c_int64, _D, _D, _D, _D, _D]),
    "asm_batch_ns_basis": (C.c_int, [_P, _I32, _I64]),
    "asm_batch_sublp_solve": (C.c_int, [_P, C.c_int, _D, _D, _D, _D, _D, _D, _D, _D, _D, _D, _I32, _D, _D, _D, _D, _D, _I32]),
    "asm_batch_slp_run": (C.c_int, [_P, C.c_int64, _D, _D, _D, _D, _D, C.POINTER(SlpParams), _D, _D, _D, _D, _D, C.POINTER(SlpResult)]),
    "asm_batch_slp_run_tr": (C.c_int, [_P, C.c_int64, _D, _D, _D, _D, _D, C.POINTER(SlpParams), C.c_double, _D, _D, _D, _D, _D, C.POINTER(SlpResult),
                                       C.POINTER(SlpTrInfo)]),
    "asm_batch_slp_run_eqp": (C.c_int, [_P, C.c_int64, _D, _D, _D, _D, _D, C.POINTER(SlpParams), C.c_double, C.POINTER(SlpEqpParams), _D, _D, _D, _D, _D,
                                        C.POINTER(SlpResult), C.POINTER(SlpTrInfo), C.POINTER(SlpEqpInfo)]),
    "asm_batch_kkt_set_form": (C.c_int, [_P, C.c_int32, C.c_int32]),
    "asm_batch_kkt_solve": (C.c_int, [_P, C.c_int64, _D, _D, _I32, _I32, C.c_int32, _D, _D, C.POINTER(KktParams), _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_batch_solution_sensitivity": (C.c_int, [_P, C.c_int64, _D, _D, _I32, _I32, C.c_int32, _D, C.c_int32, C.POINTER(KktParams), _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_batch_bound_sensitivity": (C.c_int, [_P, C.c_int64, _D, _D, _I32, _I32, C.c_int32, _I32, _D, C.POINTER(KktParams), _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_batch_var_bound_sensitivity": (C.c_int, [_P, C.c_int64, _D, _D, _I32, _I32, C.c_int32, _I32, _D, C.POINTER(KktParams), _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_batch_sensitivity_range": (C.c_int, [_P, C.c_int64, _D, _D, _D, _D, _D, _D, _D, _I32, _I32, C.c_int32, _D, _D, _D, C.POINTER(RangeInfo)]),
    "asm_batch_solution_adjoint_z": (C.c_int, [_P, C.c_int64, _D, _D, _I32, _I32, C.c_int32, _D, _D, _D, C.POINTER(KktParams), _D, _D, _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_batch_solution_adjoint": (C.c_int, [_P, C.c_int64, _D, _D, _I32, _I32, C.c_int32, _D, _D, C.POINTER(KktParams), _D, _D, _D, _D, C.POINTER(KktInfo)]),
    "asm_batch_get_stats": (C.c_int, [_P, C.POINTER(BatchStats)]),
    "asm_test_syrk": (C.c_int, [_P, _D, C.c_int64, C.c_int64, _I32, C.c_int64, _D, _D, _D, C.c_int]),
    "asm_test_syrk_update": (C.c_int, [_P, _D, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _D, C.c_int]),
    "asm_test_build_flagged": (C.c_int, [_P, _D, C.c_int64, C.c_int64, _I32, C.c_int64, _D, _D, C.c_int, C.c_int, _D, C.c_int64, C.POINTER(C.c_ubyte), _D]),
    "asm_test_build_split": (C.c_int, [_P, _D, C.c_int64, C.c_int64, _D, C.c_int, C.c_double, C.c_double, _D, _D, _D, _D]),
    "asm_test_build_dispatch": (C.c_int, [_P, _D, C.c_int, _I32, C.c_int64, _D, _D, _D, _D, _I64, _I32, _I32, _I32]),
    "asm_test_ipm_stages": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_double, _I64, _D, C.c_int64, _I32, C.c_int64, _D, _D, C.POINTER(C.c_uint32),
                                      _D, C.POINTER(C.c_uint32), C.POINTER(IpmStage), C.c_int64, C.POINTER(C.c_uint32)]),
    "asm_test_as_stages": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_double, _I64, _D, C.c_int64, _I32, C.c_int64, _D, C.c_int64,
                                     C.POINTER(AsStage), C.c_int64, C.POINTER(C.c_uint32)]),
    "asm_test_kkt_stages": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _I64, _D, C.c_int64, _I32, C.c_int64, _I64, C.c_int64,
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _D, C.POINTER(C.c_uint32), C.POINTER(KktStage), C.c_int64,
                                      C.POINTER(C.c_uint32)]),
    "asm_test_ns_stages": (C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, C.c_double, _I32, _I32, _I32, _D, _D, _D, _I64, _I32, _D, C.c_int64, _D,
                                     C.POINTER(C.c_uint32), C.POINTER(NsStage), C.c_int64, C.POINTER(C.c_uint32)]),
    "asm_test_ns_setup_stages": (C.c_int, [_P, _D, _D, C.c_int64, C.c_int64, _I32, _I64, _I32, _D, _D, _D, _D, _D, _D, _D, _D, _D, C.c_int32, _I32, C.c_int64,
                                           C.POINTER(NssStage), C.c_int64, C.POINTER(C.c_uint32), _I32, _I32]),
    "asm_test_cholesky": (C.c_int, [_P, _D, C.c_int64, _D]),
    "asm_test_chol_solve": (C.c_int, [_P, _D, C.c_int64, _D, _D]),
    "asm_test_no_polish": (C.c_int, [_P, C.c_int]),
    "asm_test_kkt_multi_rounds": (C.c_int, [_P, _I64, _I32]),
    "asm_test_panel_timeout": (C.c_int, [_P, C.c_int]),
    "asm_test_set_band": (C.c_int, [_P, C.c_int]),
    "asm_test_set_factor": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]),
    "asm_test_gemm_nt": (C.c_int, [_P, _D, _D, _D, C.c_int64, C.c_int64, C.c_int64, C.c_int, _D]),
    "asm_test_trsm_rows": (C.c_int, [_P, _D, C.c_int64, _D, C.c_int64, C.c_int, _D]),
    "asm_test_gemv": (C.c_int, [_P, _D, C.c_int64, C.c_int64, _D, _D, _D, _D]),
    "asm_test_assemble": (C.c_int, [_P, _D, _D]),
    "asm_test_skeleton_stages": (C.c_int, [_P, C.c_uint32, _D, _D, _D, _D, _D, _D, _I64, _D, _D, _D, _D, _D, _D, _D, _D, _D, _D, _D, _I32, _D, _D]),
    "asm_test_mfma_peak": (C.c_int, [_P, C.c_int, C.c_int, _D]),
    "asm_test_copy_fill": (C.c_int, [_P, C.c_uint32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _U8, _U8, _U8, _U8, _U8, _U8]),
    "asm_batch_test_run": (C.c_int, [_P, C.c_int32, C.c_int64, _P, _I32]),
    "asm_batch_test_record_size": (C.c_int64, [C.c_int32]),
    "asm_test_batch_kernel_counting": (C.c_int, [_P, C.c_int]),
    "asm_test_batch_panel_share": (C.c_int, [_P, C.c_int]),
    "asm_test_batch_kernel_table": (C.c_int, [_P, C.POINTER(BatchKernelRow), C.c_int64, _I64, C.c_int]),
}

# asm_batch_test_run: the families (ASM_TF_* of include/asm_hip.h, in order) by the hook they run.  A family's record (asm_test_*_args) has the
# hook's parameters after h as its fields, in order: hook_record(hook) makes that structure from the hook's prototype
TEST_FAMILIES = ("asm_test_skeleton_stages", "asm_test_ipm_stages", "asm_test_as_stages", "asm_test_ns_stages", "asm_test_ns_setup_stages", "asm_test_kkt_stages",
                 "asm_test_cholesky", "asm_test_chol_solve", "asm_test_trsm_rows", "asm_test_gemm_nt", "asm_test_gemv", "asm_test_syrk", "asm_test_syrk_update",
                 "asm_test_build_split", "asm_test_copy_fill")
_RECORDS = {}


def hook_record(hook):
    if hook not in _RECORDS:
        fields = [("a%d" % i, t) for i, t in enumerate(PROTOTYPES[hook][1][1:])]
        _RECORDS[hook] = type(hook + "_args", (C.Structure,), {"_fields_": fields})
    return _RECORDS[hook]


_lib = None


def load():
    """Load libasmhip.so and bind every symbol include/asm_hip.h declares."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(make -C activesetmethods_amd/csrc).  There is no CPU fallback." % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(lib, name)      # AttributeError here = ABI drift, fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def dptr(a):
    return a.ctypes.data_as(_D)


def i64ptr(a):
    return a.ctypes.data_as(_I64)


def i32ptr(a):
    return a.ctypes.data_as(_I32)
