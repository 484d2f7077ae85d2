"""ctypes binding of ``libmetran_hip.so`` (C ABI declared in ``include/metran_hip.h``).

There is NO CPU fallback: if the shared library is missing, or no gfx950 device is
visible, every compute entry point raises ``MetranHipError``.  (``oracle/`` is test
infrastructure and is never imported from here.)
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

__all__ = ["MetranHipError", "lib", "library_path", "Problem", "Outputs", "ForecastRequest", "WeightsRequest", "RegressionRequest", "ScoresRequest", "check", "API"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBNAME = "libmetran_hip.so"


class MetranHipError(Exception):
    """Raised for every failure of the HIP library (the reference raises bare ``Exception``
    with a logged message, e.g. /root/reference/metran/kalmanfilter.py:733-745)."""


c_dp = POINTER(c_double)
c_i64p = POINTER(c_int64)
c_u32p = POINTER(c_uint32)


class Problem(Structure):
    """``mk_problem`` (include/metran_hip.h)."""

    _fields_ = [
        ("n_instances", c_int64),
        ("n_records", c_int64),
        ("T", c_int64),
        ("N", c_int64),
        ("K", c_int64),
        ("warmup", c_int64),
        ("d_obs", c_void_p),
        ("d_phi", c_void_p),
        ("d_q", c_void_p),
        ("d_loadings", c_void_p),
        ("d_obsvar", c_void_p),
        ("d_x0", c_void_p),
        ("d_P0", c_void_p),
        ("obs_time_major", c_int64),
        ("d_scale", c_void_p),
        ("d_offset", c_void_p),
    ]


class Outputs(Structure):
    """``mk_outputs`` (include/metran_hip.h)."""

    _fields_ = [
        ("d_mle", c_void_p),
        ("d_sigmas", c_void_p),
        ("d_detfs", c_void_p),
        ("d_sigmacount", c_void_p),
        ("d_F", c_void_p),
        ("d_Pf", c_void_p),
        ("d_Xp", c_void_p),
        ("d_Pp", c_void_p),
        ("d_S", c_void_p),
        ("d_Ps", c_void_p),
        ("d_status", c_void_p),
        ("time_major", c_int64),
        ("d_sim_means", c_void_p),
        ("d_sim_vars", c_void_p),
        ("record_stride", c_int64),
        ("flags", c_int64),
    ]


class ForecastRequest(Structure):
    """``mk_forecast_request`` (include/metran_hip.h)."""

    _fields_ = [
        ("horizon", c_int64),
        ("t_first", c_int64),
        ("track_horizon", c_int64),
        ("coverage_z", c_double),
        ("d_fan_origins", c_void_p),
        ("d_fan_means", c_void_p),
        ("d_fan_vars", c_void_p),
        ("d_track_means", c_void_p),
        ("d_track_vars", c_void_p),
        ("d_skill", c_void_p),
    ]


class WeightsRequest(Structure):
    """``mk_weights_request`` (include/metran_hip.h)."""

    _fields_ = [
        ("n_targets", c_int64),
        ("what", c_int),
        ("d_targets", c_void_p),
        ("d_weights", c_void_p),
        ("d_intercept", c_void_p),
    ]


class RegressionRequest(Structure):
    """``mk_regression_request`` (include/metran_hip.h)."""

    _fields_ = [
        ("n_effects", c_int64),
        ("t_first", c_int64),
        ("d_effects", c_void_p),
        ("d_beta", c_void_p),
        ("d_cov", c_void_p),
        ("d_gain", c_void_p),
        ("d_normal", c_void_p),
        ("d_support", c_void_p),
        ("d_dropped", c_void_p),
    ]


class ScoresRequest(Structure):
    """``mk_scores_request`` (include/metran_hip.h)."""

    _fields_ = [
        ("d_dphi", c_void_p),
        ("d_dq", c_void_p),
        ("t_first", c_int64),
        ("d_score", c_void_p),
        ("d_grad", c_void_p),
        ("d_count", c_void_p),
        ("d_opg", c_void_p),
        ("d_cusum", c_void_p),
    ]


class BlockRequest(Structure):
    """``mk_block_request`` (include/metran_hip.h)."""

    _fields_ = [
        ("n_blocks", c_int64),
        ("n_cells", c_int64),
        ("d_blocks", c_void_p),
        ("d_checkpoints", c_void_p),
        ("d_means", c_void_p),
        ("d_vars", c_void_p),
        ("d_summary", c_void_p),
        ("d_flags", c_void_p),
    ]


class ShiftRequest(Structure):
    """``mk_shift_request`` (include/metran_hip.h)."""

    _fields_ = [
        ("d_num", c_void_p),
        ("d_den", c_void_p),
    ]


class FunctionalRequest(Structure):
    """``mk_functional_request`` (include/metran_hip.h)."""

    _fields_ = [
        ("n_windows", c_int64),
        ("n_contrasts", c_int64),
        ("d_windows", c_void_p),
        ("d_contrasts", c_void_p),
    ]


# name -> (restype, argtypes); this table is what tests check against the header.
API = {
    "mk_abi_version": (c_int, []),
    "mk_last_error": (c_char_p, []),
    "mk_device_count": (c_int, [POINTER(c_int)]),
    "mk_create": (c_int, [c_int, POINTER(c_void_p)]),
    "mk_destroy": (c_int, [c_void_p]),
    "mk_set_stream": (c_int, [c_void_p, c_void_p]),
    "mk_sync": (c_int, [c_void_p]),
    "mk_observations_changed": (c_int, [c_void_p]),
    "mk_shape_supported": (c_int, [c_int64, c_int64]),
    "mk_shape_specialised": (c_int, [c_int64, c_int64]),
    "mk_generic_max_states": (c_int64, []),
    "mk_register_shape_module": (c_int, [c_char_p]),
    "mk_record_stride": (c_int64, [c_int64]),
    "mk_record_stride_sym": (c_int64, [c_int64]),
    "mk_tape_stride": (c_int64, [c_int64, c_int64]),
    "mk_tape_supported": (c_int, [c_int64, c_int64]),
    "mk_state_tape_stride": (c_int64, [c_int64, c_int64]),
    "mk_supported_shapes": (c_int, [c_i64p, c_int]),
    "mk_malloc": (c_int, [c_void_p, c_size_t, POINTER(c_void_p)]),
    "mk_free": (c_int, [c_void_p, c_void_p]),
    "mk_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "mk_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "mk_memset": (c_int, [c_void_p, c_void_p, c_int, c_size_t]),
    "mk_params_from_alpha": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_double,
                                     c_void_p, c_void_p]),
    "mk_filter": (c_int, [c_void_p, POINTER(Problem), POINTER(Outputs)]),
    "mk_loglik": (c_int, [c_void_p, POINTER(Problem), c_void_p]),
    "mk_smooth": (c_int, [c_void_p, POINTER(Problem), POINTER(Outputs)]),
    "mk_filter_smooth": (c_int, [c_void_p, POINTER(Problem), POINTER(Outputs)]),
    "mk_smooth_dense": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    "mk_simulate": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p]),
    "mk_decompose": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                             c_void_p]),
    "mk_sum": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "mk_comm_set_library": (c_int, [c_char_p]),
    "mk_comm_unique_id": (c_int, [c_void_p]),
    "mk_comm_init_rank": (c_int, [c_void_p, c_int, c_int, c_void_p]),
    "mk_set_communicator": (c_int, [c_void_p, c_void_p]),
    "mk_comm_destroy": (c_int, [c_void_p]),
    "mk_allreduce_sum": (c_int, [c_void_p, c_void_p, c_int64]),
    "mk_loglik_grad": (c_int, [c_void_p, POINTER(Problem), c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mk_loglik_grad_phases": (c_int, [c_void_p, POINTER(Problem), c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_int]),
    "mk_adjoint_update_stride": (c_int64, [c_int64, c_int64]),
    "mk_set_adjoint_updates": (c_int, [c_void_p, c_void_p, c_int64]),
    "mk_lbfgs_direction": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int)]),
    "mk_lbfgs_trial": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mk_lbfgs_armijo": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_int64, c_void_p, POINTER(c_int), POINTER(c_int)]),
    "mk_lbfgs_update": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_int64, POINTER(c_int)]),
    "mk_alpha_grad": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_double, c_void_p,
                              c_void_p, c_void_p]),
    "mk_loo_work_stride": (c_int64, [c_int64, c_int64]),
    "mk_loo": (c_int, [c_void_p, POINTER(Problem), c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mk_disturbance_work_stride": (c_int64, [c_int64, c_int64]),
    "mk_disturbances": (c_int, [c_void_p, POINTER(Problem), c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mk_innovations_work_stride": (c_int64, [c_int64, c_int64]),
    "mk_innovations": (c_int, [c_void_p, POINTER(Problem), c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mk_innovation_stats": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "mk_residual_series": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    "mk_residual_cross": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                  c_void_p]),
    "mk_forecast_max_horizon": (c_int64, []),
    "mk_forecast_work_stride": (c_int64, [c_int64, c_int64]),
    "mk_forecast": (c_int, [c_void_p, POINTER(Problem), c_void_p, c_int, POINTER(ForecastRequest), c_void_p]),
    "mk_weights_work_stride": (c_int64, [c_int64, c_int64]),
    "mk_observation_weights": (c_int, [c_void_p, POINTER(Problem), c_void_p, c_int, POINTER(WeightsRequest), c_void_p]),
    "mk_regression_max_effects": (c_int64, []),
    "mk_regression_work_stride": (c_int64, [c_int64, c_int64]),
    "mk_regression": (c_int, [c_void_p, POINTER(Problem), c_void_p, c_int, POINTER(RegressionRequest), c_void_p]),
    "mk_regression_adjust": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mk_scores_max_states": (c_int64, []),
    "mk_scores_work_stride": (c_int64, [c_int64, c_int64]),
    "mk_scores": (c_int, [c_void_p, POINTER(Problem), c_void_p, c_int, POINTER(ScoresRequest), c_void_p]),
    "mk_block_max_cells": (c_int64, []),
    "mk_block_work_stride": (c_int64, [c_int64, c_int64]),
    "mk_block_predict": (c_int, [c_void_p, POINTER(Problem), c_void_p, c_int, POINTER(BlockRequest), c_void_p]),
    "mk_shift_work_stride": (c_int64, [c_int64, c_int64]),
    "mk_level_shifts": (c_int, [c_void_p, POINTER(Problem), c_void_p, c_int, POINTER(ShiftRequest), c_void_p]),
    "mk_functionals_max_contrasts": (c_int64, []),
    "mk_functionals_work_stride": (c_int64, [c_int64, c_int64]),
    "mk_functionals": (c_int, [c_void_p, POINTER(Problem), c_void_p, c_int, POINTER(FunctionalRequest), c_void_p, c_void_p, c_void_p]),
    "mk_draw_perturb": (c_int, [c_void_p, POINTER(Problem), c_uint64, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "mk_draw_combine": (c_int, [c_void_p, POINTER(Problem), c_int64, c_int, c_int, c_void_p, c_void_p]),
    "mk_draw_normals": (c_int, [c_void_p, c_uint64, c_int64, c_int64, c_int64, c_int64, c_int, c_int64, c_int64, c_int, c_void_p]),
    "mk_path_functional_count": (c_int64, []),
    "mk_path_functionals": (c_int, [c_void_p, POINTER(Problem), c_int64, c_int, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "mk_ensemble_max_draws": (c_int64, []),
    "mk_ensemble_summary": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_dp, c_void_p]),
    "mk_standardize": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mk_mask_observations": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "mk_pack_observations": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mk_set_kernel_variant": (c_int, [c_void_p, c_int, c_int]),
    "mk_get_kernel_variant": (c_int, [c_void_p, c_int, POINTER(c_int)]),
    "mk_fa_correlation": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "mk_fa_analyse": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p]),
    "mk_fa_minres": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p]),
    "mk_fa_rotate": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_double, c_int, c_double]),
    "mk_fa_eigh": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "mk_enable_timing": (c_int, [c_void_p, c_int]),
    "mk_last_kernel_ms": (c_int, [c_void_p, POINTER(c_float), POINTER(c_float)]),
    "mk_kernel_ms_totals": (c_int, [c_void_p, POINTER(c_double), POINTER(c_int64), POINTER(c_double), POINTER(c_int64)]),
}

ABI_VERSION = 7  # MK_ABI_VERSION of include/metran_hip.h
_lib = None


def library_path():
    return os.environ.get("METRAN_HIP_LIBRARY", os.path.join(_HERE, _LIBNAME))


def lib():
    """Load (once) and return the bound library; raises MetranHipError if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise MetranHipError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C metran_amd/csrc` (hipcc --offload-arch=gfx950). There is no CPU fallback." % path
        )
    try:
        L = ctypes.CDLL(path)
    except OSError as e:  # e.g. libamdhip64 missing
        raise MetranHipError("cannot load %s: %s" % (path, e)) from e
    for name, (res, args) in API.items():
        try:
            fn = getattr(L, name)
        except AttributeError as e:
            raise MetranHipError("%s does not export %s (stale build?)" % (path, name)) from e
        fn.restype = res
        fn.argtypes = args
    if L.mk_abi_version() != ABI_VERSION:
        raise MetranHipError("ABI version mismatch: library %d, binding %d" % (L.mk_abi_version(), ABI_VERSION))
    _lib = L
    return L


def check(rc):
    if rc != 0:
        msg = lib().mk_last_error()
        raise MetranHipError("libmetran_hip error %d: %s" % (rc, (msg or b"").decode("utf-8", "replace")))
