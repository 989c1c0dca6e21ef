"""ctypes binding of libbeta_cores.so (the C ABI declared in include/beta_cores.h).

There is no CPU fallback: if the shared library is missing, or no gfx950 device is
visible, the calls below raise.  Status codes map to the reference's exception
types: 1 -> NumericalPrecisionError, 2 -> ValueError, <0 -> RuntimeError.
"""
import ctypes as C
import os

from .util.errors import NumericalPrecisionError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('BETA_CORES_LIB') or os.path.join(_HERE, 'libbeta_cores.so')   # override: A/B builds side by side

BC_OK, BC_NUMERICAL_PRECISION, BC_INVALID_ARGUMENT, BC_RETRY_EXACT = 0, 1, 2, 3
ALG_GIGA, ALG_FW, ALG_OMP = 0, 1, 2
TILE_ROWS = 128

c_i64p = C.POINTER(C.c_int64)
c_i32p = C.POINTER(C.c_int32)
c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int)
vp = C.c_void_p
vpp = C.POINTER(C.c_void_p)

# name -> argtypes ; every function returns int except the two noted below
_SIGNATURES = {
    'bc_ctx_create': [C.c_int, vp, vpp],
    'bc_ctx_destroy': [vp],
    'bc_ctx_sync': [vp],
    'bc_ctx_kernel_time': [vp, C.c_int, c_dp, c_i64p],
    'bc_ctx_kernel_time_reset': [vp],
    'bc_ctx_enable_timing': [vp, C.c_int],
    'bc_ctx_timing_classes': [vp, C.c_uint32],
    'bc_ctx_phase_times': [vp, vp, C.c_int32, c_i64p, C.c_int],
    'bc_data_from_host': [vp, vp, C.c_int64, C.c_int32, vpp],
    'bc_data_from_device': [vp, vp, C.c_int64, C.c_int32, vpp],
    'bc_data_create': [vp, C.c_int64, C.c_int32, vpp],
    'bc_data_upload': [vp, vp, C.c_int64],
    'bc_data_gather_rows': [vp, vp, C.c_int64, vp],
    'bc_data_zero_feature_keys': [vp, C.c_int32, C.c_int64, vp, C.POINTER(C.c_int64)],
    'bc_ctx_set_constant_row_values': [vp, C.c_int, vp, C.c_int32, vp, vp, C.c_int64],
    'bc_data_destroy': [vp],
    'bc_phi_from_host': [vp, vp, C.c_int64, C.c_int32, C.c_int64, vpp],
    'bc_phi_create': [vp, C.c_int64, C.c_int32, vpp],
    'bc_project': [vp, vp, C.c_int, vp, C.c_int32, vp, C.c_int32, C.c_int64, vpp],
    'bc_project_from_host': [vp, vp, C.c_int64, C.c_int32, C.c_int, vp, C.c_int32, vp, C.c_int32, C.c_int64, vpp, vpp],
    'bc_project_grad_x': [vp, vp, C.c_int, vp, C.c_int32, vp, C.c_int32, vp],
    'bc_project_colsum': [vp, vp, C.c_int, vp, C.c_int32, vp, C.c_int32, vp, vp],
    'bc_vi_gradient': [vp, vp, vp, C.c_int64, C.c_int, vp, C.c_int32, vp, C.c_int32, vp, C.c_double, vp, vp, vp],
    'bc_vi_gradient_begin': [vp, vp, vp, C.c_int64, C.c_int, vp, C.c_int32, vp, C.c_int32, vp, C.c_double, vp],
    'bc_vi_gradient_end': [vp, vp, vp],
    'bc_phi_shape': [vp, c_i64p, c_i32p, c_i64p],
    'bc_phi_colsum': [vp, vp],
    'bc_phi_norms': [vp, vp],
    'bc_phi_norm_stats': [vp, c_i64p, c_dp],
    'bc_phi_to_host': [vp, vp],
    'bc_phi_group_sum': [vp, vp, vp, C.c_int64, vpp],
    'bc_phi_gather_rows': [vp, vp, C.c_int64, vp],
    'bc_phi_matvec': [vp, vp, vp],
    'bc_phi_destroy': [vp],
    'bc_phi_argmax': [vp, C.c_int, vp, C.c_double, c_i64p, c_dp],
    'bc_snnls_create': [vp, vp, vp, C.c_int, C.c_double, C.c_int, vpp],
    'bc_snnls_destroy': [vp],
    'bc_snnls_set_tolerance': [vp, C.c_double],
    'bc_comm_load': [C.c_char_p],
    'bc_comm_unique_id': [vp, C.c_int32],
    'bc_comm_create': [vp, vp, C.c_int32, C.c_int32, vpp],
    'bc_comm_destroy': [vp],
    'bc_comm_info': [vp, c_i32p, c_i32p],
    'bc_comm_all_gather': [vp, vp, vp, C.c_int64],
    'bc_comm_selftest': [vp],
    'bc_comm_precheck': [vp],
    'bc_comm_abort': [vp],
    'bc_comm_sum_doubles': [vp, vp, C.c_int64, vp],
    'bc_comm_rank_order_sum_selftest': [vp, vp, C.c_int32, C.c_int64, vp],
    'bc_phi_colsum_all': [vp, vp, vp],
    'bc_snnls_bind_comm': [vp, vp],
    'bc_snnls_prefilter_active': [vp, c_ip],
    'bc_snnls_prefilter_form': [vp, c_ip],
    'bc_snnls_finish_form': [vp, c_ip],
    'bc_snnls_prefilter_fallbacks': [vp, C.POINTER(C.c_int64)],
    'bc_snnls_prefilter_stats': [vp, c_i64p, c_i64p, c_i64p],
    'bc_snnls_prefilter_levels': [vp, c_i64p, c_i64p, c_i64p],
    'bc_snnls_bind_exchange': [vp, C.c_int, vp, vp],
    'bc_snnls_record_doubles': [vp, c_i32p],
    'bc_snnls_build_begin': [vp, C.c_int],
    'bc_snnls_step_local': [vp],
    'bc_snnls_step_local_exact': [vp],
    'bc_snnls_step_finish': [vp],
    'bc_snnls_build_end': [vp, c_ip, c_ip, c_ip],
    'bc_snnls_build': [vp, C.c_int, c_ip],
    'bc_snnls_select': [vp, c_i64p],
    'bc_snnls_select_local': [vp],
    'bc_snnls_select_local_exact': [vp],
    'bc_snnls_select_pick': [vp, c_i64p],
    'bc_snnls_reweight': [vp, C.c_int64],
    'bc_snnls_error': [vp, c_dp],
    'bc_snnls_size': [vp, c_i64p],
    'bc_snnls_weights': [vp, C.c_int64, vp, vp, c_i64p],
    'bc_snnls_set_weights': [vp, C.c_int64, vp, vp, vp],
    'bc_snnls_columns': [vp, C.c_int64, vp, c_i64p],
    'bc_snnls_reset': [vp],
    'bc_snnls_get_flags': [vp, c_ip],
    'bc_snnls_set_flags': [vp, C.c_int],
    'bc_snnls_trace': [vp, C.c_int64, vp, vp, vp, c_i64p],
    'bc_weighted_gram': [vp, vp, vp, vp, vp],
    'bc_weighted_gram_host': [vp, vp, C.c_int64, C.c_int32, vp, vp, vp],
}
EXPORTS = sorted(list(_SIGNATURES) + ['bc_version', 'bc_last_error'])

# entry points of the extension header include/beta_cores_laplace.h (same library, same status conventions)
_EXT_SIGNATURES = {
    'bc_logistic_newton_pass': [vp, vp, vp, vp, vp, vp, vp, vp],
}
EXT_EXPORTS = sorted(_EXT_SIGNATURES)

# entry points of the extension header include/beta_cores_f32.h (float32 data rows; same library, same status conventions)
_F32_SIGNATURES = {
    'bc_data_from_host_f32': [vp, vp, C.c_int64, C.c_int32, vpp],
    'bc_data_from_device_f32': [vp, vp, C.c_int64, C.c_int32, vpp],
    'bc_project_from_host_f32': [vp, vp, C.c_int64, C.c_int32, C.c_int, vp, C.c_int32, vp, C.c_int32, C.c_int64, vpp, vpp],
    'bc_data_elem_bytes': [vp, vp],
}
F32_EXPORTS = sorted(_F32_SIGNATURES)

# entry points of the extension header include/beta_cores_nnls.h (device NNLS refit: OrthoPursuit in the fused loop, optimize())
_NNLS_SIGNATURES = {
    'bc_snnls_device_refit': [vp, C.c_int],
    'bc_snnls_refit': [vp, C.c_int64],
    'bc_snnls_optimize': [vp, c_ip],
    'bc_snnls_refit_stats': [vp, c_i64p, c_i64p, c_i64p],
}
NNLS_EXPORTS = sorted(_NNLS_SIGNATURES)

# entry points of the extension header include/beta_cores_take.h (resident rows sub-sampled on the device)
_TAKE_SIGNATURES = {
    'bc_data_take_rows': [vp, vp, C.c_int64, vpp],
}
TAKE_EXPORTS = sorted(_TAKE_SIGNATURES)

# entry points of the extension header include/beta_cores_betagrad.h (beta-gradients of the regression models, the fused (w, beta) gradient)
_BETAGRAD_SIGNATURES = {
    'bc_model_beta_grad': [C.c_int],      # returns a model id (or -1), not a status
    'bc_vi_beta_gradient': [vp, vp, vp, C.c_int64, C.c_int, vp, C.c_int32, vp, C.c_int32, vp, C.c_double, vp, vp, vp, vp],
    'bc_vi_beta_gradient_begin': [vp, vp, vp, C.c_int64, C.c_int, vp, C.c_int32, vp, C.c_int32, vp, C.c_double, vp],
    'bc_vi_beta_gradient_end': [vp, vp, vp, vp],
}
BETAGRAD_EXPORTS = sorted(_BETAGRAD_SIGNATURES)

# entry points of the extension header include/beta_cores_encode.h (the device feature encoder of the neural-linear model)
_ENCODE_SIGNATURES = {
    'bc_encoder_create': [vp, C.c_int32, vp, vpp],
    'bc_encoder_set_layer': [vp, C.c_int32, vp, vp, vp, vp, C.c_int32],
    'bc_encoder_destroy': [vp],
    'bc_data_encode': [vp, vp, C.c_int32, C.c_int32, vpp],
}
ENCODE_EXPORTS = sorted(_ENCODE_SIGNATURES)

# entry points of the extension header include/beta_cores_viopt.h (the greedy-VI weight optimisation enqueued on the device)
_VIOPT_SIGNATURES = {
    'bc_vi_optimize_auto_chunk': [C.c_int32, C.c_int32, C.c_int64],      # returns a step count, not a status
    'bc_vi_optimize_begin': [vp, vp, vp, C.c_int64, C.c_int, vp, C.c_int32, C.c_int, vp, C.c_int32, vp, C.c_int32, vp, C.c_int64,
                             C.c_double, C.c_int],
    'bc_vi_optimize_chunk_begin': [vp, vp, vp, C.c_int32],
    'bc_vi_optimize_chunk_end': [vp],
    'bc_vi_optimize_end': [vp, vp, vp],
    'bc_vi_optimize_device_ms': [vp, c_dp],
    'bc_vi_optimize_last_draw': [vp, C.c_int32, C.c_int32, vp, vp, vp, c_dp],
    'bc_vi_optimize': [vp, vp, vp, C.c_int64, C.c_int, vp, C.c_int32, C.c_int, vp, C.c_int32, vp, C.c_int32, vp, vp, vp, C.c_int64,
                       C.c_double, C.c_int32, vp, vp],
}
VIOPT_EXPORTS = sorted(_VIOPT_SIGNATURES)

# entry points of the extension header include/beta_cores_psvi.h (BatchPSVICoreset's gradient, weights and points, in one call)
_PSVI_SIGNATURES = {
    'bc_psvi_gradient': [vp, vp, vp, C.c_int64, C.c_int, vp, C.c_int32, vp, C.c_int32, vp, C.c_double, vp, vp, vp],
    'bc_psvi_gradient_begin': [vp, vp, vp, C.c_int64, C.c_int, vp, C.c_int32, vp, C.c_int32, vp, C.c_double],
    'bc_psvi_gradient_end': [vp, vp, vp, vp],
}
PSVI_EXPORTS = sorted(_PSVI_SIGNATURES)

# entry points of the extension header include/beta_cores_vilaplace.h (the seam behind the logistic sampler of the device loop)
_VILAPLACE_SIGNATURES = {
    'bc_vi_laplace_last_mode': [vp, C.c_int32, vp, vp],
}
VILAPLACE_EXPORTS = sorted(_VILAPLACE_SIGNATURES)

# entry points of the extension header include/beta_cores_hmc.h (multi-chain HMC of the logistic posterior, the multi-chain rows pass)
_HMC_SIGNATURES = {
    'bc_logistic_logjoint_batch': [vp, vp, vp, vp, C.c_int32, vp, vp],
    'bc_hmc_auto_chunk': [C.c_int32, C.c_int32],      # returns an iteration count, not a status
    'bc_hmc_begin': [vp, vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int64],
    'bc_hmc_chunk_begin': [vp, vp, vp, C.c_int32, C.c_double],
    'bc_hmc_chunk_end': [vp, vp, vp, vp],
    'bc_hmc_end': [vp],
    'bc_hmc_device_ms': [vp, c_dp],
    'bc_hmc_logistic': [vp, vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_double, C.c_int64, vp, vp, C.c_int32, vp, vp, vp],
}
HMC_EXPORTS = sorted(_HMC_SIGNATURES)

# entry points of the extension header include/beta_cores_hmc_small.h (many small logistic posteriors sampled at once, one block each)
_HMC_SMALL_SIGNATURES = {
    'bc_hmc_small_fits': [vp, C.c_int64, C.c_int32],      # returns 1 / 0, not a status
    'bc_hmc_small_logjoint': [vp, vp, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, vp, vp],
    'bc_hmc_small_begin': [vp, vp, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, vp, C.c_int32, C.c_int64],
    'bc_hmc_small_chunk_begin': [vp, vp, vp, C.c_int64, C.c_int32, vp],
    'bc_hmc_small_chunk_end': [vp, vp, vp, vp, vp],
    'bc_hmc_small_end': [vp],
    'bc_hmc_small_device_ms': [vp, c_dp],
}
HMC_SMALL_EXPORTS = sorted(_HMC_SMALL_SIGNATURES)

# entry points of the extension header include/beta_cores_score.h (held-out accuracy counts and log-likelihoods of many thetas at once)
_SCORE_SIGNATURES = {
    'bc_lr_score': [vp, vp, vp, vp, C.c_int64, vp, vp],
    'bc_score_chunk': [vp, vp, vp],
    'bc_score_chunk_end': [vp, vp, vp, vp, vp, vp, vp],
}
SCORE_EXPORTS = sorted(_SCORE_SIGNATURES)

# entry points of the extension header include/beta_cores_laplace_small.h (many small logistic posteriors Laplace-fitted at once, one block each)
_LAPLACE_SMALL_SIGNATURES = {
    'bc_laplace_small': [vp, vp, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, vp, C.c_int64, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                         vp, vp],
    'bc_laplace_small_device_ms': [vp, c_dp],
}
LAPLACE_SMALL_EXPORTS = sorted(_LAPLACE_SMALL_SIGNATURES)

# entry points of the extension header include/beta_cores_predict.h (held-out Gaussian predictive scores of the linear-regression family)
_PREDICT_SIGNATURES = {
    'bc_linreg_predict': [vp, vp, vp, vp, vp, vp, C.c_int64, vp, vp, vp, vp],
}
PREDICT_EXPORTS = sorted(_PREDICT_SIGNATURES)

# entry points of the extension header include/beta_cores_prefdiag.h (test aids: the pre-filter's mirrors and per-row bounds)
_PREFDIAG_SIGNATURES = {
    'bc_snnls_prefdiag_info': [vp, c_i64p],
    'bc_snnls_prefdiag_copy': [vp, C.c_char_p, vp, C.c_int64, c_i64p],
    'bc_snnls_prefdiag_sweep': [vp, C.c_int32, vp, C.c_double, C.c_int32, vp, vp, vp, C.c_int64, C.c_int32, c_i32p],
}
PREFDIAG_EXPORTS = sorted(_PREFDIAG_SIGNATURES)

# entry points of the extension header include/beta_cores_psvi_many.h (BatchPSVI pseudo-coresets of many sizes in one device run)
_PSVI_MANY_SIGNATURES = {
    'bc_psvi_many_work_doubles': [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32],      # returns an int64 count, not a status
    'bc_psvi_many_auto_chunk': [C.c_int32, C.c_int32, C.c_int64],      # returns a step count, not a status
    'bc_psvi_many_begin': [vp, vp, C.c_int, C.c_int, C.c_int32, vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, C.c_int64, C.c_double],
    'bc_psvi_many_chunk_begin': [vp, vp, vp, C.c_int32],
    'bc_psvi_many_chunk_end': [vp, vp],
    'bc_psvi_many_end': [vp, vp, vp, vp, vp],
    'bc_psvi_many_device_ms': [vp, c_dp],
    'bc_psvi_many_last_step': [vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32] + [vp] * 16,
}
PSVI_MANY_EXPORTS = sorted(_PSVI_MANY_SIGNATURES)

# include/beta_cores_psvi_curve.h: the batched BatchPSVI run begun with a kind (the Gaussian-location model); a table of its own,
# the one above is left as it is
_PSVI_CURVE_SIGNATURES = {
    'bc_psvi_curve_work_doubles': [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int],      # returns an int64 count, not a status
    'bc_psvi_curve_begin': [vp, vp, C.c_int, C.c_int, C.c_int32, vp, vp, vp, C.c_int32, vp, C.c_int32, C.c_int32, vp, vp, C.c_int64, C.c_double,
                                vp, C.c_int32, vp, C.c_int32],
}
PSVI_CURVE_EXPORTS = sorted(_PSVI_CURVE_SIGNATURES)

# entry points of the extension header include/beta_cores_diag.h (posterior moments, split-R-hat and ESS of HMC chains on the device)
_DIAG_SIGNATURES = {
    'bc_diag_work_doubles': [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int64],      # returns an int64 count, not a status
    'bc_chain_summary': [vp, vp, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp],
    'bc_diag_attach': [vp, C.c_int64, C.c_int64],
    'bc_diag_chunk': [vp],
    'bc_diag_end': [vp, vp, vp, vp, vp, vp, vp, vp, vp],
}
DIAG_EXPORTS = sorted(_DIAG_SIGNATURES)

# entry points of the extension header include/beta_cores_hmc_adapt.h (the per-chain warm-up of an open batched small-problem run)
_HMC_ADAPT_SIGNATURES = {
    'bc_hmc_adapt_plan': [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, vp, vp],
    'bc_hmc_adapt_begin': [vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int32, C.c_int32, C.c_int32],
    'bc_hmc_adapt_chunk_begin': [vp, vp, vp, C.c_int64, C.c_int32],
    'bc_hmc_adapt_chunk_end': [vp, vp, vp, vp, vp, vp, vp],
    'bc_hmc_adapted_chunk_begin': [vp, vp, vp, C.c_int64, C.c_int32],
    'bc_hmc_adapt_state': [vp, vp, vp],
}
HMC_ADAPT_EXPORTS = sorted(_HMC_ADAPT_SIGNATURES)

_lib = None


def _preload_torch_hip_runtime():
    """PyTorch-ROCm ships its own libamdhip64 (same SONAME as /opt/rocm's).  A process must run ONE HIP
    runtime: if ours resolved to the system copy first, a later `import torch` would find a runtime it was
    not built against ("no ROCm-capable device is detected").  So when torch is installed, map its copy
    first -- without importing torch -- and let the loader hand that one to libbeta_cores.so as well."""
    try:
        import importlib.util
        spec = importlib.util.find_spec('torch')
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], 'lib', 'libamdhip64.so')
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def load():
    """Load the shared library (once).  Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            'beta_cores_amd: %s is missing -- build it with `python -c "import __graft_entry__ as g; g.build()"` '
            'or `make -C beta_cores_amd/csrc`. There is no CPU fallback.' % LIB_PATH)
    _preload_torch_hip_runtime()
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in list(_SIGNATURES.items()) + list(_EXT_SIGNATURES.items()) + list(_F32_SIGNATURES.items()) + list(_NNLS_SIGNATURES.items()) \
            + list(_TAKE_SIGNATURES.items()) + list(_BETAGRAD_SIGNATURES.items()) + list(_ENCODE_SIGNATURES.items()) \
            + list(_VIOPT_SIGNATURES.items()) + list(_PSVI_SIGNATURES.items()) + list(_VILAPLACE_SIGNATURES.items()) \
            + list(_HMC_SIGNATURES.items()) + list(_HMC_SMALL_SIGNATURES.items()) + list(_SCORE_SIGNATURES.items()) \
            + list(_PREFDIAG_SIGNATURES.items()) + list(_PREDICT_SIGNATURES.items()) + list(_LAPLACE_SMALL_SIGNATURES.items()) \
            + list(_PSVI_MANY_SIGNATURES.items()) + list(_PSVI_CURVE_SIGNATURES.items()) + list(_DIAG_SIGNATURES.items()) \
            + list(_HMC_ADAPT_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    lib.bc_diag_work_doubles.restype = C.c_int64
    lib.bc_psvi_many_work_doubles.restype = C.c_int64
    lib.bc_psvi_curve_work_doubles.restype = C.c_int64
    lib.bc_version.restype = C.c_int
    lib.bc_version.argtypes = []
    lib.bc_last_error.restype = C.c_char_p
    lib.bc_last_error.argtypes = []
    _lib = lib
    return lib


def last_error():
    return load().bc_last_error().decode('utf-8', 'replace')


def check(status):
    """Translate a C status into the reference's exception conventions."""
    if status == BC_OK:
        return
    msg = last_error()
    if status == BC_NUMERICAL_PRECISION:
        raise NumericalPrecisionError(msg)
    if status == BC_INVALID_ARGUMENT:
        raise ValueError(msg)
    raise RuntimeError('beta_cores HIP failure (%d): %s' % (status, msg))


def call(name, *args):
    check(getattr(load(), name)(*args))
