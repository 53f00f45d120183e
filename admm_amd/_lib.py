"""ctypes binding of libadmm_hip.so (the C ABI declared in include/admm_hip.h).

The library is built in-tree by `python -m admm_amd.build` (hipcc, gfx950).  There is no CPU
fallback: if the shared object is missing or no HIP device is usable, calls raise.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ADMM_HIP_LIB") or os.path.join(_HERE, "lib", "libadmm_hip.so")      # ADMM_HIP_LIB: A/B builds (dev)

ADMM_MEM_HOST = 0
ADMM_MEM_DEVICE = 1


class AdmmOpts(ctypes.Structure):
    _fields_ = [("maxit", ctypes.c_int), ("eps_abs", ctypes.c_double),
                ("eps_rel", ctypes.c_double), ("rho", ctypes.c_double)]


class AdmmHipOptions(ctypes.Structure):
    """include/admm_hip.h: admm_hip_options (variant selectors of the calling thread; every field 0 = library default)."""
    _fields_ = [(k, ctypes.c_int) for k in (
        "struct_size", "gram_backend", "gram_split", "factor_backend", "inverse_precision", "tall_xupdate", "tall_refine",
        "consensus_two_pass", "consensus_unfused", "bp_two_pass", "lad_no_hat", "wide_no_persist", "wide_unfused", "wide_gram_sprad",
        "sharing_bp_direct", "cv_downdate", "peer_exchange", "batch_iters", "profile_stride", "pool_mb", "screen", "lad_two_pass",
        "par_devices")] + [("reserved", ctypes.c_int * 9)]


class AdmmStats(ctypes.Structure):
    _fields_ = [("t_h2d", ctypes.c_double), ("t_standardize", ctypes.c_double), ("t_gram", ctypes.c_double),
                ("t_eigs", ctypes.c_double), ("t_factor", ctypes.c_double), ("t_loop", ctypes.c_double),
                ("t_total", ctypes.c_double), ("loop_ms_events", ctypes.c_double),
                ("xupdate_ms_avg", ctypes.c_double), ("xupdate_samples", ctypes.c_longlong),
                ("total_iter", ctypes.c_longlong), ("xupdate_launches", ctypes.c_longlong),
                ("rho", ctypes.c_double), ("eig_est", ctypes.c_double),
                ("branch", ctypes.c_int), ("xupdate_variant", ctypes.c_int),
                ("exchange_variant", ctypes.c_int), ("refine", ctypes.c_int), ("persist_iter", ctypes.c_longlong),
                ("factor_flops", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AdmmHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libadmm_hip error {code}: {msg}")
        self.code = code


_lib = None

_DP = ctypes.c_void_p      # raw pointers: host numpy buffers or device addresses
_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_float_p = ctypes.POINTER(ctypes.c_float)
_c_int_p = ctypes.POINTER(ctypes.c_int)

# every symbol include/admm_hip.h declares
EXPORTS = ["admm_hip_lasso", "admm_hip_enet", "admm_hip_parlasso", "admm_hip_lad", "admm_hip_bp",
           "admm_hip_last_error", "admm_hip_version", "admm_hip_device_count", "admm_hip_set_device",
           "admm_hip_device_synchronize", "admm_hip_lasso_plan_create", "admm_hip_lasso_plan_run",
           "admm_hip_lasso_plan_destroy", "admm_hip_comm_unique_id", "admm_hip_comm_init", "admm_hip_comm_finalize", "admm_hip_comm_info",
           "admm_hip_parlasso_dist", "admm_hip_lasso_plan_create_dist",
           "admm_hip_lasso_plan_trace_enable", "admm_hip_lasso_plan_trace_read",
           "admm_hip_lasso_plan_state_enable", "admm_hip_lasso_plan_state_read", "admm_hip_lasso_plan_system_read",
           "admm_hip_host_lanczos", "admm_hip_test_symv",
           "admm_hip_comm_peer_prepare", "admm_hip_comm_init_peer", "admm_hip_comm_init_shm", "admm_hip_comm_test_allreduce", "admm_hip_comm_test_reduce_scatter",
           "admm_hip_lasso_dist", "admm_hip_test_gram", "admm_hip_test_spd_inverse", "admm_hip_test_cv_fold_system",
           "admm_hip_lasso_dist_cols", "admm_hip_test_gemv_t", "admm_hip_lad_traced", "admm_hip_bp_traced",
           "admm_hip_lasso_plan_create_dist_cols", "admm_hip_lasso_cv", "admm_hip_lasso_multi",
           "admm_hip_parbp", "admm_hip_parbp_traced", "admm_hip_parbp_dist", "admm_hip_dantzig", "admm_hip_dantzig_traced",
           "admm_hip_lad_state", "admm_hip_bp_state", "admm_hip_lasso_plan_data_read", "admm_hip_trim_memory", "admm_hip_test_gather",
           "admm_hip_options_default", "admm_hip_options_set", "admm_hip_option_set", "admm_hip_options_reset", "admm_hip_option_get",
           "admm_hip_last_parallel_layout", "admm_hip_parallel_assign", "admm_hip_grplasso", "admm_hip_grplasso_plan_create",
           "admm_hip_quantreg", "admm_hip_quantreg_state", "admm_hip_huber", "admm_hip_huber_state",
           "admm_hip_logit", "admm_hip_logit_state", "admm_hip_logit_multi", "admm_hip_logit_ridge", "admm_hip_logit_ridge_state",
           "admm_hip_logit_enet", "admm_hip_logit_enet_lambda_max", "admm_hip_logit_enet_state", "admm_hip_test_logit_prox",
           "admm_hip_poisson", "admm_hip_poisson_lambda_max", "admm_hip_poisson_state", "admm_hip_test_poisson_prox",
           "admm_hip_logit_enet_cv", "admm_hip_logit_enet_cv_state", "admm_hip_poisson_cv", "admm_hip_poisson_cv_state",
           "admm_hip_mtlasso", "admm_hip_mtlasso_plan_create", "admm_hip_test_symv_multi", "admm_hip_test_tall_early_exits",
           "admm_hip_sgl", "admm_hip_sgl_plan_create", "admm_hip_host_sgl_lambda0",
           "admm_hip_boxenet", "admm_hip_boxenet_plan_create", "admm_hip_host_box_lambda0",
           "admm_hip_test_gemm_nt", "admm_hip_test_cholesky_linvt", "admm_hip_test_spd_inverse_shift",
           "admm_hip_test_symv_plan", "admm_hip_test_symv_ex", "admm_hip_test_symv_multi_ex", "admm_hip_test_symv_f64acc",
           "admm_hip_test_symv_one", "admm_hip_test_symv_pack_host", "admm_hip_test_symv_packed", "admm_hip_test_symv_packed_time",
           "admm_hip_test_tall_pack_info", "admm_hip_test_gemv_t_ex", "admm_hip_test_wide_op", "admm_hip_test_block_sprad",
           "admm_hip_test_wide_screen_prep", "admm_hip_test_sbp_screen_prep", "admm_hip_test_tall_gate", "admm_hip_test_tall_norms"]

GROUP_MAX = 1024          # ADMM_HIP_GROUP_MAX
MT_MAX = 16               # ADMM_HIP_MT_MAX
MT_RHS_BUILT = (2, 4, 8, 12)      # right-hand sides per pass the multi-vector kernel is built for (option MT_RHS; 0 = automatic)

# the entry points of the tall-only penalties (each with its <name>_plan_create): the argument types that replace [at:5] of the Lasso's
_GROUP_ARGS = [_c_int_p, _c_double_p, ctypes.c_int]
TALL_ONLY = [("admm_hip_grplasso", _GROUP_ARGS, 5), ("admm_hip_sgl", _GROUP_ARGS + [_c_double_p, ctypes.c_double], 5),
             ("admm_hip_boxenet", [_c_double_p] * 3 + [ctypes.c_double], 5), ("admm_hip_mtlasso", [ctypes.c_int, ctypes.c_int, _c_double_p], 4)]

# the dense entry points (basis pursuit, LAD and the losses on LAD's loop; admm_amd/api.py reaches all of them through _dense_call):
#   admm_hip_<loss>(x, y, n, p[, k], mem, after_mem..., grid arrays...[, their length], opts, beta, niter, stats)
#   <loss>_traced: never k or a grid, and one record block (buffer, capacity, count out); <loss>_state: never k, ONE value per grid
#   array and two record blocks (trace, state); <loss>_lambda_max(x, y, n, p, k, mem, after_mem..., out)
_RECORDS = [_c_double_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
_INT = [ctypes.c_int]          # after mem: the intercept flag (admm_hip_parbp: nthread)
#         loss           k      after mem  grid arrays         length  _traced  _state  _lambda_max  _cv
DENSE = [("bp",          False, [],        [],                 False,  True,    True,   False,       False),
         ("parbp",       False, _INT,      [],                 False,  True,    False,  False,       False),
         ("lad",         False, _INT,      [],                 False,  True,    True,   False,       False),
         ("quantreg",    False, _INT,      [_c_double_p],      True,   False,   True,   False,       False),
         ("huber",       False, _INT,      [_c_double_p] * 2,  True,   False,   True,   False,       False),
         ("logit",       False, _INT,      [],                 False,  False,   True,   False,       False),
         ("logit_multi", True,  _INT,      [],                 False,  False,   False,  False,       False),
         ("logit_ridge", True,  _INT,      [_c_double_p],      True,   False,   True,   False,       False),
         ("logit_enet",  True,  _INT,      [_c_double_p] * 2,  True,   False,   True,   True,        True),
         ("poisson",     True,  _INT,      [_c_double_p] * 2,  True,   False,   True,   True,        True)]
#   <loss>_cv: the grid form with the folds (fold_id, nfolds) behind `after mem` and the tables cv_mean, cv_se, fold_dev, fold_niter,
#   fold_beta, idx_min, idx_1se between niter and stats; <loss>_cv_state: the _state form with fold_id, nfolds and the fold held out
_FOLDS = [_c_int_p, ctypes.c_int]
_CV_TABLES = [_c_double_p] * 3 + [_c_int_p, _c_double_p, _c_int_p, _c_int_p]

TRACE_FIELDS = 12
TRACE_COLD, TRACE_CONVERGED, TRACE_ACCELERATE, TRACE_RESTART = -1, 0, 1, 2
TRACE_CONTINUE = 1


def load():
    """Load the shared library (once). Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("ADMM_HIP_LIB") or LIB_PATH     # ADMM_HIP_LIB: another build of the SAME library (the host-sanitizer variant)
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} not found: build it with `python -m admm_amd.build` (hipcc --offload-arch=gfx950). "
            "admm_amd has no CPU fallback.")
    if not os.environ.get("ADMM_HIP_LIB"):
        # the in-tree library must have been linked from the sources beside it (admm_amd/build.py keeps their hash in a side file):
        # a stale prebuilt .so against a newer ctypes layout is an ABI mismatch, not just stale behaviour
        from . import build as _build
        if os.path.isdir(_build.CSRC) and not _build._lib_is_current(path):
            raise RuntimeError(f"{path} was not built from the sources in {_build.CSRC} (source hash differs or is missing): "
                               "run `python -m admm_amd.build`")
    lib = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    lasso_args = [_DP, _DP, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                  _DP, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int]
    tail = [ctypes.POINTER(AdmmOpts), _c_double_p, _c_float_p, _c_int_p, ctypes.POINTER(AdmmStats)]
    lib.admm_hip_lasso.argtypes = lasso_args + tail
    lib.admm_hip_enet.argtypes = lasso_args + [ctypes.c_double] + tail
    lib.admm_hip_parlasso.argtypes = lasso_args + [ctypes.c_int] + tail
    lib.admm_hip_lasso_cv.argtypes = ([_DP, _DP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_int_p, ctypes.c_int,
                                       _DP, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                       ctypes.POINTER(AdmmOpts), _c_double_p, _c_float_p, _c_int_p,
                                       _c_double_p, _c_double_p, _c_double_p, _c_int_p, _c_float_p, _c_int_p, _c_int_p,
                                       ctypes.POINTER(AdmmStats)])
    lib.admm_hip_lasso_cv.restype = ctypes.c_int
    lib.admm_hip_lasso_multi.argtypes = ([_DP, _DP, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          _DP, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                          ctypes.POINTER(AdmmOpts), _c_double_p, _c_float_p, _c_int_p, ctypes.POINTER(AdmmStats)])
    lib.admm_hip_lasso_multi.restype = ctypes.c_int
    dense_out = [ctypes.POINTER(AdmmOpts), _c_double_p, _c_int_p, ctypes.POINTER(AdmmStats)]
    for loss, has_k, after_mem, grid, count, traced, state, lambda_max, cv in DENSE:
        head = [_DP, _DP, ctypes.c_int, ctypes.c_int, ctypes.c_int] + after_mem               # x, y, n, p, mem, ...
        head_k = head[:4] + [ctypes.c_int] + head[4:] if has_k else head
        forms = [("", head_k + grid + [ctypes.c_int] * count + dense_out)]
        if traced:
            forms.append(("_traced", head + dense_out + _RECORDS))
        if state:
            forms.append(("_state", head + [g._type_ for g in grid] + dense_out + _RECORDS * 2))
        if lambda_max:
            forms.append(("_lambda_max", head_k + [_c_double_p]))
        if cv:
            forms.append(("_cv", head_k + _FOLDS + grid + [ctypes.c_int] * count + dense_out[:3] + _CV_TABLES + dense_out[3:]))
            forms.append(("_cv_state", head + _FOLDS + [ctypes.c_int] + [g._type_ for g in grid] + dense_out + _RECORDS * 2))
        for suffix, args in forms:
            fn = getattr(lib, "admm_hip_" + loss + suffix)
            fn.argtypes, fn.restype = args, ctypes.c_int
    lib.admm_hip_test_logit_prox.argtypes = [_c_double_p, ctypes.c_longlong, ctypes.c_double, _c_double_p]
    lib.admm_hip_test_logit_prox.restype = ctypes.c_int
    lib.admm_hip_test_poisson_prox.argtypes = [_c_double_p, _c_double_p, ctypes.c_longlong, ctypes.c_double, _c_double_p]
    lib.admm_hip_test_poisson_prox.restype = ctypes.c_int
    lib.admm_hip_dantzig.argtypes = [_DP, _DP, ctypes.c_int, ctypes.c_int, ctypes.c_int, _DP, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                     ctypes.c_int, ctypes.c_int, ctypes.POINTER(AdmmOpts), _c_double_p, _c_double_p, _c_int_p, ctypes.POINTER(AdmmStats)]
    lib.admm_hip_dantzig.restype = ctypes.c_int
    lib.admm_hip_dantzig_traced.argtypes = lib.admm_hip_dantzig.argtypes + [_c_double_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
    lib.admm_hip_dantzig_traced.restype = ctypes.c_int
    lib.admm_hip_parbp_dist.argtypes = [_DP, _DP, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                        ctypes.POINTER(AdmmOpts), _c_double_p, _c_int_p, ctypes.POINTER(AdmmStats)]
    lib.admm_hip_parbp_dist.restype = ctypes.c_int
    for name in ("admm_hip_lasso", "admm_hip_enet", "admm_hip_parlasso", "admm_hip_lad", "admm_hip_bp",
                 "admm_hip_device_count", "admm_hip_set_device", "admm_hip_device_synchronize"):
        getattr(lib, name).restype = ctypes.c_int
    lib.admm_hip_set_device.argtypes = [ctypes.c_int]
    lib.admm_hip_last_error.restype = ctypes.c_char_p
    lib.admm_hip_version.restype = ctypes.c_char_p
    lib.admm_hip_lasso_plan_create.argtypes = lasso_args + [ctypes.c_double, ctypes.c_int, ctypes.POINTER(AdmmOpts),
                                               ctypes.POINTER(ctypes.c_void_p), _c_int_p]
    lib.admm_hip_lasso_plan_create.restype = ctypes.c_int
    for name, extra, at in TALL_ONLY:
        args = lasso_args[:at] + extra + lasso_args[5:]
        for fn, rest in ((getattr(lib, name), tail), (getattr(lib, name + "_plan_create"), [tail[0], ctypes.POINTER(ctypes.c_void_p), _c_int_p])):
            fn.argtypes, fn.restype = args + rest, ctypes.c_int
    lib.admm_hip_host_sgl_lambda0.argtypes = [_c_float_p, ctypes.c_int, _c_int_p, _c_double_p, ctypes.c_int, _c_double_p, ctypes.c_double, _c_float_p]
    lib.admm_hip_host_sgl_lambda0.restype = ctypes.c_int
    lib.admm_hip_host_box_lambda0.argtypes = [_c_float_p, ctypes.c_int, _c_float_p, _c_float_p, _c_double_p, ctypes.c_double, _c_float_p]
    lib.admm_hip_host_box_lambda0.restype = ctypes.c_int
    lib.admm_hip_lasso_plan_run.argtypes = [ctypes.c_void_p, _c_double_p, _c_float_p, _c_int_p, ctypes.POINTER(AdmmStats)]
    lib.admm_hip_lasso_plan_run.restype = ctypes.c_int
    lib.admm_hip_lasso_plan_destroy.argtypes = [ctypes.c_void_p]
    lib.admm_hip_lasso_plan_destroy.restype = ctypes.c_int
    dist_args = [_DP, _DP, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                 _DP, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(AdmmOpts)]
    lib.admm_hip_parlasso_dist.argtypes = dist_args + [_c_double_p, _c_float_p, _c_int_p, ctypes.POINTER(AdmmStats)]
    lib.admm_hip_parlasso_dist.restype = ctypes.c_int
    lib.admm_hip_lasso_plan_create_dist.argtypes = dist_args + [ctypes.POINTER(ctypes.c_void_p), _c_int_p]
    lib.admm_hip_lasso_plan_create_dist.restype = ctypes.c_int
    lib.admm_hip_lasso_dist.argtypes = [_DP, _DP, ctypes.c_int, ctypes.c_longlong, ctypes.c_int, ctypes.c_int,
                                        _DP, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                        ctypes.POINTER(AdmmOpts), _c_double_p, _c_float_p, _c_int_p, ctypes.POINTER(AdmmStats)]
    lib.admm_hip_lasso_dist.restype = ctypes.c_int
    lib.admm_hip_lasso_dist_cols.argtypes = [_DP, _DP, ctypes.c_int, ctypes.c_int, ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int,
                                             _DP, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                             ctypes.POINTER(AdmmOpts), _c_double_p, _c_float_p, _c_int_p, ctypes.POINTER(AdmmStats)]
    lib.admm_hip_lasso_dist_cols.restype = ctypes.c_int
    lib.admm_hip_lasso_plan_create_dist_cols.argtypes = lib.admm_hip_lasso_dist_cols.argtypes[:15] + [ctypes.POINTER(ctypes.c_void_p), _c_int_p]
    lib.admm_hip_lasso_plan_create_dist_cols.restype = ctypes.c_int
    lib.admm_hip_comm_unique_id.argtypes = [ctypes.c_void_p]
    lib.admm_hip_comm_unique_id.restype = ctypes.c_int
    lib.admm_hip_comm_init.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.admm_hip_comm_init.restype = ctypes.c_int
    lib.admm_hip_comm_finalize.argtypes = []
    lib.admm_hip_comm_finalize.restype = ctypes.c_int
    lib.admm_hip_options_default.argtypes = [ctypes.POINTER(AdmmHipOptions)]
    lib.admm_hip_options_default.restype = ctypes.c_int
    lib.admm_hip_options_set.argtypes = [ctypes.POINTER(AdmmHipOptions)]
    lib.admm_hip_options_set.restype = ctypes.c_int
    lib.admm_hip_option_set.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    lib.admm_hip_option_set.restype = ctypes.c_int
    lib.admm_hip_options_reset.argtypes = []
    lib.admm_hip_options_reset.restype = ctypes.c_int
    lib.admm_hip_option_get.argtypes = [ctypes.c_char_p]
    lib.admm_hip_option_get.restype = ctypes.c_char_p
    lib.admm_hip_comm_info.argtypes = [ctypes.POINTER(ctypes.c_int)] * 3
    lib.admm_hip_comm_info.restype = ctypes.c_int
    lib.admm_hip_comm_peer_prepare.argtypes = [ctypes.c_int, ctypes.c_void_p]
    lib.admm_hip_comm_peer_prepare.restype = ctypes.c_int
    lib.admm_hip_comm_init_peer.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.admm_hip_comm_init_peer.restype = ctypes.c_int
    lib.admm_hip_comm_init_shm.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.c_ulonglong]
    lib.admm_hip_comm_init_shm.restype = ctypes.c_int
    lib.admm_hip_comm_test_allreduce.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int]
    lib.admm_hip_comm_test_allreduce.restype = ctypes.c_int
    lib.admm_hip_comm_test_reduce_scatter.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_void_p]
    lib.admm_hip_comm_test_reduce_scatter.restype = ctypes.c_int
    lib.admm_hip_lasso_plan_trace_enable.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.admm_hip_lasso_plan_trace_enable.restype = ctypes.c_int
    lib.admm_hip_lasso_plan_trace_read.argtypes = [ctypes.c_void_p, _c_double_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
    lib.admm_hip_lasso_plan_trace_read.restype = ctypes.c_int
    lib.admm_hip_lasso_plan_state_enable.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    lib.admm_hip_lasso_plan_state_enable.restype = ctypes.c_int
    lib.admm_hip_lasso_plan_state_read.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_longlong,
                                                   ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ctypes.c_longlong)]
    lib.admm_hip_lasso_plan_state_read.restype = ctypes.c_int
    lib.admm_hip_lasso_plan_data_read.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_longlong, ctypes.POINTER(ctypes.c_float)]
    lib.admm_hip_lasso_plan_data_read.restype = ctypes.c_int
    lib.admm_hip_lasso_plan_system_read.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_longlong]
    lib.admm_hip_lasso_plan_system_read.restype = ctypes.c_int
    lib.admm_hip_test_symv.argtypes = [_c_float_p, ctypes.c_int, _c_float_p, _c_float_p, _c_float_p, _c_float_p]
    lib.admm_hip_test_symv.restype = ctypes.c_int
    lib.admm_hip_test_symv_multi.argtypes = [_c_float_p, ctypes.c_int, _c_float_p, ctypes.c_int, ctypes.c_int, _c_float_p]
    lib.admm_hip_test_symv_multi.restype = ctypes.c_int
    lib.admm_hip_test_symv_plan.argtypes = [ctypes.c_int] * 4 + [_c_int_p, ctypes.POINTER(ctypes.c_longlong), _c_int_p, ctypes.c_int]
    lib.admm_hip_test_symv_plan.restype = ctypes.c_int
    lib.admm_hip_test_symv_ex.argtypes = [_c_float_p, ctypes.c_int, _c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          _c_float_p, _c_float_p, _c_int_p]
    lib.admm_hip_test_symv_ex.restype = ctypes.c_int
    lib.admm_hip_test_symv_one.argtypes = [_c_float_p, ctypes.c_int, _c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint,
                                           _c_float_p, _c_float_p, _c_float_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong), _c_int_p]
    lib.admm_hip_test_symv_one.restype = ctypes.c_int
    _c_uint_p = ctypes.POINTER(ctypes.c_uint)
    lib.admm_hip_test_symv_pack_host.argtypes = [_c_uint_p, ctypes.c_int, _c_int_p, _c_uint_p, _c_uint_p, ctypes.c_int,
                                                 ctypes.POINTER(ctypes.c_longlong), _c_uint_p]
    lib.admm_hip_test_symv_pack_host.restype = ctypes.c_int
    lib.admm_hip_test_symv_packed.argtypes = [_c_float_p, ctypes.c_int, _c_float_p, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_int,
                                              _c_float_p, _c_float_p, _c_float_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong), _c_int_p]
    lib.admm_hip_test_symv_packed.restype = ctypes.c_int
    lib.admm_hip_test_symv_packed_time.argtypes = [_c_float_p, ctypes.c_int, _c_float_p, ctypes.c_int, _c_float_p, ctypes.POINTER(ctypes.c_longlong)]
    lib.admm_hip_test_symv_packed_time.restype = ctypes.c_int
    lib.admm_hip_test_tall_pack_info.argtypes = [ctypes.POINTER(ctypes.c_longlong)]
    lib.admm_hip_test_tall_pack_info.restype = ctypes.c_int
    lib.admm_hip_test_symv_multi_ex.argtypes = [_c_float_p, ctypes.c_int, _c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                _c_float_p, _c_int_p]
    lib.admm_hip_test_symv_multi_ex.restype = ctypes.c_int
    lib.admm_hip_test_symv_f64acc.argtypes = [_c_float_p, ctypes.c_int, _c_float_p, _c_float_p, _c_double_p, _c_double_p, _c_int_p]
    lib.admm_hip_test_symv_f64acc.restype = ctypes.c_int
    lib.admm_hip_test_tall_early_exits.argtypes = [ctypes.POINTER(ctypes.c_longlong)]
    lib.admm_hip_test_tall_early_exits.restype = ctypes.c_int
    lib.admm_hip_test_tall_gate.argtypes = [_c_double_p, _c_int_p, _c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_double_p, _c_int_p]
    lib.admm_hip_test_tall_gate.restype = ctypes.c_int
    lib.admm_hip_test_tall_norms.argtypes = [_c_double_p, ctypes.c_int, _c_double_p]
    lib.admm_hip_test_tall_norms.restype = ctypes.c_int
    lib.admm_hip_test_gram.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.admm_hip_test_gram.restype = ctypes.c_int
    lib.admm_hip_test_gemv_t.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.admm_hip_test_gemv_t.restype = ctypes.c_int
    _c_void_pp, _c_ll_p = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_longlong)
    lib.admm_hip_test_gemv_t_ex.argtypes = [ctypes.c_int] * 6 + [ctypes.c_ulonglong, ctypes.c_int, _c_int_p, _c_int_p, _c_void_pp, _c_void_pp, _c_int_p,
                                            _c_int_p, _c_void_pp, ctypes.c_longlong, _c_void_pp, _c_ll_p]
    lib.admm_hip_test_gemv_t_ex.restype = ctypes.c_int
    lib.admm_hip_test_wide_op.argtypes = [_c_float_p, ctypes.c_int, ctypes.c_int, _c_float_p, _c_float_p]
    lib.admm_hip_test_wide_op.restype = ctypes.c_int
    lib.admm_hip_test_block_sprad.argtypes = [_c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_double_p, _c_int_p]
    lib.admm_hip_test_block_sprad.restype = ctypes.c_int
    lib.admm_hip_test_wide_screen_prep.argtypes = [_c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p,
                                                   ctypes.c_longlong, _c_float_p, _c_float_p, _c_double_p, _c_ll_p]
    lib.admm_hip_test_wide_screen_prep.restype = ctypes.c_int
    lib.admm_hip_test_sbp_screen_prep.argtypes = [_c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_longlong,
                                                  _c_float_p, _c_ll_p]
    lib.admm_hip_test_sbp_screen_prep.restype = ctypes.c_int
    lib.admm_hip_test_spd_inverse.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.admm_hip_test_spd_inverse.restype = ctypes.c_int
    lib.admm_hip_test_spd_inverse_shift.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_void_p]
    lib.admm_hip_test_spd_inverse_shift.restype = ctypes.c_int
    lib.admm_hip_test_cholesky_linvt.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.admm_hip_test_cholesky_linvt.restype = ctypes.c_int
    lib.admm_hip_test_gemm_nt.argtypes = [ctypes.c_int] * 9 + [ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.admm_hip_test_gemm_nt.restype = ctypes.c_int
    lib.admm_hip_test_cv_fold_system.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.admm_hip_test_cv_fold_system.restype = ctypes.c_int
    lib.admm_hip_host_lanczos.argtypes = [_c_float_p, ctypes.c_int, _c_float_p, _c_int_p]
    lib.admm_hip_host_lanczos.restype = ctypes.c_int
    lib.admm_hip_test_gather.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, _c_double_p]
    lib.admm_hip_test_gather.restype = ctypes.c_int
    lib.admm_hip_last_parallel_layout.argtypes = [_c_int_p, _c_int_p, ctypes.c_int]
    lib.admm_hip_last_parallel_layout.restype = ctypes.c_int
    lib.admm_hip_parallel_assign.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, _c_int_p, _c_int_p, ctypes.c_int]
    lib.admm_hip_parallel_assign.restype = ctypes.c_int
    lib.admm_hip_trim_memory.argtypes = []
    lib.admm_hip_trim_memory.restype = ctypes.c_int
    _lib = lib
    return lib


def check(code):
    if code != 0:
        raise AdmmHipError(code, load().admm_hip_last_error().decode())


class DevicePtr:
    """A raw device address (e.g. torch_tensor.data_ptr()) of column-major float64 data."""

    def __init__(self, ptr):
        self.ptr = int(ptr)


def as_input(a, n=None, p=None):
    """Return (c_void_p, mem, keepalive) for a host array (copied to column-major float64) or a DevicePtr."""
    if isinstance(a, DevicePtr):
        return ctypes.c_void_p(a.ptr), ADMM_MEM_DEVICE, a
    arr = np.asfortranarray(np.asarray(a, dtype=np.float64))
    return ctypes.c_void_p(arr.ctypes.data), ADMM_MEM_HOST, arr


class options:
    """Variant selectors / tuning values of the CALLING THREAD for the duration of a `with` block (admm_hip_option_set; names as in
    INTEGRATION.md, case-insensitive, with or without the ADMM_HIP_ prefix; value None = library default):

        with admm_amd.options(GRAM_SPLIT="f16x2", INVERSE="f64"):
            fit = admm_amd.admm_lasso(x, y).penalty(nlambda=20).fit()

    A prepared problem (LassoPlan) reads them when it is created.  On exit the previous values of exactly these names are restored.
    Fields of the typed struct go through `options.struct(gram_split=2, ...)` (admm_hip_options_set: replaces ALL of the thread's settings)."""

    def __init__(self, **kw):
        self.kw = {k.upper(): (None if v is None else str(v)) for k, v in kw.items()}
        self.old = {}

    def __enter__(self):
        lib = load()
        try:
            for k, v in self.kw.items():
                cur = lib.admm_hip_option_get(k.encode())
                self.old[k] = cur.decode() if cur is not None else None
                check(lib.admm_hip_option_set(k.encode(), None if v is None else v.encode()))
        except BaseException:
            self.__exit__(None, None, None)          # a failure part-way: what was already set goes back
            raise
        return self

    def __exit__(self, *exc):
        lib = load()
        for k, v in self.old.items():
            check(lib.admm_hip_option_set(k.encode(), None if v is None else v.encode()))
        return False

    @staticmethod
    def set(**kw):
        lib = load()
        for k, v in kw.items():
            check(lib.admm_hip_option_set(k.upper().encode(), None if v is None else str(v).encode()))

    @staticmethod
    def reset():
        check(load().admm_hip_options_reset())

    @staticmethod
    def struct(**fields):
        lib = load()
        o = AdmmHipOptions()
        check(lib.admm_hip_options_default(ctypes.byref(o)))
        for k, v in fields.items():
            setattr(o, k, int(v))
        check(lib.admm_hip_options_set(ctypes.byref(o)))
        return o


def last_parallel_layout():
    """Devices of the ranks of the calling thread's last admm_hip_parlasso / admm_hip_parbp call (admm_hip_last_parallel_layout):
    one entry for the single-device path, one per rank with PAR_DEVICES, [] before any such call."""
    lib = load()
    nr = ctypes.c_int(0)
    devs = (ctypes.c_int * 64)()
    check(lib.admm_hip_last_parallel_layout(ctypes.byref(nr), devs, 64))
    return [int(devs[r]) for r in range(min(nr.value, 64))]


def parallel_assign(nblocks, par_devices, device_count):
    """Host-only (admm_hip_parallel_assign): the devices of the ranks a PAR_DEVICES call with `nblocks` blocks would run, [] when it
    runs the single-device path."""
    lib = load()
    nr = ctypes.c_int(0)
    devs = (ctypes.c_int * 64)()
    check(lib.admm_hip_parallel_assign(int(nblocks), None if par_devices is None else str(par_devices).encode(), int(device_count),
                                       ctypes.byref(nr), devs, 64))
    return [int(devs[r]) for r in range(nr.value)] if nr.value > 1 else []
