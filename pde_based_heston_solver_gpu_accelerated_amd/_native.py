"""ctypes binding of libhadi.so (the C ABI declared in include/hadi.h).

The library is the product: if it is missing or no gfx950 GPU is usable, every compute entry
point raises -- there is no CPU fallback anywhere in this package.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhadi.so")

HADI_OK = 0
EU, AM, DIV, AM_DIV = 0, 1, 2, 3
MEM_HOST, MEM_DEVICE = 0, 1
SCHEME_DOUGLAS, SCHEME_CRAIG_SNEYD, SCHEME_MCS, SCHEME_HV = 0, 1, 2, 3
STATE_FP64, STATE_FP32 = 0, 1
CALL, PUT = 0, 1
# columns of hadi_compute_greeks' outputs (enum hadi_greek)
G_PRICE, G_DELTA, G_GAMMA, G_DV, G_DVV, G_DSV, G_THETA, G_LAMBDA = range(8)
N_GREEKS = 8
GREEK_NAMES = ("price", "delta", "gamma", "dv", "dvv", "dsv", "theta", "lambda")

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


class HadiError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("libhadi error %d: %s" % (status, message))
        self.status = status


class Problem(C.Structure):
    """struct hadi_problem (include/hadi.h)."""
    _fields_ = [
        ("n_instances", C.c_int), ("m1", C.c_int), ("m2", C.c_int), ("variant", C.c_int), ("memspace", C.c_int),
        ("N", C.c_int), ("delta_t", C.c_double), ("theta", C.c_double),
        ("N_i", _ip), ("delta_t_i", _dp),
        ("r_d", C.c_double), ("r_f", C.c_double),
        ("rho", C.c_double), ("sigma", C.c_double), ("kappa", C.c_double), ("eta", C.c_double),
        ("rho_i", _dp), ("sigma_i", _dp), ("kappa_i", _dp), ("eta_i", _dp),
        ("vec_s", _dp), ("vec_v", _dp), ("delta_s", _dp), ("delta_v", _dp),
        ("num_dividends", C.c_int),
        ("dividend_dates", _dp), ("dividend_amounts", _dp), ("dividend_percentages", _dp),
        ("U", _dp), ("U_0", _dp), ("lambda_bar", _dp),
        ("scheme", C.c_int),
        ("state_precision", C.c_int),
        ("option_type", C.c_int),
        ("strike_i", _dp),
        ("V_0_i", _dp),
    ]


FIX_SHARES, FIX_RETURN = 0, 1  # enum hadi_fixing_mode


class Barrier(C.Structure):
    """struct hadi_barrier (include/hadi.h)."""
    _fields_ = [("lower_i", _dp), ("upper_i", _dp), ("rebate_i", _dp), ("n_mon", C.c_int), ("mon_steps", _ip), ("mon_rows", C.c_int)]


class Cliquet(C.Structure):
    """struct hadi_cliquet (include/hadi.h)."""
    _fields_ = [("ref_spot_i", _dp), ("mode_i", _ip), ("n_fix", C.c_int), ("fix_steps", _ip), ("fix_rows", C.c_int), ("weights", _dp)]


class Jumps(C.Structure):
    """struct hadi_jumps (include/hadi.h)."""
    _fields_ = [("lam", C.c_double), ("mu", C.c_double), ("sigma", C.c_double), ("lambda_i", _dp), ("mu_i", _dp), ("sigma_i", _dp),
                ("shared_grid", C.c_int)]


class Samples(C.Structure):
    """struct hadi_samples (include/hadi.h)."""
    _fields_ = [("n_samp", C.c_int), ("spots", _dp), ("scales", _dp), ("rows", C.c_int)]


class Timing(C.Structure):
    """struct hadi_timing (include/hadi.h)."""
    _fields_ = [
        ("setup_ms", C.c_double), ("sweep_ms", C.c_double), ("finish_ms", C.c_double),
        ("pass_a_ms", C.c_double), ("pass_b_ms", C.c_double),
        ("pass_a_launches", C.c_longlong), ("pass_b_launches", C.c_longlong),
        ("point_steps", C.c_longlong),
    ]


# every symbol include/hadi.h declares (tests check the library exports all of them)
EXPORTS = [
    "hadi_create", "hadi_destroy", "hadi_last_error", "hadi_status_string", "hadi_version",
    "hadi_set_profiling", "hadi_get_timing", "hadi_set_tuning", "hadi_get_tuning", "hadi_device_info", "hadi_describe_last_sweep",
    "hadi_stream", "hadi_wait_stream",
    "hadi_make_grid", "hadi_rebuild_variance", "hadi_find_s_index", "hadi_find_v_index",
    "hadi_DO_timestepping", "hadi_parallel_DO_solve", "hadi_compute_greeks",
    "hadi_maturity_ladder", "hadi_compute_base_prices_ladder", "hadi_compute_jacobian_ladder",
    "hadi_sample_ladder", "hadi_compute_base_prices_samples", "hadi_compute_jacobian_samples",
    "hadi_bermudan_timestepping", "hadi_compute_base_prices_bermudan", "hadi_compute_jacobian_bermudan",
    "hadi_barrier_timestepping", "hadi_compute_base_prices_barrier", "hadi_compute_jacobian_barrier",
    "hadi_cliquet_timestepping", "hadi_compute_base_prices_cliquet", "hadi_compute_jacobian_cliquet",
    "hadi_bates_timestepping", "hadi_compute_base_prices_bates", "hadi_compute_jacobian_bates", "hadi_debug_jump_matrix",
    "hadi_bates_sample_ladder", "hadi_compute_base_prices_bates_samples", "hadi_compute_jacobian_bates_samples",
    "hadi_compute_jacobian_bates_jumps", "hadi_lm_partials_n", "hadi_lm_partials_device_n", "hadi_lm_solve_n",
    "hadi_compute_base_prices", "hadi_compute_base_prices_american",
    "hadi_compute_base_prices_dividends", "hadi_compute_base_prices_american_dividends",
    "hadi_compute_jacobian", "hadi_compute_jacobian_american",
    "hadi_compute_jacobian_dividends", "hadi_compute_jacobian_american_dividends",
    "hadi_lm_partials", "hadi_lm_partials_device", "hadi_lm_solve", "hadi_compute_parameter_update",
    "hadi_debug_row_pass", "hadi_debug_col_solve", "hadi_debug_rcp",
]

_lib = None
_others = {}


def lib(path=None):
    """Loads libhadi.so; raises if it has not been built (python __graft_entry__.py build).  `path`: another build of
    the same ABI (tests load the checking build libhadi_strict.so next to the product)."""
    global _lib
    if path is not None and os.path.abspath(path) != os.path.abspath(LIB_PATH):
        key = os.path.abspath(path)
        if key not in _others:
            _others[key] = _load(key)
        return _others[key]
    if _lib is not None:
        return _lib
    _lib = _load(LIB_PATH)
    return _lib


def _load(LIB_PATH):
    if not os.path.exists(LIB_PATH):
        raise HadiError(-1, "libhadi.so not built at %s -- run `python __graft_entry__.py` (hipcc, gfx950); "
                            "this package has no CPU fallback" % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 under the same soname as
    # /opt/rocm's.  Whichever is loaded first serves both; torch cannot see the GPU through the system
    # copy, so when torch is installed let it load first (libhadi runs fine on torch's copy).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.hadi_last_error.restype = C.c_char_p
    L.hadi_status_string.restype = C.c_char_p
    L.hadi_stream.restype = C.c_void_p
    L.hadi_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.hadi_destroy.argtypes = [C.c_void_p]
    L.hadi_last_error.argtypes = [C.c_void_p]
    L.hadi_set_profiling.argtypes = [C.c_void_p, C.c_int]
    L.hadi_get_timing.argtypes = [C.c_void_p, C.POINTER(Timing)]
    L.hadi_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.hadi_get_tuning.argtypes = [C.c_void_p, C.c_char_p, _ip]
    L.hadi_wait_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.hadi_lm_partials_device.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _dp]
    L.hadi_debug_row_pass.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_int, C.c_void_p]
    L.hadi_debug_col_solve.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_void_p]
    L.hadi_debug_rcp.argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    L.hadi_device_info.argtypes = [C.c_void_p, C.c_char_p, C.c_int, _ip, C.c_char_p, C.c_int]
    L.hadi_describe_last_sweep.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.hadi_stream.argtypes = [C.c_void_p]
    L.hadi_make_grid.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                 C.c_int, C.c_double, C.c_double, C.c_double, _dp, _dp, _dp, _dp]
    L.hadi_rebuild_variance.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, _dp, _dp]
    L.hadi_find_s_index.argtypes = [C.c_int, _dp, C.c_double]
    L.hadi_find_v_index.argtypes = [C.c_int, _dp, C.c_double]
    L.hadi_DO_timestepping.argtypes = [C.c_void_p, C.POINTER(Problem)]
    L.hadi_parallel_DO_solve.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, C.c_void_p]
    L.hadi_compute_greeks.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    if hasattr(L, "hadi_maturity_ladder"):  # (`path` may name a build from before the ladder: the A/B tools load one)
        for name in ("hadi_maturity_ladder", "hadi_compute_base_prices_ladder"):
            getattr(L, name).argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, C.c_int, _ip, C.c_void_p]
        L.hadi_compute_jacobian_ladder.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, C.c_double, C.c_int, _ip,
                                                   C.c_void_p, C.c_void_p]
    if hasattr(L, "hadi_bermudan_timestepping"):  # (likewise: a build from before the Bermudan entry points)
        L.hadi_bermudan_timestepping.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_int, _ip, C.c_int]
        L.hadi_compute_base_prices_bermudan.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, C.c_int, _ip, C.c_int,
                                                        C.c_void_p]
        L.hadi_compute_jacobian_bermudan.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, C.c_double, C.c_int, _ip,
                                                     C.c_int, C.c_void_p, C.c_void_p]
    if hasattr(L, "hadi_barrier_timestepping"):  # (likewise: a build from before the barrier entry points)
        _bp = C.POINTER(Barrier)
        L.hadi_barrier_timestepping.argtypes = [C.c_void_p, C.POINTER(Problem), _bp]
        L.hadi_compute_base_prices_barrier.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, _bp, C.c_void_p]
        L.hadi_compute_jacobian_barrier.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, C.c_double, _bp, C.c_void_p,
                                                    C.c_void_p]
    if hasattr(L, "hadi_cliquet_timestepping"):  # (likewise: a build from before the cliquet entry points)
        _cp = C.POINTER(Cliquet)
        L.hadi_cliquet_timestepping.argtypes = [C.c_void_p, C.POINTER(Problem), _cp]
        L.hadi_compute_base_prices_cliquet.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, _cp, C.c_void_p]
        L.hadi_compute_jacobian_cliquet.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, C.c_double, _cp, C.c_void_p,
                                                    C.c_void_p]
    if hasattr(L, "hadi_bates_timestepping"):  # (likewise: a build from before the Bates entry points)
        _jp = C.POINTER(Jumps)
        L.hadi_bates_timestepping.argtypes = [C.c_void_p, C.POINTER(Problem), _jp]
        L.hadi_compute_base_prices_bates.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, _jp, C.c_void_p]
        L.hadi_compute_jacobian_bates.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, C.c_double, _jp, C.c_void_p,
                                                  C.c_void_p]
        L.hadi_debug_jump_matrix.argtypes = [C.c_void_p, C.c_int, _dp, C.c_double, C.c_double, _dp]
    if hasattr(L, "hadi_compute_jacobian_bates_jumps"):  # (likewise: a build from before the eight-column Jacobian)
        L.hadi_compute_jacobian_bates_jumps.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, C.c_double,
                                                        C.POINTER(Jumps), C.c_void_p, C.c_void_p]
        L.hadi_lm_partials_n.argtypes = [C.c_int, C.c_int, _dp, _dp, _dp]
        L.hadi_lm_partials_device_n.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, _dp]
        L.hadi_lm_solve_n.argtypes = [C.c_int, _dp, C.c_double, _dp]
    if hasattr(L, "hadi_sample_ladder"):  # (likewise: a build from before the sampled ladder)
        _sp = C.POINTER(Samples)
        for name in ("hadi_sample_ladder", "hadi_compute_base_prices_samples"):
            getattr(L, name).argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, _sp, C.c_int, _ip, C.c_void_p]
        L.hadi_compute_jacobian_samples.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, _sp, C.c_int, _ip,
                                                    C.c_void_p, C.c_void_p]
    if hasattr(L, "hadi_bates_sample_ladder"):  # (likewise: a build from before the Bates surface calls)
        _sp, _jp = C.POINTER(Samples), C.POINTER(Jumps)
        for name in ("hadi_bates_sample_ladder", "hadi_compute_base_prices_bates_samples"):
            getattr(L, name).argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, _sp, C.c_int, _ip, _jp, C.c_void_p]
        L.hadi_compute_jacobian_bates_samples.argtypes = [C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, _sp, C.c_int, _ip,
                                                          _jp, C.c_int, C.c_void_p, C.c_void_p]
    for sfx in ("", "_american", "_dividends", "_american_dividends"):
        getattr(L, "hadi_compute_base_prices" + sfx).argtypes = [
            C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, C.c_void_p]
        getattr(L, "hadi_compute_jacobian" + sfx).argtypes = [
            C.c_void_p, C.POINTER(Problem), C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    L.hadi_lm_partials.argtypes = [C.c_int, _dp, _dp, _dp]
    L.hadi_lm_solve.argtypes = [_dp, C.c_double, _dp]
    L.hadi_compute_parameter_update.argtypes = [C.c_int, _dp, _dp, C.c_double, _dp]
    return L
