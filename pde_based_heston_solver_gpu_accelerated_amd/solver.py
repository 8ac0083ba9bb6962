"""Host-side mirror of the reference's batched launchers over libhadi's C ABI.

Names, argument order and meaning follow the reference (`parallel_DO_solve`,
src/device_solver.hpp:52-79; `compute_base_prices*` / `compute_jacobian*`,
src/jacobian_computation.hpp:43-231); the Kokkos struct arrays that only carry scratch
(A0/A1/A2 solvers, bounds_d) have no counterpart because the library owns its scratch.

Arrays may be numpy float64 (host memory, staged by the library) or torch CUDA tensors
(HBM-resident, passed as device pointers).  All arrays of one call must live in the same space.
"""
import ctypes as C

import numpy as np

from . import _native as nat
from ._native import EU, AM, DIV, AM_DIV, CALL, PUT, HadiError, FIX_SHARES, FIX_RETURN  # noqa: F401  (re-exported)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def _is_device(x):
    return hasattr(x, "data_ptr") and getattr(x, "is_cuda", False)


def _check_array(x, name, count):
    if _is_device(x):
        import torch
        if x.dtype != torch.float64 or not x.is_contiguous():
            raise ValueError("%s must be a contiguous float64 tensor" % name)
        if x.numel() != count:
            raise ValueError("%s has %d elements, expected %d" % (name, x.numel(), count))
        return C.cast(C.c_void_p(x.data_ptr()), _dp), True
    if not isinstance(x, np.ndarray) or x.dtype != np.float64 or not x.flags.c_contiguous:
        raise ValueError("%s must be a C-contiguous float64 numpy array or CUDA tensor" % name)
    if x.size != count:
        raise ValueError("%s has %d elements, expected %d" % (name, x.size, count))
    return x.ctypes.data_as(_dp), False


def _host_f64(x):
    return None if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float64))


class Dividends:
    """The three dividend views of the reference (device_solver.hpp:409-413)."""

    def __init__(self, dates, amounts, percentages):
        self.dates, self.amounts, self.percentages = _host_f64(dates), _host_f64(amounts), _host_f64(percentages)
        if not (len(self.dates) == len(self.amounts) == len(self.percentages)):
            raise ValueError("dividend arrays differ in length")

    def __len__(self):
        return len(self.dates)


class DOWorkspace:
    """DO_Workspace<Device> (src/DO_solver_workspace.hpp:4-44).  Only `U` carries data across the
    boundary (initial condition in, solution out); the reference's other eleven arrays are scratch
    and live inside the library handle here.  `lambda_bar` is filled by the American variants."""

    def __init__(self, nInstances, total_size, device=None):
        if device is None:
            self.U = np.zeros((nInstances, total_size))
            self.lambda_bar = np.zeros((nInstances, total_size))
        else:
            import torch
            self.U = torch.zeros((nInstances, total_size), dtype=torch.float64, device=device)
            self.lambda_bar = torch.zeros((nInstances, total_size), dtype=torch.float64, device=device)


class HestonADI:
    """One library handle = one GPU + one HIP stream (the reference's single Kokkos device)."""

    def __init__(self, device_id=0, lib_path=None):
        self._lib = nat.lib(lib_path)
        h = C.c_void_p()
        rc = self._lib.hadi_create(C.byref(h), int(device_id))
        if rc != nat.HADI_OK:
            raise HadiError(rc, self._lib.hadi_status_string(rc).decode())
        self._h = h
        self.device_id = int(device_id)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hadi_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- introspection ------------------------------------------------------------------------
    def _raise(self, rc):
        raise HadiError(rc, self._lib.hadi_last_error(self._h).decode() or self._lib.hadi_status_string(rc).decode())

    def set_profiling(self, enabled):
        self._lib.hadi_set_profiling(self._h, 1 if enabled else 0)

    def set_tuning(self, key, value):
        """Execution-path switch (hadi.h: 'small_grid', 'small_seq', 'small_sch', 'graph', 'american_p', 'strip', 'row_tile', 'col_groups',
        'small_waves', 'device_vgrid', 'jump_share', 'jump_small'); results agree to round-off."""
        self._call(self._lib.hadi_set_tuning, key.encode(), int(value))

    def get_tuning(self, key):
        v = C.c_int()
        rc = self._lib.hadi_get_tuning(self._h, key.encode(), C.byref(v))
        if rc != nat.HADI_OK:
            raise HadiError(rc, "unknown tuning key %r" % key)
        return v.value

    def wait_stream(self, stream=None):
        """Orders the handle's stream after everything enqueued so far on `stream` (a torch.cuda.Stream; None = torch's
        current stream on this handle's device).  Called by every launcher that receives CUDA tensors, so a tensor
        written by an earlier torch op (copy_, fill_ ...) is complete before the library reads it."""
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(torch.device("cuda", self.device_id))
        self._call(self._lib.hadi_wait_stream, C.c_void_p(stream.cuda_stream))

    def timing(self):
        t = nat.Timing()
        self._lib.hadi_get_timing(self._h, C.byref(t))
        return {k: getattr(t, k) for k, _ in nat.Timing._fields_}

    def device_info(self):
        name, arch, cu = C.create_string_buffer(256), C.create_string_buffer(64), C.c_int()
        self._lib.hadi_device_info(self._h, name, 256, C.byref(cu), arch, 64)
        return {"name": name.value.decode(), "arch": arch.value.decode(), "compute_units": cu.value}

    def describe_last_sweep(self):
        """Kernel names and tile geometry of the last sweep (for reports)."""
        buf = C.create_string_buffer(512)
        self._lib.hadi_describe_last_sweep(self._h, buf, 512)
        return buf.value.decode()

    # ---- problem assembly ---------------------------------------------------------------------
    def _problem(self, variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids,
                 U=None, U_0=None, lambda_bar=None, dividends=None, per_instance=None, need_vgrid=True, scheme=0,
                 state_precision=0, option_type=CALL, strikes=None):
        n = grids.Vec_s.shape[0]
        m = (m1 + 1) * (m2 + 1)
        p = nat.Problem()
        keep = []
        spaces = []

        def arr(x, name, count):
            ptr, dev = _check_array(x, name, count)
            spaces.append(dev)
            keep.append(x)
            return ptr

        p.n_instances, p.m1, p.m2, p.variant = n, m1, m2, variant
        p.scheme = int(scheme)
        p.state_precision = int(state_precision)
        p.N, p.delta_t, p.theta = int(N), float(delta_t), float(theta)
        p.r_d, p.r_f = float(r_d), float(r_f)
        p.rho, p.sigma, p.kappa, p.eta = float(rho), float(sigma), float(kappa), float(eta)
        p.vec_s = arr(grids.Vec_s, "Vec_s", n * (m1 + 1))
        p.delta_s = arr(grids.Delta_s, "Delta_s", n * m1)
        if need_vgrid:
            p.vec_v = arr(grids.Vec_v, "Vec_v", n * (m2 + 1))
            p.delta_v = arr(grids.Delta_v, "Delta_v", n * m2)
        if U is not None:
            p.U = arr(U, "U", n * m)
        if U_0 is not None:
            p.U_0 = arr(U_0, "U_0", n * m)
        if lambda_bar is not None:
            p.lambda_bar = arr(lambda_bar, "lambda_bar", n * m)
        if len(set(spaces)) > 1:
            raise ValueError("array arguments mix host and device memory")
        p.memspace = nat.MEM_DEVICE if spaces and spaces[0] else nat.MEM_HOST
        if p.memspace == nat.MEM_DEVICE:
            self.wait_stream()  # input ordering: the library's stream does not wait for torch's by itself (hadi.h)
        p.option_type = int(option_type)
        if strikes is not None:
            a = _host_f64(strikes).reshape(-1)
            if a.size != n:
                raise ValueError("strikes must have n_instances entries")
            keep.append(a)
            p.strike_i = a.ctypes.data_as(_dp)
        elif option_type == PUT:
            raise ValueError("option_type=PUT needs the strikes (boundary value K e^{-r_d t})")
        if dividends is not None and len(dividends):
            p.num_dividends = len(dividends)
            p.dividend_dates = dividends.dates.ctypes.data_as(_dp)
            p.dividend_amounts = dividends.amounts.ctypes.data_as(_dp)
            p.dividend_percentages = dividends.percentages.ctypes.data_as(_dp)
            keep.append(dividends)
        if per_instance:
            for key in ("rho_i", "sigma_i", "kappa_i", "eta_i", "delta_t_i", "V_0_i"):
                if per_instance.get(key) is not None:
                    a = _host_f64(per_instance[key])
                    if a.size != n:
                        raise ValueError("%s must have n_instances entries" % key)
                    keep.append(a)
                    setattr(p, key, a.ctypes.data_as(_dp))
            if per_instance.get("N_i") is not None:
                a = np.ascontiguousarray(np.asarray(per_instance["N_i"], dtype=np.int32))
                if a.size != n:
                    raise ValueError("N_i must have n_instances entries")
                keep.append(a)
                p.N_i = a.ctypes.data_as(_ip)
        p._keep = keep
        return p

    @staticmethod
    def _option(per_instance):
        """The launchers keep the reference's argument lists; the put extension travels in `per_instance`
        ({'option_type': PUT, 'strikes': [...]}) next to the other per-instance overrides."""
        if not per_instance:
            return CALL, None
        return per_instance.get("option_type", CALL), per_instance.get("strikes")

    def _base_problem(self, variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, num_strikes,
                      deviceGrids, workspace, U_0, dividends, per_instance, scheme):
        """The problem of a compute_base_prices* launcher: workspace.U is the state, the v-grid is rebuilt by the library."""
        option_type, strikes = self._option(per_instance)
        if total_size != (m1 + 1) * (m2 + 1):
            raise ValueError("total_size != (m1+1)*(m2+1)")
        if deviceGrids.Vec_s.shape[0] != num_strikes:
            raise ValueError("num_strikes does not match the grid batch")
        return self._problem(variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids, U=workspace.U,
                             U_0=U_0, dividends=dividends, per_instance=per_instance, need_vgrid=False, scheme=scheme,
                             option_type=option_type, strikes=strikes)

    def _jacobian_problem(self, variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, deviceGrids,
                          U_0, dividends, per_instance, scheme):
        """The problem of a compute_jacobian* launcher: every solve starts from U_0, the v-grids are rebuilt by the library."""
        if total_size != (m1 + 1) * (m2 + 1):
            raise ValueError("total_size != (m1+1)*(m2+1)")
        option_type, strikes = self._option(per_instance)
        return self._problem(variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids, U=None, U_0=U_0,
                             dividends=dividends, per_instance=per_instance, need_vgrid=False, scheme=scheme,
                             option_type=option_type, strikes=strikes)

    def _call(self, fn, *args):
        """One native call on this handle; a status other than HADI_OK raises HadiError with the library's message."""
        rc = fn(self._h, *args)
        if rc != nat.HADI_OK:
            self._raise(rc)

    def _out(self, n, cols, like):
        if _is_device(like):
            import torch
            shape = (n,) if cols == 1 else (n, cols)
            t = torch.empty(shape, dtype=torch.float64, device=like.device)
            return t, C.c_void_p(t.data_ptr())
        a = np.empty((n,) if cols == 1 else (n, cols))
        return a, C.c_void_p(a.ctypes.data)

    # ---- device_DO_timestepping* (src/device_solver.hpp:194-942) -------------------------------
    def DO_timestepping(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U,
                        variant=EU, U_0=None, lambda_bar=None, dividends=None, per_instance=None, scheme=0,
                        state_precision=0, option_type=CALL, strikes=None):
        """Boundary init + operator build + N Douglas steps on the caller's grids; U is updated in
        place (initial condition in, solution at T out).  scheme=1 runs Craig-Sneyd, scheme=2 Modified Craig-Sneyd (theta = 1/3
        is the usual choice), scheme=3 Hundsdorfer-Verwer (theta = 1/2 + sqrt(3)/6) -- European call, fp64 state only;
        state_precision=1 keeps the state between the two passes in fp32 (European Douglas only, arithmetic stays fp64)."""
        p = self._problem(variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids,
                          U=U, U_0=U_0, lambda_bar=lambda_bar, dividends=dividends, per_instance=per_instance,
                          scheme=scheme, state_precision=state_precision, option_type=option_type, strikes=strikes)
        self._call(self._lib.hadi_DO_timestepping, C.byref(p))
        return U

    # ---- diagnostics: the two directional passes of one Douglas step as operators (hadi.h) -------------------------
    def debug_row_pass(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, step=1, variant=EU,
                       U_0=None, option_type=CALL, strikes=None):
        """Right-hand side of the A2 solve after the row pass of time step `step` started from U (not modified)."""
        p = self._problem(variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U=U, U_0=U_0,
                          option_type=option_type, strikes=strikes)
        out, optr = self._out(grids.Vec_s.shape[0], (m1 + 1) * (m2 + 1), U)
        self._call(self._lib.hadi_debug_row_pass, C.byref(p), int(step), optr)
        return out

    def debug_col_solve(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, rhs):
        """(I - theta dt A2)^{-1} rhs through the product's column pass (rhs not modified)."""
        p = self._problem(EU, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U=rhs)
        out, optr = self._out(grids.Vec_s.shape[0], (m1 + 1) * (m2 + 1), rhs)
        self._call(self._lib.hadi_debug_col_solve, C.byref(p), optr)
        return out

    def debug_rcp(self, x):
        """1/x exactly as the line solves of the sweep form it (v_rcp_f64 + one Newton step), elementwise (tests)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        out = np.empty_like(x)
        self._call(self._lib.hadi_debug_rcp, int(x.size), x.ctypes.data_as(nat._dp), out.ctypes.data_as(nat._dp))
        return out

    # ---- CS_scheme_shuffled (src/solver.hpp:781-907), batched on the device -----------------------
    def CS_scheme(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, per_instance=None):
        """Craig-Sneyd time stepping of European options: Douglas predictor + corrector that re-adds half of
        the explicit mixed-derivative increment (the reference has it in its host operator family only)."""
        return self.DO_timestepping(m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U,
                                    per_instance=per_instance, scheme=nat.SCHEME_CRAIG_SNEYD)

    def MCS_scheme(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, per_instance=None):
        """Modified Craig-Sneyd time stepping of European options (in 't Hout & Foulon; second order for every theta, usually
        theta = 1/3): the Craig-Sneyd corrector with the whole explicit increment re-weighted by 1/2 - theta."""
        return self.DO_timestepping(m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U,
                                    per_instance=per_instance, scheme=nat.SCHEME_MCS)

    def HV_scheme(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, per_instance=None):
        """Hundsdorfer-Verwer time stepping of European options (in 't Hout & Foulon; second order for every theta, usually
        theta = 1/2 + sqrt(3)/6): a second Douglas-type sweep from the predictor's result."""
        return self.DO_timestepping(m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U,
                                    per_instance=per_instance, scheme=nat.SCHEME_HV)

    # ---- parallel_DO_solve (src/device_solver.hpp:52-185) --------------------------------------
    def parallel_DO_solve(self, nInstances, S_0, V_0, m1, m2, N, T, delta_t, theta, r_d, r_f, rho, sigma,
                          kappa, eta, deviceGrids, workspace, base_prices=None):
        """European sweep + price pick.  (The reference declares S_0, V_0 as `int` here,
        device_solver.hpp:56-57, which truncates V_0 = 0.04 to 0; they are doubles in this mirror.)"""
        if deviceGrids.Vec_s.shape[0] != nInstances:
            raise ValueError("nInstances does not match the grid batch")
        p = self._problem(EU, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, deviceGrids,
                          U=workspace.U)
        out, optr = self._out(nInstances, 1, workspace.U)
        self._call(self._lib.hadi_parallel_DO_solve, C.byref(p), float(S_0), float(V_0), optr)
        if base_prices is not None:
            base_prices[...] = out
            return base_prices
        return out

    # ---- Greeks and the spot ladder (hadi_compute_greeks; no reference counterpart) -----------------
    def compute_greeks(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, S_0, V_0,
                       variant=EU, U_0=None, dividends=None, per_instance=None, scheme=0, option_type=CALL, strikes=None,
                       ladder=False):
        """The sweep of DO_timestepping from the initial condition U (not modified), then price, delta, gamma, dv, dvv, dsv,
        theta and lambda_bar at (S_0, V_0) from the state on the device: [n][8], columns G_PRICE .. G_LAMBDA (hadi.h, enum
        hadi_greek).  ladder=True returns the pair ([n][8], [n][m1+1][8]): the same columns for every s-node of the v-row of
        V_0.  numpy arrays for host inputs, torch tensors for device inputs.  S_0 or V_0 off an instance's grid raises
        HadiError (status 4)."""
        p = self._problem(variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U=U, U_0=U_0,
                          dividends=dividends, per_instance=per_instance, scheme=scheme, option_type=option_type,
                          strikes=strikes)
        n = grids.Vec_s.shape[0]
        out, optr = self._out(n, nat.N_GREEKS, U)
        lad, lptr = None, None
        if ladder:
            lad, lptr = self._out(n * (m1 + 1), nat.N_GREEKS, U)
            lad = lad.reshape(n, m1 + 1, nat.N_GREEKS)
        self._call(self._lib.hadi_compute_greeks, C.byref(p), float(S_0), float(V_0), optr, lptr)
        return (out, lad) if ladder else out

    # ---- maturity ladder (hadi_maturity_ladder and its launchers; no reference counterpart) ---------------
    @staticmethod
    def _snap(snap_steps):
        a = np.ascontiguousarray(np.asarray(snap_steps, dtype=np.int32).reshape(-1))
        if a.size < 1:
            raise ValueError("snap_steps is empty")
        return a

    def maturity_ladder(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, S_0, V_0, snap_steps,
                        variant=EU, U_0=None, dividends=None, per_instance=None, scheme=0, option_type=CALL, strikes=None):
        """ONE sweep of N steps from the initial condition U (not modified) on the caller's grids; returns [n][len(snap_steps)]:
        the price node of (S_0, V_0) after each of the steps snap_steps (strictly increasing, within 1..N) -- entry q is, bit for
        bit, what the same call with N = snap_steps[q] returns.  The maturities share delta_t (per_instance['delta_t_i'] gives
        every instance its own) and, for the dividend variants, the one schedule on the sweep's clock.  per_instance must not
        carry N_i.  Call boundary data with r_f != 0 raise HadiError (status 2): their tables depend on N (hadi.h)."""
        p = self._problem(variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U=U, U_0=U_0,
                          dividends=dividends, per_instance=per_instance, scheme=scheme, option_type=option_type,
                          strikes=strikes)
        steps = self._snap(snap_steps)
        out, optr = self._out(grids.Vec_s.shape[0], steps.size, U)
        self._call(self._lib.hadi_maturity_ladder, C.byref(p), float(S_0), float(V_0), int(steps.size),
                   steps.ctypes.data_as(_ip), optr)
        return out.reshape(-1, steps.size)

    def compute_base_prices_ladder(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                   num_strikes, deviceGrids, workspace, snap_steps, variant=EU, U_0=None, dividends=None,
                                   per_instance=None, scheme=0):
        """compute_base_prices* (the v-grid rebuilt for V_0 or per_instance['V_0_i']) with the ladder's output: [n][len(snap_steps)],
        entry q what the single call with N = snap_steps[q] returns.  workspace.U is the initial condition and is not modified."""
        p = self._base_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, num_strikes,
                               deviceGrids, workspace, U_0, dividends, per_instance, scheme)
        steps = self._snap(snap_steps)
        out, optr = self._out(num_strikes, steps.size, workspace.U)
        self._call(self._lib.hadi_compute_base_prices_ladder, C.byref(p), float(S_0), float(V_0), int(steps.size),
                   steps.ctypes.data_as(_ip), optr)
        return out.reshape(-1, steps.size)

    def compute_jacobian_ladder(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                num_strikes, deviceGrids, U_0, snap_steps, eps=1e-6, variant=EU, dividends=None,
                                per_instance=None, scheme=0):
        """compute_jacobian* with the ladder's outputs: (J [n][len(snap_steps)][5], base_prices [n][len(snap_steps)]); J[:, q, :]
        and base_prices[:, q] are what compute_jacobian* with N = snap_steps[q] returns."""
        p = self._jacobian_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, deviceGrids,
                                   U_0, dividends, per_instance, scheme)
        steps = self._snap(snap_steps)
        J, jptr = self._out(num_strikes * steps.size, 5, U_0)
        base, bptr = self._out(num_strikes, steps.size, U_0)
        self._call(self._lib.hadi_compute_jacobian_ladder, C.byref(p), float(S_0), float(V_0), float(eps), int(steps.size),
                   steps.ctypes.data_as(_ip), jptr, bptr)
        return J.reshape(num_strikes, steps.size, 5), base.reshape(-1, steps.size)

    # ---- sampled ladder (hadi_sample_ladder and its launchers; no reference counterpart) ---------------------
    @staticmethod
    def _samples(n, spots, scales):
        """(struct hadi_samples, the arrays it points to, n_samp) of spots given as one list for the batch or one row per
        instance; scales None = 1, else the shape of spots."""
        sp = np.ascontiguousarray(np.asarray(spots, dtype=np.float64))
        if sp.ndim == 1:
            sp = sp.reshape(1, -1)
        if sp.ndim != 2 or sp.shape[1] < 1 or sp.shape[0] not in (1, n):
            raise ValueError("spots must be [n_samp] or [n][n_samp] with n_samp >= 1")
        sc = None
        if scales is not None:
            sc = np.ascontiguousarray(np.asarray(scales, dtype=np.float64))
            if sc.ndim == 1:
                sc = sc.reshape(1, -1)
            if sc.shape != sp.shape:
                raise ValueError("scales must have the shape of spots")
        st = nat.Samples(int(sp.shape[1]), sp.ctypes.data_as(nat._dp), sc.ctypes.data_as(nat._dp) if sc is not None else None,
                         int(sp.shape[0]))
        return st, (sp, sc), int(sp.shape[1])

    def sample_ladder(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, spots, V_0, snap_steps,
                      scales=None, variant=EU, U_0=None, dividends=None, per_instance=None, scheme=0, option_type=CALL,
                      strikes=None):
        """maturity_ladder with the state of the v-row of V_0 evaluated at arbitrary spots where the ladder copies the node of S_0:
        returns [n][len(snap_steps)][n_samp], entry (k, q, s) = scales[s] * U_k(spots[s], V_0) after step snap_steps[q].  spots /
        scales: one list for the batch or one row per instance (host arrays).  A spot within 1e-10 of an s-node returns the node's
        value bit for bit; otherwise a 4-point Lagrange interpolant on the instance's own s-grid, clamped at both ends (hadi.h
        states the arithmetic).  A spot off the s-grid raises HadiError (status 4).  Admitted and refused as maturity_ladder is."""
        p = self._problem(variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U=U, U_0=U_0,
                          dividends=dividends, per_instance=per_instance, scheme=scheme, option_type=option_type,
                          strikes=strikes)
        n = grids.Vec_s.shape[0]
        steps = self._snap(snap_steps)
        st, keep, n_samp = self._samples(n, spots, scales)
        out, optr = self._out(n, steps.size * n_samp, U)
        self._call(self._lib.hadi_sample_ladder, C.byref(p), float(V_0), C.byref(st), int(steps.size), steps.ctypes.data_as(_ip),
                   optr)
        return out.reshape(n, steps.size, n_samp)

    def compute_base_prices_samples(self, spots, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                    num_strikes, deviceGrids, workspace, snap_steps, scales=None, variant=EU, U_0=None,
                                    dividends=None, per_instance=None, scheme=0):
        """compute_base_prices_ladder (the v-grid rebuilt for V_0 or per_instance['V_0_i']) with sample_ladder's output:
        [n][len(snap_steps)][n_samp].  workspace.U is the initial condition and is not modified."""
        p = self._base_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, num_strikes,
                               deviceGrids, workspace, U_0, dividends, per_instance, scheme)
        steps = self._snap(snap_steps)
        st, keep, n_samp = self._samples(num_strikes, spots, scales)
        out, optr = self._out(num_strikes, steps.size * n_samp, workspace.U)
        self._call(self._lib.hadi_compute_base_prices_samples, C.byref(p), float(V_0), C.byref(st), int(steps.size),
                   steps.ctypes.data_as(_ip), optr)
        return out.reshape(num_strikes, steps.size, n_samp)

    def compute_jacobian_samples(self, spots, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                 num_strikes, deviceGrids, U_0, snap_steps, scales=None, eps=1e-6, variant=EU, dividends=None,
                                 per_instance=None, scheme=0):
        """compute_jacobian_ladder with sample_ladder's outputs: (J [n][len(snap_steps)][n_samp][5], base [n][len(snap_steps)][n_samp])
        from ONE sweep of the 6n solves; the v0 column samples the row of V_0 + eps of its own rebuilt v-grid."""
        p = self._jacobian_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, deviceGrids,
                                   U_0, dividends, per_instance, scheme)
        steps = self._snap(snap_steps)
        st, keep, n_samp = self._samples(num_strikes, spots, scales)
        J, jptr = self._out(num_strikes * steps.size * n_samp, 5, U_0)
        base, bptr = self._out(num_strikes, steps.size * n_samp, U_0)
        self._call(self._lib.hadi_compute_jacobian_samples, C.byref(p), float(V_0), float(eps), C.byref(st), int(steps.size),
                   steps.ctypes.data_as(_ip), jptr, bptr)
        return J.reshape(num_strikes, steps.size, n_samp, 5), base.reshape(num_strikes, steps.size, n_samp)

    # ---- Bermudan options (hadi_bermudan_timestepping and its launchers; no reference counterpart) --------------
    @staticmethod
    def _schedule(exercise_steps):
        """(int32 array [rows][n_ex], rows, n_ex) of a schedule given as a list of steps (one schedule for the batch) or a
        ragged list of lists (one per instance, padded with zeros here)."""
        ex = list(exercise_steps)
        if ex and all(np.ndim(r) == 1 for r in ex):
            width = max(len(r) for r in ex)
            a = np.zeros((len(ex), width), dtype=np.int32)
            for k, r in enumerate(ex):
                a[k, :len(r)] = np.asarray(r, dtype=np.int32)
        else:
            a = np.asarray(ex, dtype=np.int32).reshape(1, -1)
        a = np.ascontiguousarray(a)
        return a, int(a.shape[0]), int(a.shape[1])

    def bermudan_timestepping(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, exercise_steps,
                              variant=EU, U_0=None, dividends=None, per_instance=None, scheme=0, option_type=CALL, strikes=None):
        """DO_timestepping (variant EU or DIV) with exercise: after the last pass of every step of `exercise_steps` every node
        of the instances that list it takes U <- max(U, payoff); the payoff is U_0, or the initial U where U_0 is None.
        exercise_steps: a list of step indices (one schedule for the batch; step n is time to maturity n delta_t, n = N the
        valuation date) or a list of lists, one per instance.  An empty schedule is the plain European call.  U is updated
        in place."""
        p = self._problem(variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U=U, U_0=U_0,
                          dividends=dividends, per_instance=per_instance, scheme=scheme, option_type=option_type, strikes=strikes)
        ex, rows, n_ex = self._schedule(exercise_steps)
        self._call(self._lib.hadi_bermudan_timestepping, C.byref(p), n_ex, ex.ctypes.data_as(_ip), rows)
        return U

    def compute_base_prices_bermudan(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                     num_strikes, deviceGrids, workspace, exercise_steps, variant=EU, U_0=None, dividends=None,
                                     per_instance=None, scheme=0):
        """compute_base_prices* (the v-grid rebuilt for V_0 or per_instance['V_0_i']) of Bermudan options: [n] prices at
        (S_0, V_0).  workspace.U is the initial condition (and the payoff where U_0 is None) and receives the field."""
        p = self._base_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, num_strikes,
                               deviceGrids, workspace, U_0, dividends, per_instance, scheme)
        ex, rows, n_ex = self._schedule(exercise_steps)
        out, optr = self._out(num_strikes, 1, workspace.U)
        self._call(self._lib.hadi_compute_base_prices_bermudan, C.byref(p), float(S_0), float(V_0), n_ex,
                   ex.ctypes.data_as(_ip), rows, optr)
        return out

    def compute_jacobian_bermudan(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                  num_strikes, deviceGrids, U_0, exercise_steps, eps=1e-6, variant=EU, dividends=None,
                                  per_instance=None, scheme=0):
        """compute_jacobian* of Bermudan options: (J [n][5], base_prices [n]); the six solves of an instance share its
        schedule, U_0 is the initial condition and the payoff."""
        p = self._jacobian_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, deviceGrids,
                                   U_0, dividends, per_instance, scheme)
        ex, rows, n_ex = self._schedule(exercise_steps)
        J, jptr = self._out(num_strikes, 5, U_0)
        base, bptr = self._out(num_strikes, 1, U_0)
        self._call(self._lib.hadi_compute_jacobian_bermudan, C.byref(p), float(S_0), float(V_0), float(eps), n_ex,
                   ex.ctypes.data_as(_ip), rows, jptr, bptr)
        return J, base

    # ---- knock-out barrier options (hadi_barrier_timestepping and its launchers; no reference counterpart) ------
    @classmethod
    def _barrier(cls, n, monitor_steps, lower, upper, rebate):
        """(struct hadi_barrier, the arrays it points into) -- host arrays [n] from scalars or sequences, None = NULL."""
        keep = []

        def arr(x):
            if x is None:
                return None
            a = np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (n,)))
            keep.append(a)
            return a.ctypes.data_as(nat._dp)

        mon, rows, n_mon = cls._schedule(monitor_steps)
        keep.append(mon)
        b = nat.Barrier(arr(lower), arr(upper), arr(rebate), n_mon, mon.ctypes.data_as(_ip), rows)
        return b, keep

    def barrier_timestepping(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, monitor_steps,
                             lower=None, upper=None, rebate=None, variant=EU, dividends=None, per_instance=None, scheme=0,
                             option_type=CALL, strikes=None):
        """DO_timestepping (variant EU or DIV) of discretely monitored knock-out options: after the last pass of every step of
        `monitor_steps` every node of the instances that list it whose spot is at or beyond a barrier (s <= lower or
        s >= upper) takes U <- rebate, undiscounted.  monitor_steps: as exercise_steps of bermudan_timestepping (one list, or
        one list per instance; monitoring_steps maps calendar dates to steps).  lower / upper / rebate: a scalar, one value per
        instance, or None (no barrier on that side / no rebate).  U is the caller's initial condition -- monitoring at maturity
        is knock_out_payoff -- and is updated in place."""
        p = self._problem(variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U=U, dividends=dividends,
                          per_instance=per_instance, scheme=scheme, option_type=option_type, strikes=strikes)
        b, keep = self._barrier(p.n_instances, monitor_steps, lower, upper, rebate)
        self._call(self._lib.hadi_barrier_timestepping, C.byref(p), C.byref(b))
        del keep
        return U

    def compute_base_prices_barrier(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                    num_strikes, deviceGrids, workspace, monitor_steps, lower=None, upper=None, rebate=None,
                                    variant=EU, dividends=None, per_instance=None, scheme=0):
        """compute_base_prices* (the v-grid rebuilt for V_0 or per_instance['V_0_i']) of knock-out options: [n] prices at
        (S_0, V_0).  workspace.U is the initial condition and receives the field."""
        p = self._base_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, num_strikes,
                               deviceGrids, workspace, None, dividends, per_instance, scheme)
        b, keep = self._barrier(num_strikes, monitor_steps, lower, upper, rebate)
        out, optr = self._out(num_strikes, 1, workspace.U)
        self._call(self._lib.hadi_compute_base_prices_barrier, C.byref(p), float(S_0), float(V_0), C.byref(b), optr)
        del keep
        return out

    def compute_jacobian_barrier(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                 num_strikes, deviceGrids, U_0, monitor_steps, lower=None, upper=None, rebate=None, eps=1e-6,
                                 variant=EU, dividends=None, per_instance=None, scheme=0):
        """compute_jacobian* of knock-out options: (J [n][5], base_prices [n]); the six solves of an instance share its
        barriers, rebate and schedule; U_0 is the initial condition."""
        p = self._jacobian_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, deviceGrids,
                                   U_0, dividends, per_instance, scheme)
        b, keep = self._barrier(num_strikes, monitor_steps, lower, upper, rebate)
        J, jptr = self._out(num_strikes, 5, U_0)
        base, bptr = self._out(num_strikes, 1, U_0)
        self._call(self._lib.hadi_compute_jacobian_barrier, C.byref(p), float(S_0), float(V_0), float(eps), C.byref(b), jptr, bptr)
        del keep
        return J, base

    # ---- forward-start options and cliquets (hadi_cliquet_timestepping and its launchers; no reference counterpart) ------
    @classmethod
    def _cliquet(cls, n, fixing_steps, ref_spot, mode, weights):
        """(struct hadi_cliquet, the arrays it points into) -- host arrays [n] from scalars or sequences; the weights padded with
        zeros as _schedule pads the steps."""
        fix, rows, n_fix = cls._schedule(fixing_steps)
        ref = np.ascontiguousarray(np.broadcast_to(np.asarray(ref_spot, dtype=np.float64), (n,)))
        md = np.ascontiguousarray(np.broadcast_to(np.asarray(mode, dtype=np.int32), (n,)))
        wt, wptr = None, None
        if weights is not None:
            wl = [float(weights)] * n_fix if np.isscalar(weights) else list(weights)
            wt = np.zeros((rows, n_fix), dtype=np.float64)
            if wl and all(np.ndim(r) == 1 for r in wl):
                if len(wl) != rows:
                    raise ValueError("weights: one list per schedule row")
                for k, r in enumerate(wl):
                    wt[k, :len(r)] = np.asarray(r, dtype=np.float64)
            else:
                if rows != 1 and len(wl) != n_fix:
                    raise ValueError("weights: one list for the batch needs one schedule for the batch")
                wt[:, :len(wl)] = np.asarray(wl, dtype=np.float64)
            wptr = wt.ctypes.data_as(nat._dp)
        q = nat.Cliquet(ref.ctypes.data_as(nat._dp), md.ctypes.data_as(_ip), n_fix, fix.ctypes.data_as(_ip), rows, wptr)
        return q, [fix, ref, md, wt]

    def cliquet_timestepping(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, fixing_steps, ref_spot,
                             mode=FIX_SHARES, weights=None, variant=EU, U_0=None, dividends=None, per_instance=None, scheme=0,
                             option_type=CALL, strikes=None):
        """DO_timestepping (variant EU or DIV) of forward-start options and cliquets: after the last pass of every step of
        `fixing_steps` every v-row j of the instances that list it takes U(i, j) <- a_i U(i_ref, j) + w P(i, j), with i_ref the
        node of `ref_spot`, a_i = s_i / s_ref (FIX_SHARES) or 1 (FIX_RETURN), w the weight of that fixing (weights: parallel to
        fixing_steps, None = 0) and P the payoff U_0, or the initial U where U_0 is None.  fixing_steps: as exercise_steps of
        bermudan_timestepping (one list, or one list per instance; fixing_steps maps calendar dates to steps).  ref_spot / mode:
        a scalar or one value per instance.  U is updated in place."""
        p = self._problem(variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U=U, U_0=U_0,
                          dividends=dividends, per_instance=per_instance, scheme=scheme, option_type=option_type, strikes=strikes)
        q, keep = self._cliquet(p.n_instances, fixing_steps, ref_spot, mode, weights)
        self._call(self._lib.hadi_cliquet_timestepping, C.byref(p), C.byref(q))
        del keep
        return U

    def compute_base_prices_cliquet(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                    num_strikes, deviceGrids, workspace, fixing_steps, ref_spot, mode=FIX_SHARES, weights=None,
                                    variant=EU, U_0=None, dividends=None, per_instance=None, scheme=0):
        """compute_base_prices* (the v-grid rebuilt for V_0 or per_instance['V_0_i']) of forward-start options and cliquets: [n]
        prices at (S_0, V_0).  workspace.U is the initial condition (and the payoff where U_0 is None) and receives the field."""
        p = self._base_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, num_strikes,
                               deviceGrids, workspace, U_0, dividends, per_instance, scheme)
        q, keep = self._cliquet(num_strikes, fixing_steps, ref_spot, mode, weights)
        out, optr = self._out(num_strikes, 1, workspace.U)
        self._call(self._lib.hadi_compute_base_prices_cliquet, C.byref(p), float(S_0), float(V_0), C.byref(q), optr)
        del keep
        return out

    def compute_jacobian_cliquet(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                 num_strikes, deviceGrids, U_0, fixing_steps, ref_spot, mode=FIX_SHARES, weights=None, eps=1e-6,
                                 variant=EU, dividends=None, per_instance=None, scheme=0):
        """compute_jacobian* of forward-start options and cliquets: (J [n][5], base_prices [n]); the six solves of an instance
        share its reference spot, mode, schedule and weights; U_0 is the initial condition and the payoff."""
        p = self._jacobian_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, deviceGrids,
                                   U_0, dividends, per_instance, scheme)
        q, keep = self._cliquet(num_strikes, fixing_steps, ref_spot, mode, weights)
        J, jptr = self._out(num_strikes, 5, U_0)
        base, bptr = self._out(num_strikes, 1, U_0)
        self._call(self._lib.hadi_compute_jacobian_cliquet, C.byref(p), float(S_0), float(V_0), float(eps), C.byref(q), jptr, bptr)
        del keep
        return J, base

    # ---- the Bates model: lognormal jumps (hadi_bates_timestepping and its launchers; no reference counterpart) ------
    @staticmethod
    def _jumps(n, jump_intensity, jump_mean, jump_vol, shared_grid):
        """(struct hadi_jumps, the arrays it points into) -- a scalar fills the shared field, a sequence becomes a host array [n]."""
        keep = []

        def field(x, name):
            if np.ndim(x) == 0:
                return float(x), None
            a = np.ascontiguousarray(x, dtype=np.float64)
            if a.shape != (n,):
                raise ValueError("%s: a scalar or one value per instance" % name)
            keep.append(a)
            return 0.0, a.ctypes.data_as(nat._dp)

        (lam, lam_i), (mu, mu_i), (sg, sg_i) = (field(jump_intensity, "jump_intensity"), field(jump_mean, "jump_mean"),
                                                field(jump_vol, "jump_vol"))
        return nat.Jumps(lam, mu, sg, lam_i, mu_i, sg_i, int(bool(shared_grid))), keep

    def bates_timestepping(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, jump_intensity, jump_mean,
                           jump_vol, shared_grid=False, variant=EU, dividends=None, per_instance=None, scheme=0, option_type=CALL,
                           strikes=None):
        """DO_timestepping (variant EU or DIV) under the Bates model: Heston plus compound-Poisson jumps in the spot of intensity
        `jump_intensity` with ln Y ~ N(jump_mean, jump_vol^2).  After the last pass of EVERY step each v-row takes
        U <- U + lambda dt (G U), G the generator of the jump term on the instance's own s-grid (include/hadi.h).  The three jump
        arguments: a scalar or one value per instance.  shared_grid: the caller's promise that every instance has instance 0's
        s-grid -- with a shared (jump_mean, jump_vol) one matrix then serves the whole batch; the promise is checked.  First order
        in time; European and dividend sweeps on the streaming path only.  U is updated in place."""
        p = self._problem(variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U=U, dividends=dividends,
                          per_instance=per_instance, scheme=scheme, option_type=option_type, strikes=strikes)
        j, keep = self._jumps(p.n_instances, jump_intensity, jump_mean, jump_vol, shared_grid)
        self._call(self._lib.hadi_bates_timestepping, C.byref(p), C.byref(j))
        del keep
        return U

    def compute_base_prices_bates(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                  num_strikes, deviceGrids, workspace, jump_intensity, jump_mean, jump_vol, shared_grid=False,
                                  variant=EU, dividends=None, per_instance=None, scheme=0):
        """compute_base_prices* (the v-grid rebuilt for V_0 or per_instance['V_0_i']) under the Bates model: [n] prices at
        (S_0, V_0).  workspace.U is the initial condition and receives the field."""
        p = self._base_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, num_strikes,
                               deviceGrids, workspace, None, dividends, per_instance, scheme)
        j, keep = self._jumps(num_strikes, jump_intensity, jump_mean, jump_vol, shared_grid)
        out, optr = self._out(num_strikes, 1, workspace.U)
        self._call(self._lib.hadi_compute_base_prices_bates, C.byref(p), float(S_0), float(V_0), C.byref(j), optr)
        del keep
        return out

    def compute_jacobian_bates(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                               num_strikes, deviceGrids, U_0, jump_intensity, jump_mean, jump_vol, shared_grid=False, eps=1e-6,
                               variant=EU, dividends=None, per_instance=None, scheme=0):
        """compute_jacobian* under the Bates model: (J [n][5], base_prices [n]), columns kappa, eta, sigma, rho, V_0 -- the jump
        parameters are inputs, held fixed; the six solves of an instance share its matrix.  U_0 is the initial condition."""
        p = self._jacobian_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, deviceGrids,
                                   U_0, dividends, per_instance, scheme)
        j, keep = self._jumps(num_strikes, jump_intensity, jump_mean, jump_vol, shared_grid)
        J, jptr = self._out(num_strikes, 5, U_0)
        base, bptr = self._out(num_strikes, 1, U_0)
        self._call(self._lib.hadi_compute_jacobian_bates, C.byref(p), float(S_0), float(V_0), float(eps), C.byref(j), jptr, bptr)
        del keep
        return J, base

    def compute_jacobian_bates_jumps(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                     num_strikes, deviceGrids, U_0, jump_intensity, jump_mean, jump_vol, shared_grid=False, eps=1e-6,
                                     variant=EU, dividends=None, per_instance=None, scheme=0):
        """compute_jacobian_bates with the jump law among the columns: (J [n][8], base_prices [n]), columns kappa, eta, sigma, rho,
        V_0, jump_intensity, jump_mean, jump_vol, forward differences with the one step eps -- nine groups of one batched sweep
        over three sets of matrices (include/hadi.h).  (jump_intensity + eps) delta_t must not exceed 1."""
        p = self._jacobian_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, deviceGrids,
                                   U_0, dividends, per_instance, scheme)
        j, keep = self._jumps(num_strikes, jump_intensity, jump_mean, jump_vol, shared_grid)
        J, jptr = self._out(num_strikes, 8, U_0)
        base, bptr = self._out(num_strikes, 1, U_0)
        self._call(self._lib.hadi_compute_jacobian_bates_jumps, C.byref(p), float(S_0), float(V_0), float(eps), C.byref(j), jptr, bptr)
        del keep
        return J, base

    # ---- a Bates surface from one sweep: the sample calls with the jump sub-step (hadi_bates_sample_ladder and its launchers) ------
    def bates_sample_ladder(self, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U, spots, V_0, snap_steps,
                            jump_intensity, jump_mean, jump_vol, shared_grid=False, scales=None, variant=EU, U_0=None,
                            dividends=None, per_instance=None, scheme=0, option_type=CALL, strikes=None):
        """sample_ladder under the Bates model: the jump sub-step of bates_timestepping at the end of every step, behind the step's
        last column pass and in front of the snapshot.  Returns [n][len(snap_steps)][n_samp]; snapshot q is what the call with
        N = snap_steps[q] returns.  Jumps are multiplicative, so the problem stays homogeneous in (s, K): strike_samples turns one
        sweep into every strike (only proportional dividends keep that).  Admitted and refused as sample_ladder and
        bates_timestepping both are.  Zero intensities: sample_ladder, bit for bit."""
        p = self._problem(variant, m1, m2, N, delta_t, theta, r_d, r_f, rho, sigma, kappa, eta, grids, U=U, U_0=U_0,
                          dividends=dividends, per_instance=per_instance, scheme=scheme, option_type=option_type,
                          strikes=strikes)
        n = grids.Vec_s.shape[0]
        steps = self._snap(snap_steps)
        st, keep, n_samp = self._samples(n, spots, scales)
        j, keepj = self._jumps(n, jump_intensity, jump_mean, jump_vol, shared_grid)
        out, optr = self._out(n, steps.size * n_samp, U)
        self._call(self._lib.hadi_bates_sample_ladder, C.byref(p), float(V_0), C.byref(st), int(steps.size),
                   steps.ctypes.data_as(_ip), C.byref(j), optr)
        del keep, keepj
        return out.reshape(n, steps.size, n_samp)

    def compute_base_prices_bates_samples(self, spots, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                          num_strikes, deviceGrids, workspace, snap_steps, jump_intensity, jump_mean, jump_vol,
                                          shared_grid=False, scales=None, variant=EU, U_0=None, dividends=None, per_instance=None,
                                          scheme=0):
        """compute_base_prices_samples under the Bates model (the v-grid rebuilt for V_0 or per_instance['V_0_i']):
        [n][len(snap_steps)][n_samp].  workspace.U is the initial condition and is not modified."""
        p = self._base_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, num_strikes,
                               deviceGrids, workspace, U_0, dividends, per_instance, scheme)
        steps = self._snap(snap_steps)
        st, keep, n_samp = self._samples(num_strikes, spots, scales)
        j, keepj = self._jumps(num_strikes, jump_intensity, jump_mean, jump_vol, shared_grid)
        out, optr = self._out(num_strikes, steps.size * n_samp, workspace.U)
        self._call(self._lib.hadi_compute_base_prices_bates_samples, C.byref(p), float(V_0), C.byref(st), int(steps.size),
                   steps.ctypes.data_as(_ip), C.byref(j), optr)
        del keep, keepj
        return out.reshape(num_strikes, steps.size, n_samp)

    def compute_jacobian_bates_samples(self, spots, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t,
                                       num_strikes, deviceGrids, U_0, snap_steps, jump_intensity, jump_mean, jump_vol,
                                       shared_grid=False, jump_columns=False, scales=None, eps=1e-6, variant=EU, dividends=None,
                                       per_instance=None, scheme=0):
        """compute_jacobian_samples under the Bates model: (J [n][len(snap_steps)][n_samp][n_par], base [n][len(snap_steps)][n_samp])
        from ONE sweep.  jump_columns False: n_par = 5, the six groups of compute_jacobian_bates (the jump law held fixed); True:
        n_par = 8, the nine groups and three matrix sets of compute_jacobian_bates_jumps (columns kappa, eta, sigma, rho, V_0,
        jump_intensity, jump_mean, jump_vol; (jump_intensity + eps) delta_t must not exceed 1)."""
        p = self._jacobian_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, deviceGrids,
                                   U_0, dividends, per_instance, scheme)
        steps = self._snap(snap_steps)
        st, keep, n_samp = self._samples(num_strikes, spots, scales)
        j, keepj = self._jumps(num_strikes, jump_intensity, jump_mean, jump_vol, shared_grid)
        n_par = 8 if jump_columns else 5
        J, jptr = self._out(num_strikes * steps.size * n_samp, n_par, U_0)
        base, bptr = self._out(num_strikes, steps.size * n_samp, U_0)
        self._call(self._lib.hadi_compute_jacobian_bates_samples, C.byref(p), float(V_0), float(eps), C.byref(st), int(steps.size),
                   steps.ctypes.data_as(_ip), C.byref(j), n_par, jptr, bptr)
        del keep, keepj
        return J.reshape(num_strikes, steps.size, n_samp, n_par), base.reshape(num_strikes, steps.size, n_samp)

    def debug_jump_matrix(self, vec_s, jump_mean, jump_vol):
        """The generator G [m1+1][m1+1] of the jump term on the grid vec_s, natural order, as the sweep's kernel builds it."""
        vs = np.ascontiguousarray(vec_s, dtype=np.float64)
        G = np.empty((vs.size, vs.size))
        self._call(self._lib.hadi_debug_jump_matrix, vs.size - 1, vs.ctypes.data_as(nat._dp), float(jump_mean), float(jump_vol),
                   G.ctypes.data_as(nat._dp))
        return G

    # ---- compute_base_prices* (src/jacobian_computation.cpp:368, 629, 922, 1232) ---------------
    def _base_prices(self, variant, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N,
                     theta, delta_t, num_strikes, deviceGrids, workspace, U_0=None, dividends=None,
                     per_instance=None, scheme=0):
        p = self._base_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, num_strikes,
                               deviceGrids, workspace, U_0, dividends, per_instance, scheme)
        out, optr = self._out(num_strikes, 1, workspace.U)
        self._call(self._lib.hadi_compute_base_prices, C.byref(p), float(S_0), float(V_0), optr)
        return out

    def compute_base_prices(self, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta,
                            delta_t, num_strikes, deviceGrids, workspace, per_instance=None, scheme=0):
        """scheme: the time stepper of every solve (0 Douglas, 1 Craig-Sneyd, 2 Modified Craig-Sneyd, 3 Hundsdorfer-Verwer; see
        DO_timestepping).  The European launchers take it; the library refuses the schemes for the other variants."""
        return self._base_prices(EU, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta,
                                 delta_t, num_strikes, deviceGrids, workspace, per_instance=per_instance, scheme=scheme)

    def compute_base_prices_american(self, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N,
                                     theta, delta_t, num_strikes, deviceGrids, U_0, workspace, per_instance=None):
        return self._base_prices(AM, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta,
                                 delta_t, num_strikes, deviceGrids, workspace, U_0=U_0, per_instance=per_instance)

    def compute_base_prices_dividends(self, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N,
                                      theta, delta_t, num_strikes, deviceGrids, workspace, dividends,
                                      per_instance=None):
        return self._base_prices(DIV, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta,
                                 delta_t, num_strikes, deviceGrids, workspace, dividends=dividends,
                                 per_instance=per_instance)

    def compute_base_prices_american_dividends(self, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2,
                                               total_size, N, theta, delta_t, num_strikes, deviceGrids, U_0,
                                               workspace, dividends, per_instance=None):
        return self._base_prices(AM_DIV, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N,
                                 theta, delta_t, num_strikes, deviceGrids, workspace, U_0=U_0, dividends=dividends,
                                 per_instance=per_instance)

    # ---- compute_jacobian* (src/jacobian_computation.cpp:204, 457, 726, 1031) ------------------
    def _jacobian(self, variant, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta,
                  delta_t, num_strikes, deviceGrids, U_0, eps, dividends=None, per_instance=None, scheme=0):
        p = self._jacobian_problem(variant, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, delta_t, deviceGrids,
                                   U_0, dividends, per_instance, scheme)
        J, jptr = self._out(num_strikes, 5, U_0)
        base, bptr = self._out(num_strikes, 1, U_0)
        self._call(self._lib.hadi_compute_jacobian, C.byref(p), float(S_0), float(V_0), float(eps), jptr, bptr)
        return J, base

    def compute_jacobian(self, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta,
                         delta_t, num_strikes, deviceGrids, U_0, eps=1e-6, per_instance=None, scheme=0):
        """Returns (J [n][5] with columns kappa, eta, sigma, rho, v0; base_prices [n]).  scheme: as compute_base_prices."""
        return self._jacobian(EU, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta,
                              delta_t, num_strikes, deviceGrids, U_0, eps, per_instance=per_instance, scheme=scheme)

    def compute_jacobian_american(self, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N,
                                  theta, delta_t, num_strikes, deviceGrids, U_0, eps=1e-6, per_instance=None):
        return self._jacobian(AM, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta,
                              delta_t, num_strikes, deviceGrids, U_0, eps, per_instance=per_instance)

    def compute_jacobian_dividends(self, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N,
                                   theta, delta_t, num_strikes, deviceGrids, U_0, dividends, eps=1e-6,
                                   per_instance=None):
        return self._jacobian(DIV, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta,
                              delta_t, num_strikes, deviceGrids, U_0, eps, dividends=dividends,
                              per_instance=per_instance)

    def compute_jacobian_american_dividends(self, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2,
                                            total_size, N, theta, delta_t, num_strikes, deviceGrids, U_0,
                                            dividends, eps=1e-6, per_instance=None):
        return self._jacobian(AM_DIV, S_0, V_0, T, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta,
                              delta_t, num_strikes, deviceGrids, U_0, eps, dividends=dividends,
                              per_instance=per_instance)

    # ---- multi-maturity launchers (src/heston_calibration.cpp:2174-2424, 2936-3243) ----------------------
    # One instance per CalibrationPoint{strike, maturity, time_steps, delta_t, global_index}: the batch shares the
    # grid shape and the model parameters, every instance steps its own (N, delta_t).
    @staticmethod
    def _steps(calibration_points, total_calibration_size):
        if len(calibration_points) != total_calibration_size:
            raise ValueError("total_calibration_size does not match the calibration points")
        N_i = np.array([pt.time_steps for pt in calibration_points], dtype=np.int32)
        dt_i = np.array([pt.delta_t for pt in calibration_points], dtype=np.float64)
        return {"N_i": N_i, "delta_t_i": dt_i}, int(N_i.max()) if len(N_i) else 1, float(dt_i[0]) if len(dt_i) else 1.0

    def compute_jacobian_multi_maturity(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, theta,
                                        calibration_points, total_calibration_size, deviceGrids, U_0, eps=1e-6, scheme=0):
        per, N, dt = self._steps(calibration_points, total_calibration_size)
        return self._jacobian(EU, S_0, V_0, None, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta, dt,
                              total_calibration_size, deviceGrids, U_0, eps, per_instance=per, scheme=scheme)

    def compute_base_prices_multi_maturity(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, theta,
                                           calibration_points, total_calibration_size, deviceGrids, workspace, scheme=0):
        per, N, dt = self._steps(calibration_points, total_calibration_size)
        return self._base_prices(EU, S_0, V_0, None, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta,
                                 dt, total_calibration_size, deviceGrids, workspace, per_instance=per, scheme=scheme)

    def compute_jacobian_multi_maturity_american_dividends(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2,
                                                           total_size, theta, calibration_points,
                                                           total_calibration_size, deviceGrids, U_0, dividends,
                                                           eps=1e-6):
        per, N, dt = self._steps(calibration_points, total_calibration_size)
        return self._jacobian(AM_DIV, S_0, V_0, None, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N, theta,
                              dt, total_calibration_size, deviceGrids, U_0, eps, dividends=dividends, per_instance=per)

    def compute_base_prices_multi_maturity_american_dividends(self, S_0, V_0, r_d, r_f, rho, sigma, kappa, eta, m1, m2,
                                                              total_size, theta, calibration_points,
                                                              total_calibration_size, deviceGrids, U_0, workspace,
                                                              dividends):
        per, N, dt = self._steps(calibration_points, total_calibration_size)
        return self._base_prices(AM_DIV, S_0, V_0, None, r_d, r_f, rho, sigma, kappa, eta, m1, m2, total_size, N,
                                 theta, dt, total_calibration_size, deviceGrids, workspace, U_0=U_0,
                                 dividends=dividends, per_instance=per)


def strike_samples(S_0, base_strike, strikes):
    """(spots, scales) that price the strikes K' at spot S_0 from ONE sweep on grids built at `base_strike` K:
    spots = S_0 K / K', scales = K' / K, so that scale * U_K(spot) = price of strike K' at S_0.

    The Heston operators and both boundary classes are homogeneous of degree one in (s, K): solving on the grid scaled by
    a = K'/K (s-nodes a s_i, payoff of strike K') gives a U_K, node by node, to round-off (measured on the oracle: at most 6e-15,
    1.4e-14 and 5.4e-14 of max|U| on 50x25x20, 100x50x40 and 200x100x40).  So the price of strike K' at S_0 is a U_K(S_0 / a); S_0 / a
    is in general no node, which is what sample_ladder's interpolants are for.  Limits: it holds for calls and puts (the put's
    strike in per_instance must be base_strike) and for proportional dividends; a cash dividend AMOUNT breaks it (the jump
    s -> s - D is not homogeneous).  The grids and the payoff must be built at base_strike, and the claim is stated for European
    exercise.  The surface is the one of the scaled grids, not of the grids GridViewsBatch.for_strikes builds per strike: the two
    differ by less than either grid's own discretisation error."""
    K = np.asarray(strikes, dtype=np.float64).reshape(-1)
    if not (base_strike > 0) or np.any(~(K > 0)):
        raise ValueError("strikes must be positive")
    return float(S_0) * float(base_strike) / K, K / float(base_strike)


def exercise_steps(T, delta_t, dates):
    """Step indices of calendar exercise dates: date t (time from the valuation date, 0 <= t < T) is time to maturity T - t,
    i.e. step (T - t) / delta_t of the sweep; t = 0 is step N.  Returns them strictly increasing.  Raises ValueError when a
    date is further than 1e-9 T from a step, outside [0, T), or listed twice."""
    steps = []
    for t in dates:
        x = (float(T) - float(t)) / float(delta_t)
        n = int(round(x))
        if abs(n * float(delta_t) - (float(T) - float(t))) > 1e-9 * float(T):
            raise ValueError("exercise date %r is not on the time grid (T = %r, delta_t = %r)" % (t, T, delta_t))
        if n < 1 or n * float(delta_t) > float(T) * (1 + 1e-9):
            raise ValueError("exercise date %r is outside [0, T)" % (t,))
        steps.append(n)
    if len(set(steps)) != len(steps):
        raise ValueError("an exercise date is listed twice")
    return sorted(steps)


def monitoring_steps(T, delta_t, dates):
    """Step indices of calendar monitoring dates of a barrier option: exercise_steps for dates in [0, T).  (A fixing at T itself
    is monitoring at maturity: knock_out_payoff.)"""
    return exercise_steps(T, delta_t, dates)


def fixing_steps(T, delta_t, dates):
    """Step indices of calendar fixing dates of a forward-start option or cliquet: exercise_steps for dates in [0, T)."""
    return exercise_steps(T, delta_t, dates)


def local_return_payoff(grids, ref_spot, strike=1.0, floor=None, cap=None):
    """The local-return payoff of a cliquet period on the host: clamp(s / ref_spot - strike, floor, cap) on every v-row,
    [n][(m1+1)(m2+1)].  ref_spot / strike / floor / cap: a scalar or one value per instance; None = no clamp on that side."""
    vs = np.asarray(grids.Vec_s, dtype=np.float64)
    n, m1p = vs.shape
    col = lambda x: np.broadcast_to(np.asarray(x, dtype=np.float64), (n,))[:, None]
    f = vs / col(ref_spot) - col(strike)
    if floor is not None:
        f = np.maximum(f, col(floor))
    if cap is not None:
        f = np.minimum(f, col(cap))
    nrows = int(np.asarray(grids.Vec_v).shape[1])
    return np.ascontiguousarray(np.broadcast_to(f[:, None, :], (n, nrows, m1p))).reshape(n, -1)


def knock_out_payoff(grids, U, lower, upper, rebate=None):
    """Monitoring at maturity, on the host: a copy of the payoff U [n][(m1+1)(m2+1)] in which every node whose spot is at or
    beyond a barrier (Vec_s <= lower or Vec_s >= upper: the library's comparison) holds the rebate (default 0), in every v-row.
    lower / upper / rebate: a scalar, one value per instance, or None."""
    vs = np.asarray(grids.Vec_s, dtype=np.float64)
    n, m1p = vs.shape
    col = lambda x, default: np.broadcast_to(np.asarray(default if x is None else x, dtype=np.float64), (n,))[:, None]
    knocked = (vs <= col(lower, -np.inf)) | (vs >= col(upper, np.inf))
    field = np.asarray(U, dtype=np.float64).reshape(n, -1, m1p)
    return np.where(knocked[:, None, :], col(rebate, 0.0)[:, :, None], field).reshape(n, -1)


# ---- LM linear algebra (host; jacobian_computation.cpp:20-195) -------------------------------------
LM_MAX_PAR = 8  # HADI_LM_MAX_PAR


def _lm_width(n_par):
    if not 1 <= n_par <= LM_MAX_PAR:
        raise ValueError("the LM functions take 1 .. %d parameters, not %d" % (LM_MAX_PAR, n_par))
    return n_par


def _lm_width_of(partials):
    """n_par of a partials vector [J^T J n_par^2][J^T r n_par][sum r^2]."""
    for n_par in range(1, LM_MAX_PAR + 1):
        if n_par * n_par + n_par + 1 == partials.size:
            return n_par
    raise ValueError("%d doubles are no partials vector of 1 .. %d parameters" % (partials.size, LM_MAX_PAR))


def lm_partials(J, residuals):
    """[J^T J (n_par^2), J^T r (n_par), sum r^2 (1)] of this rank's rows, n_par = J.shape[1]: the doubles that are all-reduced
    (31 at five parameters, 73 at eight)."""
    J, r = _host_f64(J), _host_f64(residuals)
    n_par = _lm_width(J.shape[1]) if J.ndim == 2 else 5
    out = np.empty(n_par * n_par + n_par + 1)
    if n_par == 5:
        rc = nat.lib().hadi_lm_partials(J.shape[0], J.ctypes.data_as(_dp), r.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    else:
        rc = nat.lib().hadi_lm_partials_n(J.shape[0], n_par, J.ctypes.data_as(_dp), r.ctypes.data_as(_dp), out.ctypes.data_as(_dp))
    if rc != nat.HADI_OK:
        raise HadiError(rc, "hadi_lm_partials")
    return out


def lm_partials_device(solver, J, model_prices, market_prices):
    """The same doubles reduced on the GPU from device-resident J [n][n_par], model prices [n] and market prices [n]
    (CUDA tensors): only they leave the device per LM iteration (hadi_lm_partials_device, hadi_lm_partials_device_n)."""
    n = int(J.shape[0])
    n_par = _lm_width(int(J.shape[1])) if J.dim() == 2 else 5
    for t, name, cnt in ((J, "J", n_par * n), (model_prices, "model_prices", n), (market_prices, "market_prices", n)):
        _check_array(t, name, cnt)
        if not _is_device(t):
            raise ValueError("%s must be a CUDA tensor" % name)
    solver.wait_stream()
    out = np.empty(n_par * n_par + n_par + 1)
    ptrs = (C.c_void_p(J.data_ptr()), C.c_void_p(model_prices.data_ptr()), C.c_void_p(market_prices.data_ptr()), out.ctypes.data_as(_dp))
    if n_par == 5:
        solver._call(solver._lib.hadi_lm_partials_device, n, *ptrs)
    else:
        solver._call(solver._lib.hadi_lm_partials_device_n, n, n_par, *ptrs)
    return out


def lm_solve(partials, lam):
    """delta [n_par] from a partials vector of lm_partials' layout; n_par follows from its length."""
    part = _host_f64(partials)
    n_par = _lm_width_of(part)
    delta = np.empty(n_par)
    if n_par == 5:
        rc = nat.lib().hadi_lm_solve(part.ctypes.data_as(_dp), float(lam), delta.ctypes.data_as(_dp))
    else:
        rc = nat.lib().hadi_lm_solve_n(n_par, part.ctypes.data_as(_dp), float(lam), delta.ctypes.data_as(_dp))
    if rc != nat.HADI_OK:
        raise HadiError(rc, "hadi_lm_solve")
    return delta


def compute_parameter_update(J, residuals, lam):
    """compute_parameter_update_on_device (jacobian_computation.cpp:107-195)."""
    return lm_solve(lm_partials(J, residuals), lam)
