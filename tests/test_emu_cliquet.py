"""CPU-only check of the strike fixings of forward-start options and cliquets under the wave emulator (tests/emu/emu_cliquet.cpp):
the five whole-loop kernels (hadi_small_kernel with 4 and 8 wavefronts, hadi_small_seq_kernel, hadi_small_seq2_kernel with an odd
batch, hadi_small_sch_kernel for CS / MCS / HV) apply the event to their LDS field inside their time loop (hadi_fixing_lds); the
streaming ring and strips are followed by hadi_fixing_gather_kernel and hadi_fixing_kernel; hadi_fixing_locate_kernel supplies the
reference nodes.  The emulator's lanes are host threads that meet only at the barriers, so a write of column i_ref that is not
ordered behind every reader of the row shows up here.  Every field is compared with tests/cliquet_ref.py at this file family's
bound, 1e-10 of the instance's max|U_ref|, on well-conditioned grids (asserted); with n_fix = 0 the run is bit for bit the plain
emulated run; no pad slot of the packed state changes against the same run without fixings; SHARES with w = 0 leaves node
(i_ref, j) with its bits and RETURN with w = 0 leaves every node of row j with c_j's bits.  tests/test_cliquet_ref.py shows that
i_ref +- 1, a shifted schedule, the other mode, a dropped fixing or a dropped weight moves the reference by >= 1e-4 of max|U|."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import bermudan_ref as BR
import cliquet_ref as QR
import common as Cm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_SO = os.path.join(HERE, "emu", "libhadi_emu_cliquet.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

BLOCK4, BLOCK8, SEQ, SEQ2, SCH, STREAM = range(6)
NAMES = {BLOCK4: "block4", BLOCK8: "block8", SEQ: "seq", SEQ2: "pairs", SCH: "sch", STREAM: "streaming"}
MODEL = (Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA)
TH = {0: Cm.THETA, 1: 0.5, 2: 1.0 / 3.0, 3: 0.5 + math.sqrt(3.0) / 6.0}
SHARES, RETURN = QR.SHARES, QR.RETURN


def _P(a):
    return None if a is None else a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def emu():
    csrc = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
    srcs = [os.path.join(HERE, "emu", f) for f in ("emu_cliquet.cpp", "emu_small_sch.cpp", "emu_driver.cpp", "wave_emu.h")] + \
           [os.path.join(csrc, f) for f in os.listdir(csrc)]
    if not os.path.exists(EMU_SO) or any(os.path.getmtime(s) > os.path.getmtime(EMU_SO) for s in srcs):
        tmp = "%s.tmp.%d" % (EMU_SO, os.getpid())  # (parallel test workers may all build: each moves a whole file into place)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-pthread", "-DHADI_EMU",
                               "-I" + os.path.join(HERE, "emu"), "-I" + csrc, "-o", tmp,
                               os.path.join(HERE, "emu", "emu_cliquet.cpp")])
        os.replace(tmp, EMU_SO)
    lib = C.CDLL(EMU_SO)
    lib.emu_cliquet_packed_size.restype = C.c_longlong
    lib.emu_set_tuning(b"reset", 0)
    return lib


_GRIDS = {}


def grids(m1, m2, n):
    """Well-conditioned batch (asserted), built once per shape and left unchanged."""
    if (m1, m2, n) not in _GRIDS:
        strikes = Cm.well_conditioned_strikes(m1, n)
        g = Cm.oracle_grids(m1, m2, strikes, V0=Cm.v0_for(m2))
        Cm.assert_well_conditioned(g[2], g[3])
        _GRIDS[(m1, m2, n)] = (strikes,) + g
    return _GRIDS[(m1, m2, n)]


def near_strike(m1, m2, n, shift=(0, 3, -2, 1, -5)):
    """Reference nodes around the instances' strikes: (i_ref [n], ref_spot [n])."""
    strikes, vs = grids(m1, m2, n)[:2]
    i = np.array([int(np.argmin(np.abs(vs[k] - strikes[k]))) + shift[k % 5] for k in range(n)])
    return i, np.array([vs[k][i[k]] for k in range(n)])


def padded(rows, n, dtype):
    """The host array of the ABI: [rows][width], zero-padded; one list = one shared row."""
    if rows and np.ndim(rows[0]) == 1:
        a = np.zeros((n, max(1, max(len(r) for r in rows))), dtype=dtype)
        for k, r in enumerate(rows):
            a[k, :len(r)] = r
        return a
    return np.asarray(rows, dtype=dtype).reshape(1, -1)


def run(emu, m1, m2, n, kind, N_i, dt_i, fix, ref_spot, mode, weights=None, payoff=None, scheme=0, put=False, div=False, strip=None):
    """(field [n][m], packed state, pad mask, located nodes and status words [2][n])."""
    strikes, vs, vv, ds, dv, U0 = grids(m1, m2, n)
    par8 = np.array([list(MODEL) + [dt_i[k], N_i[k], strikes[k] if put else 0.0, 1.0 if put else 0.0] for k in range(n)])
    Uin = Cm.put_payoff(vs, strikes, m2) if put else U0
    Uout = np.zeros_like(Uin)
    dd = [np.ascontiguousarray(x, dtype=np.float64) for x in Cm.DIVS] if div else [None] * 3
    a = padded(fix, n, np.int32)
    n_fix = 0 if a.size == 0 else a.shape[1]
    w = None if weights is None else np.ascontiguousarray(padded(weights, n, np.float64))
    assert w is None or w.shape == a.shape
    ref = np.ascontiguousarray(np.broadcast_to(np.asarray(ref_spot, dtype=np.float64), (n,)))
    md = np.ascontiguousarray(np.broadcast_to(np.asarray(mode, dtype=np.int32), (n,)))
    pay = None if payoff is None else np.ascontiguousarray(payoff, dtype=np.float64)
    size = emu.emu_cliquet_packed_size(n, m1, m2)
    P, pad, iref = np.zeros(size), np.zeros(size, dtype=np.uint8), np.zeros((2, n), dtype=np.int32)
    if strip is not None:
        emu.emu_set_tuning(b"strip", strip)
    try:
        rc = emu.emu_cliquet(n, m1, m2, C.c_double(TH[scheme]), C.c_double(Cm.R_D), C.c_double(Cm.R_F), _P(par8), _P(vs), _P(vv),
                             _P(ds), _P(dv), _P(Uin), _P(pay), kind, scheme, len(dd[0]) if div else 0, _P(dd[0]), _P(dd[1]), _P(dd[2]),
                             _P(ref), md.ctypes.data_as(_ip), n_fix, a.ctypes.data_as(_ip), a.shape[0], _P(w), _P(Uout), _P(P),
                             pad.ctypes.data_as(C.c_void_p), iref.ctypes.data_as(_ip))
    finally:
        emu.emu_set_tuning(b"reset", 0)
    assert rc == 0, rc
    assert emu.emu_take_error() == 0
    return Uout, P, pad.astype(bool), iref


def reference(m1, m2, n, N_i, dt_i, fix, ref_spot, mode, weights=None, payoff=None, scheme=0, put=False, div=False):
    strikes, vs, vv, ds, dv, U0 = grids(m1, m2, n)
    Uin = Cm.put_payoff(vs, strikes, m2) if put else U0
    return QR.solve_batch(m1, m2, max(N_i), dt_i[0], TH[scheme], Cm.R_D, Cm.R_F, *MODEL, vs, vv, ds, dv, Uin, fix, ref_spot, mode,
                          weights, payoff, dividends=Cm.DIVS if div else None, put_strikes=strikes if put else None, scheme=scheme,
                          N_i=N_i, dt_i=dt_i)


def check(emu, name, m1, m2, n, kind, N_i, dt_i, fix, ref_spot, mode, weights=None, **kw):
    strip = kw.pop("strip", None)
    U, P, pad, iref = run(emu, m1, m2, n, kind, N_i, dt_i, fix, ref_spot, mode, weights, strip=strip, **kw)
    Uo = reference(m1, m2, n, N_i, dt_i, fix, ref_spot, mode, weights, **kw)
    err = np.abs(U - Uo).max(axis=1) / np.abs(Uo).max(axis=1)
    print("%s %s %dx%d: %.2e of max|U_ref|" % (name, NAMES[kind], m1, m2, err.max()))
    assert np.isfinite(U).all() and err.max() <= 1e-10, (name, NAMES[kind], err)
    # the pad slots of the state: exactly what the same run leaves there without fixings
    _, P0, pad0, _ = run(emu, m1, m2, n, kind, N_i, dt_i, [], ref_spot, mode, strip=strip, **kw)
    assert pad.any() and np.array_equal(pad, pad0) and np.array_equal(P[pad], P0[pad]), (name, NAMES[kind])
    return U, iref


# (kind, strip tuning) of every path; 50x25 has one node per lane and so no strip kernel: its streaming run is the ring
DOUGLAS_PATHS = [(BLOCK4, None), (BLOCK8, None), (SEQ, None), (SEQ2, None), (STREAM, 0), (STREAM, 1)]
IDS = ["block4", "block8", "seq", "pairs", "ring", "strips"]
SHAPES = [(50, 25, 20), (100, 20, 8)]
MODES3, W3 = [SHARES, RETURN, RETURN], lambda N: [[0.0, 0.5, 1.0], [1.0, 0.0], []]


def cases(shapes):
    """Every path on every shape but the strips on one node per lane (50x25: that run is the ring's)."""
    out = [(m1, m2, N, k, s) for m1, m2, N in shapes for k, s in DOUGLAS_PATHS if not (s == 1 and m1 <= 64)]
    return out, ["%dx%dx%d-%s" % (m1, m2, N, IDS[DOUGLAS_PATHS.index((k, s))]) for m1, m2, N, k, s in out]


def uniform(n, N):
    return [N] * n, [Cm.T / N] * n


def paying(N):
    return sorted(BR.dividend_steps(N, Cm.T / N, Cm.DIVS[0]))


@pytest.mark.parametrize("m1,m2,N,kind,strip", cases(SHAPES)[0], ids=cases(SHAPES)[1])
def test_dividends_puts_and_per_instance_schedules(emu, m1, m2, N, kind, strip):
    """Three instances (the pairs kernel's last wavefront holds one), each with its own reference node, mode, schedule and weights
    (zero and non-zero mixed).  Instance 0 fixes at the END of a step that pays a dividend at its START and at the valuation date
    n = N; instance 1 one step later and not at N; instance 2 never."""
    pay = paying(N)
    assert len(pay) >= 2 and (N != 20 or pay == [4, 8, 11, 16])
    fix = [[pay[0], pay[1], N], [pay[0] + 1, pay[1] + 1], []]
    _, ref = near_strike(m1, m2, 3)
    check(emu, "DIV put per-instance", m1, m2, 3, kind, *uniform(3, N), fix, ref, MODES3, W3(N), put=True, div=True, strip=strip)


SHORT = [(50, 25, 6), (100, 20, 4)]


@pytest.mark.parametrize("m1,m2,N,kind,strip", cases(SHORT)[0], ids=cases(SHORT)[1])
@pytest.mark.parametrize("put,div", [(False, False), (False, True), (True, False)], ids=["EU-call", "DIV-call", "EU-put"])
def test_shared_schedule(emu, m1, m2, N, kind, strip, put, div):
    """One schedule and one weight list for the batch; a payoff P that is not the initial field."""
    _, ref = near_strike(m1, m2, 3)
    strikes, vs = grids(m1, m2, 3)[:2]
    pay = np.repeat(np.minimum(np.maximum(vs / ref[:, None] - 1.0, 0.0), 0.08)[:, None, :], m2 + 1, axis=1).reshape(3, -1)
    check(emu, "shared", m1, m2, 3, kind, *uniform(3, N), [1, N // 2 + 1, N], ref, [RETURN, SHARES, RETURN], [1.0, 0.0, 0.25],
          payoff=pay, put=put, div=div, strip=strip)
    check(emu, "shared, no weights", m1, m2, 3, kind, *uniform(3, N), [1, N // 2 + 1, N], ref, SHARES, put=put, div=div, strip=strip)


@pytest.mark.parametrize("kind,strip", DOUGLAS_PATHS, ids=IDS)
@pytest.mark.parametrize("div", [False, True], ids=["EU", "DIV"])
def test_mixed_step_grids(emu, kind, strip, div):
    """Every instance its own (N_i, dt_i), dividend dating, schedule, reference node, mode and weights; the pairs kernel holds
    instances of different N (the dispatch order puts 8 with 7, 6 with 5, and 3 alone) and different schedules in one wavefront."""
    N_i = [5, 8, 3, 7, 6]
    dt_i = [0.5 / 5, Cm.T / 8, 0.25 / 3, 0.8 / 7, 0.6 / 6]
    fix = [[2, 5], [1, 4, 8], [3], [], [3, 4]]
    w = [[1.0, 0.0], [0.0, 0.5, 0.0], [2.0], [], [0.0, 0.0]]
    m1, m2 = (100, 20) if strip else (50, 25)
    _, ref = near_strike(m1, m2, 5)
    check(emu, "mixed", m1, m2, 5, kind, N_i, dt_i, fix, ref, [SHARES, RETURN, SHARES, RETURN, RETURN], w, put=True, div=div, strip=strip)
    if not div:  # ... and one schedule for all of them, within the shortest time loop
        check(emu, "mixed shared", m1, m2, 5, kind, N_i, dt_i, [1, 3], ref, [RETURN, SHARES, SHARES, RETURN, SHARES], [0.0, 1.0],
              put=True, strip=strip)


@pytest.mark.parametrize("scheme", [1, 2, 3], ids=["CS", "MCS", "HV"])
@pytest.mark.parametrize("m1,m2,N,kind,strip", [(50, 25, 6, SCH, None), (100, 20, 4, SCH, None), (50, 25, 6, STREAM, 0),
                                                 (100, 20, 4, STREAM, 1)], ids=["50x25-sch", "100x20-sch", "50x25-ring", "100x20-strips"])
def test_schemes(emu, scheme, m1, m2, N, kind, strip):
    """The fixing follows the corrector's column pass."""
    _, ref = near_strike(m1, m2, 3)
    check(emu, "scheme %d" % scheme, m1, m2, 3, kind, *uniform(3, N), [[1, N], [2], [N // 2, N - 1]], ref, MODES3,
          [[0.5, 0.0], [1.0], [0.0, 0.0]], scheme=scheme, strip=strip)


# ---- the reference node: every special slot, and the exact-bit properties ------------------------------------------------------
@pytest.mark.parametrize("m1,m2,kind,strip", [(50, 25, BLOCK4, None), (50, 25, BLOCK8, None), (50, 25, SEQ, None), (50, 25, SEQ2, None),
                                              (50, 25, STREAM, 0), (100, 20, BLOCK8, None), (100, 20, SEQ, None), (100, 20, STREAM, 0),
                                              (100, 20, STREAM, 1)],
                         ids=["50x25-block4", "50x25-block8", "50x25-seq", "50x25-pairs", "50x25-ring", "100x20-block8", "100x20-seq",
                              "100x20-ring", "100x20-strips"])
def test_reference_node_placements_and_exact_bits(emu, m1, m2, kind, strip):
    """Six instances, no weights, one fixing at the last step so that the event's output is what the run returns.  RETURN with
    i_ref = 0 (the special slot behind the row) and i_ref = m1; SHARES with i_ref = 1 and m1; an odd and an even i_ref (the two
    halves of a 16-byte pair; with two nodes per lane also the last node of a lane and the first of the next).  The fields are the
    reference's, the located nodes are these, and: SHARES leaves (i_ref, j) with the bits of the run without the fixing; RETURN
    leaves every node of row j with those bits."""
    n, N = 6, 3
    vs = grids(m1, m2, n)[1]
    i_ref = [0, m1, 1, m1, m1 // 2 | 1, (m1 // 2 | 1) + 1]
    modes = [RETURN, RETURN, SHARES, SHARES, SHARES, RETURN]
    ref = np.array([vs[k][i_ref[k]] for k in range(n)])
    U, iref = check(emu, "placements", m1, m2, n, kind, *uniform(n, N), [N], ref, modes, put=True, strip=strip)
    assert iref[0].tolist() == i_ref and not iref[1].any(), iref
    plain, _, _, _ = run(emu, m1, m2, n, kind, *uniform(n, N), [], ref, modes, put=True, strip=strip)
    Ur, Pr = U.reshape(n, m2 + 1, m1 + 1), plain.reshape(n, m2 + 1, m1 + 1)
    for k in range(n):
        c = Pr[k][:, i_ref[k]]
        assert np.array_equal(Ur[k][:, i_ref[k]], c), k
        if modes[k] == RETURN:
            assert np.array_equal(Ur[k], np.repeat(c[:, None], m1 + 1, axis=1)), k
        else:
            assert not np.array_equal(Ur[k][:, i_ref[k] - 1], c), k


def test_locate_kernel_applies_the_price_picks_rule(emu):
    """Within 1e-10 is on the node; further off is off the grid: -1 and a status word, and the field is left alone."""
    m1, m2, n, N = 50, 25, 3, 2
    vs = grids(m1, m2, n)[1]
    ref = np.array([vs[0][20] + 5e-11, vs[1][20] + 2e-10, 0.5 * (vs[2][7] + vs[2][8])])
    U, _, _, iref = run(emu, m1, m2, n, STREAM, *uniform(n, N), [1, 2], ref, RETURN, strip=0)
    assert iref.tolist() == [[20, -1, -1], [0, 1, 1]], iref
    plain, _, _, _ = run(emu, m1, m2, n, STREAM, *uniform(n, N), [], ref, RETURN, strip=0)
    assert np.array_equal(U[1:], plain[1:]) and not np.array_equal(U[0], plain[0])
    V, _, _, iref = run(emu, m1, m2, n, BLOCK4, *uniform(n, N), [1, 2], ref, RETURN)
    plain4, _, _, _ = run(emu, m1, m2, n, BLOCK4, *uniform(n, N), [], ref, RETURN)
    assert np.array_equal(V[1:], plain4[1:]) and not np.array_equal(V[0], plain4[0]) and iref.tolist() == [[20, -1, -1], [0, 1, 1]]


# ---- n_fix = 0 is the plain emulated run, bit for bit -------------------------------------------------------------------------
def plain(emu, m1, m2, n, kind, N, scheme, put, div, strip):
    """emu_solve / emu_small_sch (emu_driver.cpp, emu_small_sch.cpp) on the same inputs."""
    strikes, vs, vv, ds, dv, U0 = grids(m1, m2, n)
    U = (Cm.put_payoff(vs, strikes, m2) if put else U0).copy()
    par = np.array([list(MODEL)] * n)
    if kind == SCH:
        par8 = np.array([list(MODEL) + [Cm.T / N, N, 0.0, 0.0] for _ in range(n)])
        rc = emu.emu_small_sch(n, m1, m2, C.c_double(TH[scheme]), C.c_double(Cm.R_D), C.c_double(Cm.R_F), _P(par8), _P(vs), _P(vv),
                               _P(ds), _P(dv), _P(U), scheme, 64, None)
        assert rc == 0, rc
        return U
    dd = [np.ascontiguousarray(x, dtype=np.float64) for x in Cm.DIVS] if div else [None] * 3
    ks = np.ascontiguousarray(strikes, dtype=np.float64) if put else None
    use_small = {BLOCK4: 1, BLOCK8: 2, SEQ: 3, SEQ2: 5, STREAM: 0}[kind]
    if strip is not None:
        emu.emu_set_tuning(b"strip", strip)
    try:
        rc = emu.emu_solve(n, m1, m2, N, C.c_double(Cm.T / N), C.c_double(TH[scheme]), C.c_double(Cm.R_D), C.c_double(Cm.R_F), _P(par),
                           2 if div else 0, _P(vs), _P(vv), _P(ds), _P(dv), _P(U), None, None, 8 * 256, len(dd[0]) if div else 0,
                           _P(dd[0]), _P(dd[1]), _P(dd[2]), 64, use_small, {0: 0, 1: 1, 2: 4, 3: 5}[scheme], _P(ks), None, None)
    finally:
        emu.emu_set_tuning(b"reset", 0)
    assert rc == 0, rc
    return U


@pytest.mark.parametrize("kind,strip,scheme", [(k, s, 0) for k, s in DOUGLAS_PATHS] + [(SCH, None, 2), (STREAM, 0, 3)],
                         ids=IDS + ["sch-MCS", "ring-HV"])
def test_empty_schedule_is_the_plain_run_bit_for_bit(emu, kind, strip, scheme):
    m1, m2 = (100, 20) if strip else (50, 25)
    N = 5
    put, div = (scheme == 0), (scheme == 0)
    _, ref = near_strike(m1, m2, 3)
    U, _, _, _ = run(emu, m1, m2, 3, kind, *uniform(3, N), [], ref, MODES3, scheme=scheme, put=put, div=div, strip=strip)
    assert np.array_equal(U, plain(emu, m1, m2, 3, kind, N, scheme, put, div, strip))


# ---- the route of a cliquet call ----------------------------------------------------------------------------------------------
SMALL_SCH, SMALL, SMALL_SEQ, SMALL_SEQ2, TEAM, STREAMING = range(6)  # enum HadiRouteKind
FIX_LOOP, FIX_STREAM = "; cliquet: strike fixing at the end of %d steps inside the time loop", \
                       "; cliquet: hadi_fixing_kernel after each of %d fixing steps"


def route(emu, n, m1, m2, n_fix_steps, weights=False, variant=0, scheme=0, tuning="", cus=256, theta=Cm.THETA, team=0):
    arr = (C.c_int * 16)(cus, n, m1, m2, variant, scheme, 0, 0, 0, 0, 0, int(variant == 2), 1, 0, 0, team)
    o, subs, desc = (C.c_longlong * 17)(), (C.c_int * (4 * 64))(), C.create_string_buffer(1024)
    emu.emu_route_cliquet.argtypes = [C.c_void_p, C.c_double, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p,
                                      C.c_int]
    assert emu.emu_route_cliquet(arr, theta, tuning.encode(), n_fix_steps, int(weights), o, subs, 64, desc, 1024) == 0
    return list(o), [tuple(subs[4 * k:4 * k + 4]) for k in range(o[3])], desc.value.decode()


def test_route_never_the_team_launch_or_the_resident_sweep(emu):
    # team-eligible: 300x140 x 4; resident-eligible: 300x80 x 256 and 512x256 x 256
    o, _, d = route(emu, 4, 300, 140, 0)
    assert o[1] == TEAM and "cliquet" not in d
    o, _, d = route(emu, 4, 300, 140, 2)
    assert o[1] == STREAMING and o[15] == 1 and d.endswith(FIX_STREAM % 2), d
    for n, m1, m2, tuning in ((256, 300, 80, "resident_sweep=1"), (256, 512, 256, "")):
        o, subs, d = route(emu, n, m1, m2, 0, tuning=tuning)
        assert o[6] == 1 and "hadi_sweep_resident" in d, d
        o, subs, d = route(emu, n, m1, m2, 12, tuning=tuning)
        assert o[1] == STREAMING and o[6] == 0 and not any(s[3] for s in subs) and "hadi_sweep_resident" not in d, d
        assert "row pass" in d and d.endswith(FIX_STREAM % 12), d
    # 512x256 x 320: a round and a remainder, side by side on two streams
    o, subs, d = route(emu, 320, 512, 256, 1)
    assert [s[1] for s in subs] == [256, 64] and o[4] == 1 and "two streams" in d, d


def test_route_takes_the_whole_loop_kernels_by_the_existing_rules(emu):
    cases = [(3, 50, 25, 0, "", SMALL), (300, 50, 25, 0, "", SMALL_SEQ), (600, 50, 25, 0, "", SMALL_SEQ2),
             (3, 50, 25, 0, "small_seq=1,small_pairs=1", SMALL_SEQ2), (300, 50, 25, 2, "", SMALL_SCH), (3, 50, 25, 2, "small_sch=1", SMALL_SCH),
             (20, 300, 80, 0, "", STREAMING)]
    for n, m1, m2, scheme, tuning, kind in cases:
        o0, s0, d0 = route(emu, n, m1, m2, 0, scheme=scheme, tuning=tuning, theta=TH[scheme])
        for weights in (False, True):
            o1, s1, d1 = route(emu, n, m1, m2, 3, weights, scheme=scheme, tuning=tuning, theta=TH[scheme])
            assert o0[1] == o1[1] == kind, (n, m1, m2, scheme, tuning, o0[1], o1[1])
            assert o0[:15] == o1[:15] and s0 == s1 and o0[15] == 0 and o1[15] == 1
            assert o0[16] == 0 and o1[16] == int(weights)  # (the packed payoff only where a weight is non-zero)
            assert d1 == d0 + (FIX_STREAM if kind == STREAMING else FIX_LOOP) % 3 and "cliquet" not in d0, (d0, d1)


def test_recorded_routes(emu):
    """tests/golden/route_selection_cliquet.json, recorded on the MI355X (tools/record_cliquet_routes.py): hadi_route and
    hadi_describe_route reproduce the description of every recorded cliquet call and of the plain call of the same batch."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import record_cliquet_routes as R
    fix = json.load(open(R.FIXTURE))
    assert len(fix["cases"]) == len(R.CASES) >= 12
    for row in fix["cases"]:
        tuning = ",".join("%s=%d" % kv for kv in row["tuning"].items())
        kw = dict(scheme=row["scheme"], tuning=tuning, cus=fix["cu_count"], theta=R.TH[row["scheme"]])
        o0, _, _ = route(emu, row["n"], row["m1"], row["m2"], 0, **kw)
        team = 1 if o0[1] == TEAM else 0  # (a team launch is taken to have run)
        weights = bool(row["weights"]) and any(w != 0.0 for w in row["weights"])
        assert route(emu, row["n"], row["m1"], row["m2"], 0, team=team, **kw)[2] == row["plain"], row["name"]
        o1, _, d1 = route(emu, row["n"], row["m1"], row["m2"], len(row["fix_steps"]), weights, **kw)
        assert d1 == row["cliquet"] and o1[15] == 1 and o1[1] != TEAM, (row["name"], d1)
