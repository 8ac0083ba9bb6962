"""GPU regression tests of the cases a fuzz campaign flagged (tools/fuzz_parity.py; round 2: gpurun_out/fuzz_a.log seed 2024
cases 378 and 485, gpurun_out/fuzz_small.log seed 5 case 279), adjudicated by the extended-precision build of the oracle
(oracle/heston_oracle_xp.c), and of the device error word behind the bounded pair rendezvous."""
import importlib.util
import os

import numpy as np
import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H

import common as Cm
import fuzz_cases as F

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("fuzz_parity", os.path.join(os.path.dirname(Cm.HERE), "tools", "fuzz_parity.py"))
FP = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FP)


def _worst_instances(r, count):
    """The most ill-conditioned instances of a batch and the instance libhadi and the oracle differ most on."""
    per = np.abs(r["U"] - r["Uo"]).max(axis=1)
    if r["lo"] is not None:
        per = per + np.abs(r["lam"] - r["lo"]).max(axis=1)
    ks = list(np.argsort(-r["ratio"])[:count]) + [int(np.argmax(per))]
    return sorted(set(int(k) for k in ks))


def test_fuzz_seed5_case279_small_american_dividend(solver):
    """'BAD' in round 2 (field 1.16e-7 / lambda_bar 1.24e-6 against the oracle on one instance of 130): instance 101 has S_0
    inserted 7.4e-6 beside a node of a 16-interval s-grid.  The adjudicator showed the defect was libhadi's -- the
    one-node-per-lane cyclic reduction (1.7e-7 from the exact result against the oracle's 4.5e-10) -- fixed by the
    excess-carrying update in hadi_row_step (see tests/test_emu_kernel_logic.py for the CPU twin of this test).  Same batch,
    same kernel choice as the campaign; every ill-conditioned instance within 3x of the oracle's own distance from exact."""
    c = F.case(5, 279, small=True)
    assert F.summary(c) == "AM_DIV m1=16 m2=11 N=9 n=130 r_f=0.03"
    r = FP.run_case(solver, c)
    assert "hadi_small_kernel<1,8,AM>" in r["path"]
    for k in _worst_instances(r, 3):
        a = FP.adjudicate(c, r, k)
        assert a["hadi_U"] < max(3 * a["oracle_U"], 1e-11), (k, a)
        assert a["hadi_lam"] < max(10 * a["oracle_lam"], 1e-9), (k, a)
    ok, j = FP.judge(c, r)
    assert ok, j


def test_fuzz_seed2024_case378_wide_american_put(solver):
    """'BAD' in round 2 by the tool's lambda_bar bound alone (1.23e-7 against the oracle; field 3.4e-10): 977 x 29, two
    wavefronts per row, explicit (U, lambda_bar) pair, instance 96 with neighbouring s-intervals 8021x apart (1.9e-5 beside
    0.155).  Adjudicated: BOTH fp64 solvers sit at cond * eps from the exact result there -- field: libhadi 4.4e-10, oracle
    1.9e-10; lambda_bar (= the unprojected field's error / dt): 1.2e-7 against 1.2e-8.  Scanning the position of such an
    interval over the lanes (same parameters, emulator) the ratio of the two distances ranges over 0.2 .. 5.6: realisations
    of the same round-off, no systematic loss -- unlike the one-node-per-lane defect of case 279 (380x).  Bound: 30x."""
    c = F.case(2024, 378)
    assert F.summary(c) == "AM put m1=977 m2=29 N=12 n=130 r_f=0.00"
    r = FP.run_case(solver, c)
    assert "hadi_pass_a<8,2,4,1,1,AM>" in r["path"]
    for k in _worst_instances(r, 2):
        a = FP.adjudicate(c, r, k)
        assert a["hadi_U"] < max(30 * a["oracle_U"], 1e-11), (k, a)
        assert a["hadi_lam"] < max(30 * a["oracle_lam"], 1e-9), (k, a)
    ok, j = FP.judge(c, r)
    assert ok, j


def test_fuzz_seed2024_case485_fp32_state_dividend_put(solver):
    """'BAD' in round 2 by the fp32-state bound (3.4e-6 against 2e-7 N = 2.4e-6): paired strips, fp32 state, put with
    dividends, 691 x 92.  The checker of this mode is the oracle with the same two roundings per step; the adjudicator (exact
    arithmetic, state rounded where the kernels round it) agrees with that oracle to the last bit here, so the 3.5e-6 are
    libhadi's: float roundings flipped by last-bit fp64 differences (6e-8 each) and grown by the same mechanism that grows
    the mode's own rounding noise -- on this batch the fp32-state oracle is 2.2e-5 from the fp64-state one.  The yardstick is
    therefore that noise, PER INSTANCE: libhadi's distance from the checker stays below 1.5x the checker's own distance
    from the fp64 result on well-conditioned instances (most instances differ by 0 or 1 float ulp; the flagged one by 3.4e-6,
    its noise being 3.6e-6), and below 4x on the one ill-conditioned instance (s-intervals 30x apart: 2.8e-5 against 1.1e-5
    -- flips amplified like the noise itself)."""
    from oracle import oracle as O
    c = F.case(2024, 485)
    assert F.summary(c) == "DIV put f32 m1=691 m2=92 N=12 n=70 r_f=0.00"
    r = FP.run_case(solver, c)
    assert "hadi_pass_a_strip<8,EU,float,2>" in r["path"]
    g, N = r["grids"], c["N"]
    p64 = O.make_params(c["m1"], c["m2"], N, Cm.T / N, Cm.THETA, Cm.R_D, c["r_f"], *c["model"], c["variant"], Cm.DIVS,
                        option_type=O.PUT, strikes=np.array(c["strikes"]))
    U64, _, _ = O.solve_batch(p64, g.Vec_s, g.Vec_v, g.Delta_s, g.Delta_v, r["U0"], r["U0"])
    scale = np.abs(U64).max()
    mine = np.abs(r["U"] - r["Uo"]).max(axis=1) / scale     # libhadi vs the fp32-state checker
    noise = np.abs(r["Uo"] - U64).max(axis=1) / scale       # the fp32 state's own rounding noise, per instance
    ill = r["ratio"] > 30
    assert (mine[~ill] < 1.5 * noise[~ill] + 2e-7 * N).all(), (mine[~ill].max(), noise[~ill].max())
    assert (mine[ill] < 4 * noise[ill] + 2e-7 * N).all(), (mine[ill], noise[ill])
    k = int(np.argmax(np.where(ill, 0.0, mine)))
    a = FP.adjudicate(c, r, k)
    assert a["oracle_U"] < 1e-7 and a["hadi_U"] < 1.5 * noise[k] + 2e-7 * N, (k, a, noise[k])


def test_fuzz_seed331_case358_fp32_state_on_an_ill_conditioned_wide_grid(solver):
    """'BAD' in round 3's last campaign by the 4x rule of the case above: DIV put, fp32 state, 910 x 171, shared-ring row pass;
    instance 9 has neighbouring s-intervals 482x apart and libhadi sits 1.28e-5 (of the batch's max |U|) from the fp32-state
    checker where the checker itself is 1.67e-6 from the fp64 result: 7.7x that instance's own fp32 noise (instance 42,
    ratio 32: 4.0x; the well-conditioned instances: at most 3.7x of a noise of 1e-7 .. 1.8e-6, inside 1.5x + 2e-7 N).  Float
    roundings flipped by last-bit fp64 differences, amplified by the 1/ds^2 coefficients like the noise itself -- the mode's
    error level on such an instance is 1e-5 either way (it does not meet 1e-6 on ANY 2000-step run).
    Bound for ill-conditioned instances: 10x the instance's noise."""
    from oracle import oracle as O
    c = F.case(331, 358)
    assert F.summary(c) == "DIV put f32 m1=910 m2=171 N=11 n=70 r_f=0.03"
    r = FP.run_case(solver, c)
    assert "hadi_pass_a<8,2,4,1,1,EU,float>" in r["path"]
    g, N = r["grids"], c["N"]
    p64 = O.make_params(c["m1"], c["m2"], N, Cm.T / N, Cm.THETA, Cm.R_D, c["r_f"], *c["model"], c["variant"], Cm.DIVS,
                        option_type=O.PUT, strikes=np.array(c["strikes"]))
    U64, _, _ = O.solve_batch(p64, g.Vec_s, g.Vec_v, g.Delta_s, g.Delta_v, r["U0"], r["U0"])
    scale = np.abs(U64).max()
    mine = np.abs(r["U"] - r["Uo"]).max(axis=1) / scale
    noise = np.abs(r["Uo"] - U64).max(axis=1) / scale
    ill = r["ratio"] > 30
    assert ill.sum() >= 3 and r["ratio"].max() > 400
    assert (mine[~ill] < 1.5 * noise[~ill] + 2e-7 * N).all(), (mine[~ill].max(), noise[~ill].max())
    assert (mine[ill] < 10 * noise[ill] + 2e-7 * N).all(), (mine[ill], noise[ill])
    assert mine.max() < 3e-5
    ok, j = FP.judge(c, r)
    assert ok, j


def test_gpu_sweep_seed1052_case1_tall_grid_american_lambda_bar(solver):
    """Outside the bounds in round 4's second campaign (tools/gpu_sweep.py 1052 1, case 1): one American call on a 102 x 432 grid
    -- taller than anything the frozen generator of tools/fuzz_parity.py draws: 14 column chunks -- P representation on forced
    strips, 3 steps.  lambda_bar 1.4e-8 against the oracle (bound 1e-8), field 5.3e-11.  Adjudicated (binary128): libhadi 3.9e-10
    from the exact field where the oracle is 3.9e-10, lambda_bar 2.8e-8 where the oracle is 3.3e-8 -- round-off in both solvers
    alike, and the larger campaign (11 400 cases) said whose: ALL its outliers sit on m2 = 432, the one v-grid size whose V_0 =
    0.04 is inserted 2.4e-8 beside a node (v-intervals 2.8e4 x apart; 2.5 .. 3.8 x at every other size tried): the column
    operator's twin of the ill-conditioned s-grids of DESIGN.md section 2.  Pinned as the adjudicated relation: libhadi within 3x
    of the oracle's own distance from exact."""
    from oracle import oracle as O
    m1, m2, N, ks = 102, 432, 3, [86.33639475947474]
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, ks)
    U0 = grids.call_payoff(ks)
    p = Cm.oracle_params(m1, m2, N, O.AM, r_f=0.0)
    Uo, lo, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0, want_lambda=True)
    U, lam = U0.copy(), np.zeros_like(U0)
    solver.set_tuning("strip", 1)
    try:
        solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.0, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U,
                               variant=H.AM, U_0=U0, lambda_bar=lam)
        path = solver.describe_last_sweep()
    finally:
        solver.set_tuning("strip", -1)
    assert "hadi_pass_a_strip<2,AM-P>" in path and "hadi_pass_b1<16,AM-P>" in path, path
    Ux, lx = O.solve_xp(p, grids.Vec_s[0], grids.Vec_v[0], grids.Delta_s[0], grids.Delta_v[0], U0[0], U0[0])
    sc, sl = np.abs(Ux).max(), max(1.0, np.abs(lx).max())
    hadi_U, oracle_U = np.abs(U[0] - Ux).max() / sc, np.abs(Uo[0] - Ux).max() / sc
    hadi_l, oracle_l = np.abs(lam[0] - lx).max() / sl, np.abs(lo[0] - lx).max() / sl
    assert hadi_U < max(3 * oracle_U, 1e-11), (hadi_U, oracle_U)
    assert hadi_l < max(3 * oracle_l, 1e-9), (hadi_l, oracle_l)
    assert np.abs(U - Uo).max() <= 1e-10 * np.abs(Uo).max()


@pytest.mark.parametrize("what", ["put", "am_p", "call_R1e4"])
@pytest.mark.parametrize("strip", [0, 1], ids=["ring", "paired_strips"])
def test_two_wavefront_rows_with_a_tiny_interval_astride(solver, strip, what):
    """Found by tests/test_gpu_ill_grids.py (the tiny interval PLACED between node 512, the last of wavefront 0, and node 513, the
    first of wavefront 1, of a 600-interval row): put data, R = 1e6: libhadi 1.45e-7 of max|U| from binary128 where the fp64 oracle
    is 3.4e-9 (43x); the American sweep at R = 1e5: 2.15e-8 against 6.3e-10 (34x); a call at R = 1e4: 2.4e-9 against 1.1e-10 (11x) --
    on the shared ring and on paired strips alike, on the last v-rows (v = 5, where the row operator's couplings are largest),
    smooth along s; the wave emulator, whose reciprocals are IEEE divisions, stood at 0.06 .. 1.3x.  Cause: hadi_rcp's one Newton
    step leaves every reciprocal LOW by e^2 <= 2^-49; the cyclic reduction of a two-wavefront row hands Bc and Dd to the pair's
    2x2 system, whose determinant 1 - Bc Dd is ~1 / R for such a pair of nodes, and the six levels' common bias is amplified by R
    (reproduced on the CPU by giving the emulator the device's reciprocal, tests/test_emu_ill_grids.py).  Fixed by the third-order
    step on the reduction's reciprocals of G = 2 rows (hadi_rcp_acc).  Same batches as the finding, judged by the frozen rule and
    pinned as the adjudicated relation: the flagged instance within 10x of the yardstick."""
    import ill_grids as I
    import test_gpu_ill_grids as T
    from oracle import oracle as O
    kw = {"put": dict(put=True), "am_p": dict(variant=O.AM), "call_R1e4": {}}[what]
    tuning = dict(T._st(strip=strip), american_p=1)
    c = I.cfg(3, r_f=T.R_F, **kw)
    insts, _ = T._batch(solver, tuning, 600, 40, "s", 1 if what == "call_R1e4" else 0, c)
    U, lam, d, _ = T._sweep(solver, tuning, insts, c)
    assert ("hadi_pass_a_strip<8," in d and "paired strips" in d) if strip else "hadi_pass_a<8,2," in d, d
    verdicts = T._judge("600x40 %s %s" % ("paired strips" if strip else "ring", what), c, insts, U, lam)
    k = next(i for i, x in enumerate(insts) if x.sname == "astride two wavefronts")
    Ux, lx = I.exact(c, insts[k])
    e_h = I.distances(U[k], None, Ux, None)[0]
    y = I.yard(c, insts[k])[0]
    print("astride two wavefronts: e_h %.2e, yard %.2e, ratio %.2f" % (e_h, y, e_h / y))
    assert e_h < max(10 * y, 1e-11), (e_h, y)


@pytest.mark.parametrize("strip", [1, 0])
def test_rendezvous_timeout_fails_the_call(solver, strip):
    """The pair rendezvous of the two-wavefront rows (paired strips / shared ring, m1 > 512) polls a bounded number of
    times; running out of polls used to fall through to a solve with stale exchange values and HADI_OK.  Now the kernel
    records it in the handle's device error word and the call fails with HADI_ERR_INTERNAL.  Forced here by a test hook
    that withholds one token per row 1; the next call (hook off) is clean again and bit-identical to a fresh solve."""
    m1, m2, N, strikes = 700, 40, 2, [100.0, 93.0]
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, strikes)
    U0 = grids.call_payoff(strikes)

    def run():
        U = U0.copy()
        solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.0, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U)
        return U

    solver.set_tuning("strip", strip)
    try:
        good = run()
        assert ("paired strips" in solver.describe_last_sweep()) == bool(strip)
        solver.set_tuning("debug_fault", 1)
        with pytest.raises(H.HadiError) as ei:
            run()
        assert ei.value.status == 7 and "rendezvous" in str(ei.value)  # HADI_ERR_INTERNAL
        solver.set_tuning("debug_fault", 0)
        assert np.array_equal(run(), good)
    finally:
        solver.set_tuning("debug_fault", 0)
        solver.set_tuning("strip", -1)


# ---- instance-resident launch (hadi_team_kernel) ----------------------------------------------------------------------------
def _team_case(m1, m2, N, strikes, put=False, r_f=0.0, div=False):
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, strikes)
    U0 = grids.put_payoff(strikes) if put else grids.call_payoff(strikes)
    from oracle import oracle as O
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, r_f, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.DIV if div else O.EU,
                      Cm.DIVS if div else None, option_type=O.PUT if put else O.CALL, strikes=np.array(strikes) if put else None)
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0)
    kw = dict(option_type=H.PUT, strikes=strikes) if put else {}
    if div:
        kw.update(variant=H.DIV, dividends=H.Dividends(*Cm.DIVS))
    return grids, U0, Uo, kw


@pytest.mark.parametrize("m1,m2,N,n,put,r_f,div", [(512, 256, 12, 1, False, 0.0, False), (512, 256, 6, 8, False, 0.01, False), (300, 140, 10, 3, True, 0.0, False),
                                                   (256, 128, 10, 5, False, 0.0, False), (200, 30, 8, 2, False, 0.02, False), (400, 263, 5, 2, True, 0.01, False),
                                                   (512, 256, 12, 2, False, 0.0, True), (256, 128, 24, 8, True, 0.01, True), (300, 140, 6, 1, False, 0.0, True)])
def test_instance_resident_launch_vs_oracle_and_streaming_path(solver, m1, m2, N, n, put, r_f, div):
    """Batches of up to 8 large European instances run their whole time loop in ONE launch, every instance kept in the L2 of
    one XCD by a team of 32 blocks (hadi_team_kernel; the reference runs all N steps of an instance inside one kernel,
    device_solver.hpp:83-88,226-265).  Full field against the oracle (1e-10) and against the two-launches-per-step path
    (1e-11: same operators, the row step of the strip kernels against the shared-ring one); 8 and 4 nodes per lane, 1 .. 8
    column chunks, call and put boundary data, r_f != 0 (the boundary time factors then need an exp per step)."""
    strikes = Cm.strikes_for(n)
    grids, U0, Uo, kw = _team_case(m1, m2, N, strikes, put, r_f, div)  # (div: discrete dividends -- the jump runs inside the launch)
    res = {}
    for mode in (1, 0):
        solver.set_tuning("team_launch", mode)
        try:
            U = U0.copy()
            solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, r_f, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U, **kw)
            res[mode] = (U, solver.describe_last_sweep(), solver.get_tuning("team_launch"))
        finally:
            solver.set_tuning("team_launch", -1)
    assert "hadi_team_kernel" in res[1][1] and res[1][2] == 1, res[1][1:]   # it ran, and the team protocol did not fail
    assert "hadi_team_kernel" not in res[0][1]
    scale = np.abs(Uo).max()
    assert np.abs(res[1][0] - Uo).max() < 1e-10 * scale
    assert np.abs(res[1][0] - res[0][0]).max() < 1e-11 * scale


@pytest.mark.parametrize("m1,m2,N,n", [(512, 256, 1000, 1), (512, 256, 600, 8), (256, 128, 800, 3)])
def test_instance_resident_launch_over_a_long_time_loop_matches_the_streaming_path(solver, m1, m2, N, n):
    """The cross-CU visibility of the team kernel (stores acknowledged by the XCD's L2, `buffer_inv sc1` behind every team
    barrier, L1-bypassing loads) over a LONG loop: 600 - 1000 steps = 1200 - 2000 team barriers per instance, every one a
    chance for a stale L1 line to return the previous step's row.  The whole field against the two-launches-per-step path
    (no oracle at this size: it would take minutes), plus the recorded price of the literal config 2."""
    strikes = Cm.strikes_for(n)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, strikes)
    U0 = grids.call_payoff(strikes)
    res = {}
    for mode in (1, 0):
        solver.set_tuning("team_launch", mode)
        try:
            U = U0.copy()
            solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, Cm.R_F, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U)
            res[mode] = (U, solver.describe_last_sweep(), solver.get_tuning("team_launch"))
        finally:
            solver.set_tuning("team_launch", -1)
    assert "hadi_team_kernel" in res[1][1] and res[1][2] == 1, res[1][1:]
    assert "hadi_team_kernel" not in res[0][1]
    scale = np.abs(res[0][0]).max()
    assert np.abs(res[1][0] - res[0][0]).max() < 2e-11 * scale
    if (m1, m2, N, n) == (512, 256, 1000, 1):
        g = H.Grid(m1, 800.0, Cm.S_0, 100.0, 20.0, m2, 5.0, Cm.V_0, 5.0 / 500)
        price = res[1][0][0, g.find_s_index(Cm.S_0) + g.find_v0_index(Cm.V_0) * (m1 + 1)]
        assert abs(price - 8.8942192888223310) < 1e-9


def test_instance_resident_launch_is_the_default_for_small_batches_of_large_grids(solver):
    strikes = Cm.strikes_for(2)
    grids, U0, Uo, kw = _team_case(512, 256, 4, strikes)
    U = U0.copy()
    solver.DO_timestepping(512, 256, 4, Cm.T / 4, Cm.THETA, Cm.R_D, 0.0, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U)
    assert "hadi_team_kernel<8>" in solver.describe_last_sweep()
    assert np.abs(U - Uo).max() < 1e-10 * np.abs(Uo).max()
    # nine instances, American sweeps, theta = 0: the streaming kernels
    for kw2, nn in ((dict(), 9), (dict(variant=H.AM, U_0=None), 2)):
        ks = Cm.strikes_for(nn)
        g2 = H.GridViewsBatch.for_strikes(512, 256, Cm.S_0, Cm.V_0, ks)
        U2 = g2.call_payoff(ks)
        if "variant" in kw2:
            kw2 = dict(variant=H.AM, U_0=U2.copy())
        solver.DO_timestepping(512, 256, 2, Cm.T / 2, Cm.THETA, Cm.R_D, 0.0, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, g2, U2, **kw2)
        assert "hadi_team_kernel" not in solver.describe_last_sweep()


def test_a_failed_team_launch_falls_back_to_the_streaming_path():
    """Every wait of the instance-resident launch is bounded.  Test hook: one block of every team deserts before the first
    barrier -> the others run out of polls (~0.1 s), the kernel records HADI_DEVERR_TEAM, and the SAME call returns the right
    field from the two-launches-per-step path; the automatic choice then stays away from the launch on this handle."""
    s = H.HestonADI(0)
    try:
        strikes = Cm.strikes_for(2)
        grids, U0, Uo, kw = _team_case(300, 140, 5, strikes)
        s.set_tuning("debug_fault", 128)
        U = U0.copy()
        s.DO_timestepping(300, 140, 5, Cm.T / 5, Cm.THETA, Cm.R_D, 0.0, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U)
        assert "after a failed instance-resident launch" in s.describe_last_sweep()
        assert s.get_tuning("team_launch") == -2
        assert np.abs(U - Uo).max() < 1e-10 * np.abs(Uo).max()
        s.set_tuning("debug_fault", 0)
        U = U0.copy()
        s.DO_timestepping(300, 140, 5, Cm.T / 5, Cm.THETA, Cm.R_D, 0.0, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U)
        assert "hadi_team_kernel" not in s.describe_last_sweep()  # stays away
        assert np.abs(U - Uo).max() < 1e-10 * np.abs(Uo).max()
    finally:
        s.close()


# ---- shapes beyond the streaming kernels (sequential passes) ------------------------------------------------------------------
@pytest.mark.parametrize("m1,m2,N,n,variant,name,put", [(1500, 600, 3, 2, H.EU, "EU", False), (300, 800, 3, 3, H.EU, "EU", False),
                                                        (1100, 100, 4, 2, H.AM, "AM", True), (200, 560, 24, 2, H.AM_DIV, "AM_DIV", False),
                                                        (1030, 530, 3, 1, H.DIV, "DIV", False), (2100, 40, 3, 2, H.EU, "EU", False)])
def test_grids_beyond_1024_s_intervals_or_527_v_intervals(solver, m1, m2, N, n, variant, name, put):
    """The reference bounds a grid by its total size only (src/perfomance_test.cpp:62); rounds 1-2 rejected m1 > 1024 and
    m2 > 527.  Such grids run on sequential passes in the reference's own thread mapping -- hadi_pass_a_seq (lane <-> v-row,
    hes_a1_kernels.hpp:139-161) and hadi_pass_b_seq (lane <-> s-column, hes_a2_shuffled_kernels.hpp:243-299) -- each combined
    with the streaming kernel of the other direction where that one still fits.  Full field (and lambda_bar) against the
    oracle at the usual 1e-10."""
    from oracle import oracle as O
    strikes = Cm.strikes_for(n)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, strikes)
    U0 = grids.put_payoff(strikes) if put else grids.call_payoff(strikes)
    U, lam = U0.copy(), np.zeros_like(U0)
    american = variant in (H.AM, H.AM_DIV)
    div = H.Dividends(*Cm.DIVS) if variant in (H.DIV, H.AM_DIV) else None
    solver.DO_timestepping(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U, variant=variant,
                           U_0=U0, lambda_bar=lam if american else None, dividends=div, option_type=H.PUT if put else H.CALL,
                           strikes=strikes if put else None)
    path = solver.describe_last_sweep()
    assert ("hadi_pass_a_seq" in path) == (m1 > 1024) and ("hadi_pass_b_seq" in path) == (m2 > 527), path
    p = O.make_params(m1, m2, N, Cm.T / N, Cm.THETA, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, Cm.VARIANT[name],
                      Cm.DIVS if div is not None else None, option_type=O.PUT if put else O.CALL, strikes=np.array(strikes) if put else None)
    Uo, lo, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0, want_lambda=True)
    assert np.abs(U - Uo).max() < 1e-10 * np.abs(Uo).max()
    if american:
        assert np.abs(lam - lo).max() < 1e-8 * max(1.0, np.abs(lo).max())


# ---- the strips at a tiny theta (tests/test_gpu_time_regimes.py, regime T7) ----------------------------------------------------
@pytest.mark.parametrize("name,m1,m2,n,tuning,kernel", [
    ("strips", 300, 80, 4, {"strip": 1, "team_launch": 0, "resident_sweep": 0, "small_grid": 0}, "hadi_pass_a_strip<8,EU>"),
    ("pairs", 200, 60, 4, {"strip": 1, "pair_strips": 1, "team_launch": 0, "resident_sweep": 0, "small_grid": 0}, "hadi_pass_a_pairs<EU>"),
    ("paired_strips", 600, 40, 4, {"strip": 1, "team_launch": 0, "resident_sweep": 0, "small_grid": 0}, "hadi_pass_a_strip<8,EU,double,2>"),
    ("team", 300, 140, 3, {"team_launch": 1}, "hadi_team_kernel<8>"),
    ("resident", 300, 80, 256, {"resident_sweep": 1}, "hadi_sweep_resident<8>")])
def test_strip_step_at_theta_1e_minus_9(solver, name, m1, m2, n, tuning, kernel):
    """theta = 1e-9, dt = 1e-6, N = 3: hadi_strip_step formed theta dt A1 U from the implicit diagonal, (1 - im) u0 with
    im = fl(1 + theta dt r_d / 2 - (il + iu)), which keeps 1 - im to eps ABSOLUTE, and carried it into the step with
    kap = (1 - theta) / theta: an error of eps / theta of |U| whatever dt.  Under the wave emulator, before the fix, against
    the oracle (itself <= 1e-13 from its binary128 twin there): strips 3.6e-7, pairs 3.5e-7, paired strips 3.6e-7, team kernel
    3.6e-7 (1.0e-6 with dividends), resident sweep 3.6e-7 of max|U|, the shared-ring and LDS kernels 2e-16 .. 7e-16; at
    theta = 0.8 the same term is 5e-17 and nothing showed.  Below theta = 1e-3 the step now forms il + iu - theta dt r_d / 2 on
    its own and im from it (hadi_strip_theta; above it every bit stays what it was): <= 2e-15 on the same cases.  Every
    strip-step kernel, full field at the project's 1e-10."""
    from oracle import oracle as O
    if name in ("team", "resident") and solver.device_info()["compute_units"] != 256:
        pytest.skip("needs the 256-CU device")
    theta, dt, N = 1e-9, 1e-6, 3
    strikes = Cm.well_conditioned_strikes(m1, n)
    grids = H.GridViewsBatch.for_strikes(m1, m2, Cm.S_0, Cm.V_0, strikes)
    Cm.assert_well_conditioned(grids.Delta_s, grids.Delta_v)
    U0 = grids.call_payoff(strikes)
    U = U0.copy()
    defaults = {"strip": -1, "pair_strips": -1, "team_launch": -1, "resident_sweep": -1, "small_grid": 1}
    for k, v in tuning.items():
        solver.set_tuning(k, v)
    try:
        solver.DO_timestepping(m1, m2, N, dt, theta, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, grids, U)
        path = solver.describe_last_sweep()
    finally:
        for k in tuning:
            solver.set_tuning(k, defaults[k])
    assert kernel in path, path
    p = O.make_params(m1, m2, N, dt, theta, Cm.R_D, 0.01, Cm.RHO, Cm.SIGMA, Cm.KAPPA, Cm.ETA, O.EU)
    Uo, _, _ = O.solve_batch(p, grids.Vec_s, grids.Vec_v, grids.Delta_s, grids.Delta_v, U0, U0, threads=16)
    assert np.isfinite(Uo).all() and np.abs(Uo - U0).max() > 1e-5 * np.abs(Uo).max()  # (the three steps moved the field)
    e = (np.abs(U - Uo).max(axis=1) / np.abs(Uo).max(axis=1)).max()
    print("%s at theta 1e-9: field error %.3e of max|U_ref|" % (name, e))
    assert e <= 1e-10, e
