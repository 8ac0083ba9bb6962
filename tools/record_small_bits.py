"""Records (or, with --check, replays) tests/golden/small_kernel_bits.json: the bits of the one-launch small-grid kernels and of
every kernel that applies the dividend jump.

tests/golden/route_selection.json runs two steps of European call data: no dividend is ever paid, and put data, two nodes per
lane, m2 > m1, per-instance step counts, exercise and the ladder never reach hadi_small_seq_kernel, hadi_small_seq2_kernel,
hadi_small_sch_kernel or hadi_small_kernel.  The cases here do: each is one call through the public Python API on a fresh
handle, twice, with its kernel pinned by tuning keys and asserted from describe_last_sweep().  Recorded per case: the inputs,
the piece of the description that names the kernel, and the SHA-256 of the returned array's bytes.

    python tools/record_small_bits.py [--lib other/libhadi.so] [--out file.json]   # record (the committed fixture: from the parent build)
    python tools/record_small_bits.py --against first.json                         # second recording: a case whose hash differs is dropped
    python tools/record_small_bits.py --check [--lib ...]                           # replay the committed fixture and compare

tests/test_gpu_small_kernel_bits.py runs run_case() below and record_routes.compare(), so the test and --check are one
implementation.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
import dividend_schedules as D  # noqa: E402  (the suite's mirror of the dividend dating rule)
import time_regimes as TR  # noqa: E402
from record_routes import DIVS, ETA, KAPPA, R_D, RHO, S_0, SIGMA, T, V_0, compare, holds  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "small_kernel_bits.json")
R_F, THETA = 0.01, 0.8
CS, MCS, HV = 1, 2, 3
SCHEME_THETA = {CS: 0.5, MCS: 1.0 / 3.0, HV: 0.5 + 3.0 ** 0.5 / 6.0}
# input kinds: name -> (variant, put, N)
INPUTS = {"eu_call": ("EU", 0, 7), "div_put": ("DIV", 1, 10), "div_call_rotated": ("DIV", 0, 4), "bermudan": ("DIV", 0, 10),
          "ladder": ("DIV", 1, 10), "amdiv_call": ("AM_DIV", 0, 10),
          "sch_bermudan": ("EU", 0, 7), "sch_ladder": ("EU", 0, 7)}
VARIANTS = {"EU": 0, "DIV": 2, "AM_DIV": 3}
# The rotated batch holds steps of 5, 1e-6, 0.25 and 1e-3 on one schedule (dated on each instance's own clock, consumed in
# array order): one date inside a step interval of each of the three short clocks
ROTATED_DIVS = ([1.5e-6, 2.5e-3, 0.8], [0.5, 0.3, 0.2], [0.02] * 3)


def _cases():
    out = []

    def add(kernel, tuning, m1, m2, inp, n=5, scheme=0):
        name = "%s_%dx%d_%s" % (kernel[0], m1, m2, inp)
        out.append(dict(name=name, m1=m1, m2=m2, n=n, input=inp, expect=kernel[1] % (1 if m1 <= 64 else 2) if "%d" in kernel[1] else kernel[1],
                        tuning=tuning, scheme=scheme))

    seq = (("seq", "hadi_small_seq_kernel<%d>"), {"small_seq": 1, "small_pairs": 0})
    seq2 = (("seq2", "hadi_small_seq2_kernel<%d>"), {"small_seq": 1, "small_pairs": 1})
    blk4 = (("block4", "hadi_small_kernel<%d,4,"), {"small_seq": 0, "small_waves": 4})
    blk8 = (("block8", "hadi_small_kernel<%d,8,"), {"small_seq": 0, "small_waves": 8})
    rest = ("div_call_rotated", "bermudan", "ladder")
    # every shape on the two sequential kernels, European call and dividend put (64x32: nrows 33, seq only; 64x31: both halves full)
    for k, shapes in ((seq, [(50, 25), (65, 8), (128, 26), (20, 25), (64, 32)]), (seq2, [(50, 25), (65, 8), (128, 26), (20, 25), (64, 31)])):
        for m1, m2 in shapes:
            for inp in ("eu_call", "div_put"):
                add(*k, m1, m2, inp)
    # the remaining inputs where one and where two nodes sit in a lane
    for m1, m2 in ((50, 25), (65, 8)):
        for k in (seq, seq2):
            for inp in rest:
                add(*k, m1, m2, inp)
        for inp in ("eu_call", "div_put") + rest:
            add(*blk4, m1, m2, inp)
    for inp in ("eu_call", "div_put") + rest:
        add(*blk8, 50, 25, inp)
    add(("block4", "hadi_small_kernel<%d,4,AM>"), blk4[1], 50, 25, "amdiv_call")
    for sch, sname in ((CS, "CS"), (MCS, "MCS"), (HV, "HV")):
        for m1, m2 in ((50, 25), (65, 8)):
            for inp in ("eu_call", "sch_bermudan", "sch_ladder"):
                add(("sch" + sname, "hadi_small_sch_kernel<%d," + sname + ">"), {"small_sch": 1}, m1, m2, inp, scheme=sch)
    # the dividend jump outside LDS: hadi_dividend_kernel between the streaming passes (the description names the passes only),
    # and the team kernel's own
    add(("streaming", "row pass hadi_pass_a<"), {"small_grid": 0, "team_launch": 0}, 128, 64, "div_put", n=3)
    add(("team", "hadi_team_kernel<"), {"team_launch": 1}, 256, 128, "div_put", n=2)
    return out


CASES = _cases()


def run_case(H, case, lib_path=None):
    """The case twice on a fresh handle: {"desc", "sha256"} -- and the two results must be the same bytes."""
    c = case
    m1, m2, n, inp = c["m1"], c["m2"], c["n"], c["input"]
    variant, put, N = INPUTS[inp]
    strikes = [85.0 + 30.0 * k / (n - 1) for k in range(n)]
    grids = H.GridViewsBatch.for_strikes(m1, m2, S_0, V_0, strikes)
    if put:
        U0 = np.ascontiguousarray(np.tile(np.maximum(np.asarray(strikes).reshape(-1, 1) - grids.Vec_s, 0.0), (1, m2 + 1)))
    else:
        U0 = grids.call_payoff(strikes)
    dt, r_f = T / N, R_F
    theta = SCHEME_THETA.get(c["scheme"], THETA)
    kw = dict(variant=VARIANTS[variant], scheme=c["scheme"])
    if put:
        kw.update(option_type=H.PUT, strikes=strikes)
    if variant != "EU":
        kw["dividends"] = H.Dividends(*DIVS)
        assert inp == "div_call_rotated" or D.paying_steps(N, dt, DIVS[0]), "no dividend is paid"
    if variant == "AM_DIV":
        kw["U_0"] = U0
    if inp == "div_call_rotated":  # every instance its own (dt, N) and its own model parameters
        times = TR.time_rotation(n)
        kw["dividends"] = H.Dividends(*ROTATED_DIVS)
        payers = [k for k, (dt_k, N_k) in enumerate(times) if D.paying_steps(N_k, dt_k, ROTATED_DIVS[0])]
        assert len(payers) >= 3 and len(payers) < n, "the batch must hold instances that pay and instances that do not: %r" % payers
        kw["per_instance"] = dict(TR.per_instance(times), rho_i=[RHO + 0.1 * k for k in range(n)], sigma_i=[SIGMA + 0.02 * k for k in range(n)],
                                  kappa_i=[KAPPA + 0.1 * k for k in range(n)], eta_i=[ETA + 0.005 * k for k in range(n)])
        assert max(t[1] for t in times) == N
    if inp == "sch_ladder":
        r_f = 0.0  # (call boundary data: the ladder takes r_f = 0 only)
    args = (m1, m2, N, dt, theta, R_D, r_f, RHO, SIGMA, KAPPA, ETA, grids)
    with H.HestonADI(0, lib_path=lib_path) as sv:
        for k, v in c["tuning"].items():
            sv.set_tuning(k, v)
        before = [sv.get_tuning("graph_captures"), sv.get_tuning("graph_replays")]
        res = []
        for _ in range(2):
            U = U0.copy()
            if inp in ("ladder", "sch_ladder"):
                out = sv.maturity_ladder(*args, U, S_0, V_0, [3, 7, 10] if N == 10 else [2, 5, 7], **kw)
            elif inp in ("bermudan", "sch_bermudan"):  # one schedule per instance: the rows differ, one is empty
                ex = [[2, N], [1, 3, 5], [], [3], [4, N - 1]][:n]
                out = sv.bermudan_timestepping(*args, U, ex, **kw)
            else:
                lam = np.zeros_like(U) if variant == "AM_DIV" else None
                out = sv.DO_timestepping(*args, U, lambda_bar=lam, **kw)
            res.append(hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest())
        desc = sv.describe_last_sweep()
        after = [sv.get_tuning("graph_captures"), sv.get_tuning("graph_replays")]
    assert res[0] == res[1], "%s: two identical calls on one handle returned different bytes" % c["name"]
    # (the fragment, not the whole text: the fixture stays small)
    return {"desc": c["expect"] if holds(c["expect"], desc) else "NOT " + c["expect"] + ": " + desc,
            "graph": [after[0] - before[0], after[1] - before[1]], "sha256": res[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libhadi.so (same ABI)")
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--check", action="store_true", help="replay the fixture instead of recording it")
    ap.add_argument("--against", default=None, help="a first recording of the same build: a case whose hash differs is dropped")
    a = ap.parse_args()
    import pde_based_heston_solver_gpu_accelerated_amd as H
    if a.check:
        bad = 0
        fix = json.load(open(FIXTURE))
        for rec in fix["cases"]:
            diff = compare(rec, run_case(H, rec["in"], a.lib))
            bad += bool(diff)
            print("%-40s %s" % (rec["in"]["name"], "ok" if not diff else "; ".join(diff)), flush=True)
        print("%d of %d cases differ" % (bad, len(fix["cases"])))
        return 1 if bad else 0
    first = {r["in"]["name"]: r for r in json.load(open(a.against))["cases"]} if a.against else None
    rows, dropped, missed = [], 0, 0
    for case in CASES:
        got = run_case(H, case, a.lib)
        same = first is None or (case["name"] in first and not compare(first[case["name"]], got))
        ok = got["desc"] == case["expect"]
        print("%-40s %s%s%s %s" % (case["name"], "" if ok else "MISSES ITS KERNEL (%s) " % got["desc"],
                                   "" if same else "DIFFERS FROM THE FIRST RECORDING: DROPPED ", got["graph"], got["sha256"][:16]), flush=True)
        if same:
            rows.append({"in": case, **got})
        dropped += not same
        missed += not ok
    with open(a.out, "w") as f:
        f.write('{"cases": [\n')
        f.write(",\n".join("  {\"in\": %s,\n   \"graph\": %s, \"desc\": %s, \"sha256\": \"%s\"}"
                           % (json.dumps(r["in"]), json.dumps(r["graph"]), json.dumps(r["desc"]), r["sha256"]) for r in rows))
        f.write("\n ]}\n")
    print("%d cases -> %s; %d dropped, %d miss their kernel" % (len(rows), a.out, dropped, missed))
    return 1 if missed else 0


if __name__ == "__main__":
    sys.exit(main())
