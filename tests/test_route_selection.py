"""The route of a whole call -- csrc/hadi_route.h: which whole-loop kernel or streaming path, which sub-batches and streams, which
of them on the resident sweep, whether the loop is replayed from a graph, and how hadi_describe_last_sweep words it -- against
tests/golden/route_selection.json, recorded on the MI355X from run_sweep as it stood before the header took the rules over
(tests/golden/README.md).  The route is reached through the wave emulator's driver (emu_route)."""
import ctypes as C
import json
import os
import re
import sys

import pytest

from test_emu_kernel_logic import emu  # noqa: F401  (the fixture that builds tests/emu/libhadi_emu.so)

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import record_routes as R  # noqa: E402

FIX = json.load(open(R.FIXTURE))
SMALL_SCH, SMALL, SMALL_SEQ, SMALL_SEQ2, TEAM, STREAMING = range(6)  # enum HadiRouteKind
TEAM_RAN = 1
OUT = ("status", "kind", "small_waves", "nsub", "two_streams", "fork_before", "n_resident", "read_payoff_shape", "pair_tab",
       "need_lam_u0", "need_ut", "need_f32", "need_v_r1_c2", "need_r1", "graphable")


def route(emu, case, cus=256):  # noqa: F811
    """The route of a fixture case on a device of `cus` CUs: (dict of OUT, [(off, cnt, lane, resident)], description).  The
    payoff-shape read-back is what the case's payoff says; a team launch is taken to have run."""
    c = R.filled(case)
    variant = R.VARIANTS[c["variant"]]
    tuning = ",".join("%s=%d" % kv for kv in c["tuning"].items()).encode()

    def call(amp, team):
        arr = (C.c_int * 16)(cus, c["n"], c["m1"], c["m2"], variant, c["scheme"], c["prec"], int(c["r_f"] == R.R_D), 0, c["profiling"],
                             len(c["snap"]) if c["call"] == "ladder" else 0, int(variant in (2, 3)), 1, 0, amp, team)
        o, subs, desc = (C.c_longlong * 15)(), (C.c_int * (4 * 64))(), C.create_string_buffer(1024)
        emu.emu_route.argtypes = [C.c_void_p, C.c_double, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int]
        rc = emu.emu_route(arr, c["theta"], tuning, o, subs, 64, desc, 1024)
        assert rc == 0, (case["name"], rc, o[0])
        out = dict(zip(OUT, o))
        return out, [tuple(subs[4 * k:4 * k + 4]) for k in range(out["nsub"])], desc.value.decode()

    out, _, _ = call(0, 0)
    return call(int(bool(out["read_payoff_shape"]) and c["payoff"] == "s"), TEAM_RAN if out["kind"] == TEAM else 0)


def said(desc):
    """What a recorded description says about the cut: (sub-batch sizes or None for one sub-batch, two streams, only the last
    two on two streams, resident sub-batches or 'all')."""
    m = re.search(r"; (\d+) sub-batches of ([\d ]+) instances", desc)
    sizes = None
    if m:
        sizes = [int(x) for x in m.group(2).split()]
        sizes = sizes * int(m.group(1)) if len(sizes) == 1 else sizes
        assert len(sizes) == int(m.group(1)), desc
    k = re.search(r"in one launch for (\d+) sub-batches of one round", desc)
    res = int(k.group(1)) if k else "all" if "both passes of every step in one launch: hadi_sweep_resident<8>" in desc else 0
    return sizes, "side by side on two streams" in desc, "the last two side by side" in desc, res


def test_fixture_covers_the_branches():
    assert FIX["cu_count"] == 256 and len(FIX["cases"]) >= 60
    assert os.path.getsize(R.FIXTURE) <= 256 * 1024
    assert [c["in"] for c in FIX["cases"]] == R.CASES  # (the recorder's list is what was recorded)
    for c in FIX["cases"]:
        assert R.holds(c["in"]["expect"], c["desc"]), (c["in"]["name"], c["desc"])  # the branch the case is there for


@pytest.mark.parametrize("rec", FIX["cases"], ids=[c["in"]["name"] for c in FIX["cases"]])
def test_recorded_route(emu, rec):  # noqa: F811
    out, subs, desc = route(emu, rec["in"])
    assert desc == rec["desc"]  # byte for byte
    # a loop replayed from a graph is captured by the first of the two identical calls and replayed by the second
    loop = out["kind"] == STREAMING
    assert rec["graph"] == ([1, 1] if loop and out["graphable"] else [0, 0]), (out, rec["graph"])
    sizes, two, last_two, res = said(rec["desc"])
    if out["kind"] in (TEAM, SMALL_SCH, SMALL, SMALL_SEQ, SMALL_SEQ2):
        assert sizes is None and res == 0
        return
    assert [s[1] for s in subs] == (sizes or [rec["in"]["n"]])
    assert bool(out["two_streams"]) == two and (out["fork_before"] > 0) == last_two
    assert {s[2] for s in subs} == ({0, 1} if two else {0})
    assert out["n_resident"] == (len(subs) if res == "all" else res) == sum(s[3] for s in subs)


@pytest.mark.parametrize("cus", [304, 64])
def test_invariants_on_other_devices(emu, cus):  # noqa: F811
    """No recording for these devices: what must hold on any."""
    for rec in FIX["cases"]:
        out, subs, _ = route(emu, rec["in"], cus)
        assert out["kind"] != TEAM, rec["in"]["name"]  # the team is the 256-CU device's
        assert all(s[1] <= cus for s in subs if s[3]), (rec["in"]["name"], subs)  # a resident sub-batch is one round of CUs
        assert sum(s[1] for s in subs) == rec["in"]["n"] and [s[0] for s in subs] == [sum(x[1] for x in subs[:k]) for k in range(len(subs))]
