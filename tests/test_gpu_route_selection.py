"""tests/golden/route_selection.json against the library itself: every recorded call replayed on a fresh handle (the code of
tools/record_routes.py --check).  The description, the deltas of the graph counters over two identical calls and the SHA-256 of
the returned array must be what run_sweep gave before csrc/hadi_route.h took its rules over: the same route, the same launches,
the same bits.  (Every hash of the fixture agreed between two recordings of that build: none is compared with the oracle
instead.)"""
import json
import os
import sys

import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_routes as R  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = json.load(open(R.FIXTURE))


@pytest.mark.parametrize("rec", FIX["cases"], ids=[c["in"]["name"] for c in FIX["cases"]])
def test_recorded_call(rec):
    got = R.run_case(H, rec["in"])
    if R.filled(rec["in"])["cu256"] and got["cu_count"] != FIX["cu_count"]:
        pytest.skip("recorded on the %d-CU device" % FIX["cu_count"])
    assert not R.compare(rec, got)
