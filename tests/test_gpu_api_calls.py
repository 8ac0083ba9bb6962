"""tests/golden/api_calls.json against the library itself: every recorded call replayed on a fresh handle (the code of
tools/record_api_calls.py --check).  Result cases: the SHA-256 of every returned array, the description and the deltas of the graph
counters over two identical calls; refusal cases: the status and the exact hadi_last_error text, so the order of the host-side
checks is pinned with their words.  Recorded from the build before the host drivers of csrc/hadi_api.hip were restructured around
one call description; every hash agreed between two recordings of that build."""
import json
import os
import sys

import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_api_calls as R  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = json.load(open(R.FIXTURE))


def test_fixture_covers_the_case_list():
    assert [c["in"] for c in FIX["cases"]] == R.CASES


@pytest.mark.parametrize("rec", FIX["cases"], ids=[c["in"]["name"] for c in FIX["cases"]])
def test_recorded_call(rec):
    assert not R.compare(rec, R.run_case(H, rec["in"]))
