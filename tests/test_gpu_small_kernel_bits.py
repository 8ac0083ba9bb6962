"""tests/golden/small_kernel_bits.json against the library itself: every recorded call replayed on a fresh handle (the code of
tools/record_small_bits.py --check).  The fixture was recorded, twice with equal hashes, from a libhadi.so built at commit 39417d4
("Price Bermudan options: exercise on chosen steps of a sweep"; tests/golden/README.md): the kernel named in the description and the SHA-256 of the returned array must be the same.  tests/golden/route_selection.json pins
the same kernels on two steps of European call data only; here dividends are paid (asserted with the dating mirror when a case
is built), puts, two nodes per lane, m2 > m1, nrows 32 and 33, per-instance N, exercise and the ladder all reach them."""
import json
import os
import sys

import pytest

import pde_based_heston_solver_gpu_accelerated_amd as H

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import record_routes as R  # noqa: E402
import record_small_bits as RB  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = json.load(open(RB.FIXTURE))


def test_fixture_holds_every_case():
    assert [c["in"] for c in FIX["cases"]] == RB.CASES


@pytest.mark.parametrize("rec", FIX["cases"], ids=[c["in"]["name"] for c in FIX["cases"]])
def test_recorded_call(rec):
    assert rec["desc"] == rec["in"]["expect"]  # (the recording reached its kernel)
    assert not R.compare(rec, RB.run_case(H, rec["in"]))
