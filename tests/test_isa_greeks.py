"""Build-time check of the Greeks kernel (hadi_greeks_kernel) from the compiler's own metadata and assembly (no GPU): no scratch
and no spills -- its per-node weight and output arrays must stay in registers."""
import os, re, subprocess, sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def greeks():
    import kernel_regs
    rows, asm = kernel_regs.collect()
    body = None
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        if name.startswith("hadi_greeks_kernel("):
            body = m.group(2)
    regs = [r for r in rows if r[0].startswith("hadi_greeks_kernel(")]
    return body, regs


def test_no_scratch_and_no_spills(greeks):
    body, regs = greeks
    assert body is not None and len(regs) == 1
    assert not re.search(r"\bscratch_(load|store)", body)
    _, vgpr, sgpr, spill, scratch, lds = regs[0]
    assert spill == 0 and scratch == 0, regs[0]
    assert vgpr <= 128  # 256 threads per block: two blocks per SIMD stay possible
    assert lds == 0     # dynamic LDS only (at most 52 KB: six staged rows of 1040 doubles)


def test_results_leave_in_vector_stores(greeks):
    body, _ = greeks
    assert len(re.findall(r"\bglobal_store_dwordx4\b", body)) >= 8  # a ladder row and the node row: 4 x 16 bytes each
