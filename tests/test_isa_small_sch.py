"""Build-time check of hadi_small_sch_kernel from the compiler's own metadata (no GPU): no spilled registers, no scratch, no
static LDS (the four fields and the tables are dynamic LDS) in any of its instantiations."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def regs():
    import kernel_regs
    rows, _ = kernel_regs.collect()
    return [r for r in rows if "hadi_small_sch_kernel<" in r[0]]


def test_no_spills_no_scratch_no_static_lds(regs):
    assert len(regs) == 6, regs  # 1 and 2 nodes per lane of the packed layout x CS, MCS, HV
    for name, vgpr, sgpr, spill, scratch, lds in regs:
        print("%s: %d VGPRs, %d SGPRs" % (name, vgpr, sgpr))
        assert spill == 0 and scratch == 0 and lds == 0, (name, spill, scratch, lds)
