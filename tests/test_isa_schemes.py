"""Build-time guards (no GPU) of the Modified Craig-Sneyd / Hundsdorfer-Verwer row passes, the same as tests/test_isa_counts.py
applies to hadi_pass_a_strip / hadi_pass_a: their counted `s_waitcnt vmcnt(n)` know the LDS-DMA pieces, the row stores and the
corrector's R1 / C2 register loads, nothing else -- so no scratch, exactly the DMA pieces of the strip formula, and at least the
stores and loads the counts assume."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

STORES = lambda B: 1 if B == 1 else B // 2                # hadi_put_block_stores<B, double>
PAD = lambda B: 8 if B < 4 else 16                         # HADI_ROW_PAD(B, 8)
STRIP_NS = lambda B, G: 3 if G == 2 else 4                 # HADI_STRIP_NS(B, G, 8)


@pytest.fixture(scope="module")
def kernels():
    import kernel_regs
    rows, asm = kernel_regs.collect()
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        if name.startswith("void hadi_pass_a_strip_sch<") or name.startswith("void hadi_pass_a_sch<"):
            out[name.replace("(HadiSweepArgs, int)", "").replace("void ", "")] = m.group(2)
    return rows, out


def _args(name):
    return [int(a) for a in name[name.index("<") + 1:name.rindex(">")].split(",")]


def test_every_scheme_kernel_is_there(kernels):
    _, k = kernels
    strips = [n for n in k if n.startswith("hadi_pass_a_strip_sch<")]
    rings = [n for n in k if n.startswith("hadi_pass_a_sch<")]
    # strips: 2, 4, 8 nodes per lane x (predictor, corrector) + the paired strips' corrector, per scheme
    assert len(strips) == 2 * (3 * 2 + 1) and len(rings) == 2 * 2 * 5, sorted(k)


def test_strip_kernels_issue_the_dma_pieces_stores_and_loads_the_waits_count(kernels):
    _, k = kernels
    for name, body in k.items():
        if not name.startswith("hadi_pass_a_strip_sch<"):
            continue
        B, G, mode, sch = _args(name)
        n_dma = len(re.findall(r"\bglobal_load_lds_dwordx4\b", body))
        n_st = len(re.findall(r"\bglobal_store_dwordx4\b", body))
        rowp = 64 * B * G + PAD(B)
        pieces = -(-(rowp * 8 // 16) // 64) if G == 1 else (B * 8 // 16) + 1
        assert n_dma == (STRIP_NS(B, G) + 1) * pieces, (name, n_dma)
        # predictor: two copies of the step (last v-row or not), each stores Y, R1 and C2; corrector: one copy, Y
        assert n_st >= (6 if mode == 1 else 1) * STORES(B), (name, n_st)
        if mode == 2:  # R1 and C2 rows at two sites (prologue, loop), HV included (its C2 is loaded and counted, not used)
            n_x4 = len(re.findall(r"\bglobal_load_dwordx4\b", body))
            assert n_x4 >= 2 * 2 * (B // 2) + 3 * (B // 2), (name, n_x4)


def test_ring_kernels_issue_at_least_the_stores_the_waits_count(kernels):
    _, k = kernels
    for name, body in k.items():
        if not name.startswith("hadi_pass_a_sch<"):
            continue
        B = _args(name)[0]
        wide = len(re.findall(r"\bglobal_store_dwordx4\b", body))
        narrow = len(re.findall(r"\bglobal_store_dwordx2\b", body)) + len(re.findall(r"\bglobal_store_dword\b", body))
        assert (wide if B >= 2 else narrow) >= 2 * STORES(B), name


def test_no_scheme_row_kernel_touches_scratch(kernels):
    rows, _ = kernels
    seen = 0
    for name, vgpr, sgpr, spills, scratch, lds in rows:
        if "hadi_pass_a_strip_sch<" in name or "hadi_pass_a_sch<" in name:
            assert spills == 0 and scratch == 0 and vgpr <= 256, (name, vgpr, spills, scratch)
            seen += 1
    assert seen == 34
