"""Build-time checks of the resident sweep kernel (hadi_sweep_resident<8>) from the compiler's own assembly (no GPU): no
scratch at all -- a spill reload inside the time loop would sit in the row loop's counted-wait window -- and exactly the LDS-DMA
pieces, and at least the stores, that the counted waits of the row phase assume (the rules of tests/test_isa_counts.py for
hadi_pass_a_strip<8,EU>, whose body the row phase is)."""
import os, re, subprocess, sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def resident():
    import kernel_regs
    rows, asm = kernel_regs.collect()
    found = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        if name.startswith("void hadi_sweep_resident<") or name.startswith("void hadi_pass_a_strip<8, 0, double, 1, 0>"):
            found[name.split("(")[0].replace("void ", "")] = m.group(2)
    regs = {r[0].split("(")[0].replace("void ", ""): r for r in rows}
    meta = [b for b in asm.split("- .agpr_count:")[1:] if re.search(r"\.name:\s+_Z19hadi_sweep_resident", b)]
    found["__meta__"] = meta[0] if meta else ""
    return found, regs


def test_no_scratch_and_no_spills(resident):
    found, regs = resident
    body = found["hadi_sweep_resident<8>"]
    assert not re.search(r"\bscratch_(load|store)", body)
    _, vgpr, sgpr, spill, scratch, _ = regs["hadi_sweep_resident<8>"]
    assert spill == 0 and scratch == 0, regs["hadi_sweep_resident<8>"]
    assert vgpr <= 256


def test_dma_pieces_and_stores_match_the_strip_kernel(resident):
    """5 fetch sites (the strip's first row and the rows 1 .. 3 ahead in the prologue, one in the loop) x 5 DMA pieces of a
    528-double row; two copies of hadi_strip_step (last v-row or not), 4 row stores each.  The same counts as the streaming
    strip kernel compiled from the same body."""
    found, _ = resident
    body, strip = found["hadi_sweep_resident<8>"], found["hadi_pass_a_strip<8, 0, double, 1, 0>"]
    n_dma = len(re.findall(r"\bglobal_load_lds_dwordx4\b", body))
    assert n_dma == 5 * 5 == len(re.findall(r"\bglobal_load_lds_dwordx4\b", strip)), n_dma
    n_st = len(re.findall(r"\bglobal_store_dwordx4\b", body))
    assert n_st >= 2 * 4, n_st


def test_argument_block_is_at_kernarg_offset_0(resident):
    """hadi_resident_args() re-reads the argument block from offset 0 of the kernarg segment: the first parameter must be the
    whole HadiSweepArgs (224 bytes, static_assert in hadi_k_common.h) at offset 0."""
    found, _ = resident
    args = re.search(r"\.args:\s*\n\s*- \.offset:\s+(\d+)\s*\n\s*\.size:\s+(\d+)\s*\n\s*\.value_kind:\s+(\w+)", found["__meta__"])
    assert args and args.groups() == ("0", "224", "by_value"), args and args.groups()
