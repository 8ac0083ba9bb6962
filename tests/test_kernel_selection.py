"""The dispatch of csrc/hadi_dispatch.h -- which kernel runs a pass, with which grid, block and dynamic LDS, and how
hadi_describe_last_sweep words it -- against tests/golden/kernel_selection.json: the choices of the hand-written launchers and
description this header replaced, recorded from them over every kernel family (tests/golden/README.md).  The selectors are
reached through the wave emulator's driver, which runs its solves through the same functions."""
import ctypes as C
import json
import os
import re

import pytest

from test_emu_kernel_logic import emu  # noqa: F401  (the fixture that builds tests/emu/libhadi_emu.so)

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = json.load(open(os.path.join(HERE, "golden", "kernel_selection.json")))

# Entries of the table of instantiations that no pass selector returns: launched by run_sweep through their own functions
# (hadi_select_pair_table, hadi_select_resident, hadi_select_small).  The two team kernels have their own argument block and
# are not in the table (hadi_for_each_kernel visits them behind it).
OUTSIDE = {"hadi_pass_a_strip<8, 0, double, 2, 3>", "hadi_sweep_resident<8>",
           "hadi_small_kernel<1, 4, false>", "hadi_small_kernel<1, 4, true>", "hadi_small_kernel<2, 4, false>",
           "hadi_small_kernel<2, 4, true>", "hadi_small_kernel<1, 8, false>", "hadi_small_kernel<1, 8, true>",
           "hadi_small_kernel<2, 8, false>", "hadi_small_kernel<2, 8, true>", "hadi_small_seq_kernel<1>",
           "hadi_small_seq_kernel<2>", "hadi_small_seq2_kernel<1>", "hadi_small_seq2_kernel<2>"}
FAMILY = ["hadi_pass_a", "hadi_pass_a_sch", "hadi_pass_a_strip", "hadi_pass_a_strip_sch", "hadi_pass_a_pairs", "hadi_pass_a_seq",
          "hadi_pass_b", "hadi_pass_b1", "hadi_pass_b2", "hadi_pass_b_seq"]
TAG = ["EU", "AM", "AM-P"]
SCH = {1: "CS", 2: "MCS", 3: "HV"}


def _select(emu, case_in, mode, what):
    """(rc, table index and template values, name, grid, block, LDS bytes, description) of one pass of a fixture case."""
    m1, m2, n, strip, pairs, nos, american, amp, xstep, f32, scheme, cs_strips, cp = case_in
    arr = (C.c_int * 16)(m1, m2, n, FIX["target_waves"], strip, pairs, nos, american, amp, xstep, f32, scheme, cs_strips, cp, mode, what)
    o = (C.c_longlong * 11)()
    name, desc = C.create_string_buffer(512), C.create_string_buffer(512)
    rc = emu.emu_select(arr, o, name, desc, 512)
    return rc, list(o), name.value.decode(), desc.value.decode()


def _table(emu):
    arr = (C.c_int * 16)(*([0] * 15 + [2]))
    o = (C.c_longlong * 11)()
    name, desc = C.create_string_buffer(512), C.create_string_buffer(512)
    out = []
    for i in range(emu.emu_select(arr, o, name, desc, 512)):
        arr[0] = i
        emu.emu_select(arr, o, name, desc, 512)
        assert o[0] == i
        out.append(name.value.decode())
    return out


@pytest.fixture(scope="module")
def selected(emu):  # noqa: F811
    """Every pass of every fixture case through the selector, once: [(case, [(recorded pass, selected pass)], description)]."""
    out = []
    for c in FIX["cases"]:
        passes = [(r[1:], _select(emu, c["in"], r[0], 0)) for r in c["row"]] + [(c["col"], _select(emu, c["in"], 0, 1))]
        out.append((c, passes))
    return out


def test_fixture_covers_the_domain():
    assert FIX["target_waves"] == 8 * 256 and len(FIX["cases"]) >= 600
    assert os.path.getsize(os.path.join(HERE, "golden", "kernel_selection.json")) <= 256 * 1024


def test_every_case_reproduces(selected):
    """(a) kernel, grid, block, dynamic LDS bytes and the description, exactly."""
    for c, passes in selected:
        for want, (rc, o, name, desc) in passes:
            assert rc == 0, c
            assert [name, o[8], o[9], o[10]] == want, (c["in"], want, name, o)
            assert desc == c["desc"], (c["in"], desc)


def test_every_instantiation_is_selected_somewhere(emu, selected):  # noqa: F811
    """(b) every entry of the table of instantiations is returned for at least one case, but for the ones launched outside the
    pass selectors -- and those are in the table."""
    table = _table(emu)
    assert len(set(table)) == len(table)
    assert OUTSIDE <= set(table), OUTSIDE - set(table)
    hit = {o[0] for _, passes in selected for _, (_, o, _, _) in passes}
    missed = {table[i] for i in range(len(table)) if i not in hit}
    assert missed == OUTSIDE, (sorted(missed - OUTSIDE), sorted(OUTSIDE - missed))


def _named(text):
    """'hadi_pass_a_strip<8,EU,double,2>' -> (family, [template values])."""
    m = re.fullmatch(r"(\w+)<([^>]*)>", text)
    assert m, text
    return m.group(1), m.group(2).split(",")


def test_the_description_names_the_selected_kernel(selected):
    """(c) the kernel the description names for the row pass (the Douglas step, or the corrector of a predictor-corrector
    scheme with `cs_strips` 0 / 1) and for the column pass is the kernel selected: family, nodes per lane or chunk capacity,
    variant, state type, wavefronts per row and scheme, wherever the name spells them."""
    for c, passes in selected:
        cs_strips, scheme = c["in"][11], c["in"][10]
        m = re.fullmatch(r"row pass (\S+) \(.*\); column pass (\S+) \(.*\)", c["desc"])
        assert m, c["desc"]
        # (an explicit (U, lambda_bar) step of the P representation runs the plain American kernels: the text is about the others)
        if c["in"][8]:
            continue
        checks = [(m.group(2), passes[-1][1][1])]
        if not (scheme and cs_strips in (2, 3)):  # (diagnostics: worded as `cs_strips` = 1, see hadi_describe_passes)
            checks.append((m.group(1), passes[-2][1][1]))
        for text, o in checks:
            fam, args = _named(text)
            _, family, B, G, amer, mode, sch, f32 = o[:8]
            assert fam == FAMILY[family], (c["in"], text, o)
            assert TAG[amer] in args, (c["in"], text, o)
            if fam in ("hadi_pass_a", "hadi_pass_a_sch"):
                assert args[:2] == [str(B), str(G)] and (("float" in args) == bool(f32)), (c["in"], text, o)
            if fam in ("hadi_pass_a_strip", "hadi_pass_a_strip_sch"):
                assert args[0] == str(B) and (("float" in args) == bool(f32)), (c["in"], text, o)
                assert (len(args) > 3 and args[3] == "2") == (G == 2), (c["in"], text, o)
            if fam in ("hadi_pass_b", "hadi_pass_b1", "hadi_pass_b2"):
                assert args[0] == str(B), (c["in"], text, o)
            if mode:
                assert args[-1] == SCH[sch], (c["in"], text, o)
            else:
                assert args[-1] not in SCH.values(), (c["in"], text, o)
