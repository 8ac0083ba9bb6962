"""CPU-only: tests/cpp/jump_substep_san.cpp -- the emulated Bates sub-step over every shape of tests/jump_cases.py, and the stage of
the whole-loop kernel (hadi_small_jump_stage) over every shape of tests/bates_domain_cases.py, as a stand-alone program -- built with -fsanitize=address,undefined and run as a program: nothing is loaded into Python and nothing is preloaded (the two runtimes are
linked into the program).
The emulator's scheduler (lanes as fibers on mmap'ed stacks) runs under AddressSanitizer as it is.  Any report of either sanitizer
ends the program with a non-zero status (-fno-sanitize-recover); each launch is also held to the isolation rule in long double."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pde_based_heston_solver_gpu_accelerated_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "emu")
SRC = os.path.join(ROOT, "tests", "cpp", "jump_substep_san.cpp")
EXE = os.path.join(ROOT, "tests", "cpp", "jump_substep_san")


def _build():
    srcs = [SRC, os.path.join(EMU, "emu_jump_substep.cpp"), os.path.join(EMU, "emu_small_jump_stage.cpp"), os.path.join(EMU, "wave_emu.h")] +[os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    if not os.path.exists(EXE) or any(os.path.getmtime(s) > os.path.getmtime(EXE) for s in srcs):
        tmp = "%s.tmp.%d" % (EXE, os.getpid())
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-D_GLIBCXX_ASSERTIONS", "-pthread", "-DHADI_EMU", "-I" + EMU, "-I" + CSRC,
                               "-o", tmp, SRC])
        os.replace(tmp, EXE)
    return EXE


def test_cpp_jump_substep_under_the_sanitizers():
    out = subprocess.run([_build()], capture_output=True, text=True, timeout=900)
    print(out.stdout[-6000:], out.stderr[-4000:])
    assert out.returncode == 0 and "all sub-step shapes passed" in out.stdout
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
