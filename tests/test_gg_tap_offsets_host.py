"""Host check of the gather GEMM's tap-offset rules (csrc/gg_tap_rules.h): tests/gg_tap_offsets_host.cc, a stand-alone program,
walks the kernel's loader state over every (row, tap) of small layers and compares the per-tile (base, mask) + scalar delta rule
with the reference formula.  Built twice with the host compiler -- plain, and with AddressSanitizer and UBSan linked into the
program itself -- and run as an ordinary process.  No GPU."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "gg_tap_offsets_host.cc"


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    pytest.fail("no host C++ compiler (g++ / c++ / clang++) on PATH")


SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


@pytest.mark.parametrize("flags", [("-O2",), SANITIZE], ids=["plain", "asan-ubsan"])
def test_tap_state_rule_gives_the_reference_offsets(flags, tmp_path):
    exe = tmp_path / "gg_tap_offsets_host"
    cxx = _compiler()
    if flags is SANITIZE and "clang" not in cxx:
        # the sanitizer runtimes inside the program (clang's default): it then runs the same under any loader environment
        flags = flags + ("-static-libasan", "-static-libubsan")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, str(SRC), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    assert " 0 mismatches" in r.stdout


def test_kernel_and_plan_use_the_header():
    csrc = ROOT / "shallow-ntc_amd" / "csrc"
    kernel = (csrc / "gather_gemm_kernel.h").read_text()
    assert '#include "gg_tap_rules.h"' in kernel and "gg_tap_offset(a_base[i], a_mask[i], ld_delta, ld_sel)" in kernel
    plan = (csrc / "conv_plan.hip").read_text()
    assert "kTapGridMax" in plan                      # a tap grid beyond the masks is rejected when the plan is built
    assert "gg_tap_rules.h" in (csrc / "Makefile").read_text()
