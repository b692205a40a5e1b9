"""Host check of the gather GEMMs' piece walk (csrc/gg_pieces.h, Part A): tests/gg_pieces_host.cc, a stand-alone program, walks
every worker of small stream-K launches and every block of static ones through the functions the kernels run, and checks coverage,
the hand-off partners (the no-deadlock argument) and the static map.  Built twice with the host compiler -- plain, and with
AddressSanitizer and UBSan linked into the program itself -- and run as an ordinary process.  No GPU."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "gg_pieces_host.cc"


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    pytest.fail("no host C++ compiler (g++ / c++ / clang++) on PATH")


SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


@pytest.mark.parametrize("flags", [("-O2",), SANITIZE], ids=["plain", "asan-ubsan"])
def test_piece_walk_covers_every_unit_and_cannot_deadlock(flags, tmp_path):
    exe = tmp_path / "gg_pieces_host"
    cxx = _compiler()
    if flags is SANITIZE and "clang" not in cxx:
        # the sanitizer runtimes inside the program (clang's default): it then runs the same under any loader environment
        flags = flags + ("-static-libasan", "-static-libubsan")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", *flags, str(SRC), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    assert " 0 mismatches" in r.stdout
    walked = re.search(r"walked (\d+) geometries", r.stdout)
    assert walked and int(walked.group(1)) > 0


def test_both_kernels_use_the_header():
    csrc = ROOT / "shallow-ntc_amd" / "csrc"
    for name in ("gather_gemm_kernel.h", "bf3_gemm.hip"):
        text = (csrc / name).read_text()
        assert '#include "gg_pieces.h"' in text, name
        assert "PieceWalk<" in text and "static_piece(" in text and "sk_consume<" in text and "sk_publish<" in text, name
        # neither kernel keeps a walk of its own
        assert not re.search(r"\b(next_piece|locate|tile_of)\s*=\s*\[", text), name
        assert not re.search(r"\b(void|bool|auto)\s+(next_piece|locate|tile_of)\s*\(", text), name
        assert "struct Piece" not in text and "sk_phase" not in text, name
    assert "gg_pieces.h" in (csrc / "Makefile").read_text()
