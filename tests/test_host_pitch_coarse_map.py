"""The index map of the pitch search's coarse correlation (csrc/af_pitch_coarse_map.h) enumerated over all 64 steps x 64 lanes:
tests/host/pitch_coarse_map_main.cpp, a stand-alone host program built with AddressSanitizer and UndefinedBehaviorSanitizer.
Every (lag, j) product once and in order, every operand word inside its array, guard words exactly outside the frame, no two
different words of a step in one bank.  No GPU, no HIP runtime."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the ROCm clang++ is not installed")
def test_coarse_map_covers_every_product_once_inside_its_arrays(tmp_path):
    exe = str(tmp_path / "pitch_coarse_map_main")
    build = subprocess.run(
        [CLANG, "-std=c++17", "-g", "-O1", "-Wall", "-I" + os.path.join(ROOT, "audio-forge_amd", "csrc"),
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         os.path.join(ROOT, "tests", "host", "pitch_coarse_map_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "pitch_coarse_map: ok" in run.stdout
