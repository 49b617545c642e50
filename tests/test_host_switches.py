"""The run-time switch table and the suppressor window schedule of csrc/af_switches.hpp: tests/host/switches_main.cpp, a
stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer.  No HIP runtime, no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the ROCm clang++ is not installed")
def test_switch_table_and_window_schedule(tmp_path):
    exe = str(tmp_path / "switches_main")
    build = subprocess.run(
        [CLANG, "-std=c++17", "-g", "-O1", "-Wall", "-I" + os.path.join(ROOT, "audio-forge_amd", "csrc"),
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         os.path.join(ROOT, "tests", "host", "switches_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "switches: ok" in run.stdout
