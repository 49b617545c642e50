"""The canonical limiter ring of csrc/af_stream_state.h -- what an export stores and how an import re-phases it -- against a
brute-force model of the chain kernels' ring / suffix / prefix update: tests/host/stream_state_main.cpp, a stand-alone host
program built with AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU, no HIP runtime."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the ROCm clang++ is not installed")
def test_rephased_ring_continues_bit_for_bit(tmp_path):
    exe = str(tmp_path / "stream_state_main")
    build = subprocess.run(
        [CLANG, "-std=c++17", "-g", "-O1", "-Wall", "-I" + os.path.join(ROOT, "audio-forge_amd", "csrc"),
         "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         os.path.join(ROOT, "tests", "host", "stream_state_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "stream_state: ok" in run.stdout
