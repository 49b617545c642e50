"""The owner types of csrc/af_hip_resources.hpp against a fake HIP runtime: tests/host/resources_main.cpp, a stand-alone
program built with AddressSanitizer and UndefinedBehaviorSanitizer and not linked against the HIP runtime.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the ROCm clang++ is not installed")
def test_owner_types_against_a_fake_runtime(tmp_path):
    exe = str(tmp_path / "resources_main")
    build = subprocess.run(
        [CLANG, "-std=c++17", "-g", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
         "-I" + os.path.join(ROOT, "audio-forge_amd", "csrc"), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         os.path.join(ROOT, "tests", "host", "resources_main.cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "resources: ok" in run.stdout
