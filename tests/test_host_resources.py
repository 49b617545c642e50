"""The host-side owners of device memory against a fake HIP runtime (tests/host/fake_hip_runtime.hpp): stand-alone programs built
with AddressSanitizer and UndefinedBehaviorSanitizer and not linked against the HIP runtime.  No GPU.

resources_main.cpp: the owner types of csrc/af_hip_resources.hpp.  suppressor_host_main.cpp: SuppressorHost
(csrc/af_suppressor_host.hpp) -- its workspace, state and upload with every allocation failed in turn, its buffer-set accessor,
and the pure host builder of the weight and table blob."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/llvm/bin/clang++"


def _build_and_run(tmp_path, name, expect):
    exe = str(tmp_path / name)
    build = subprocess.run(
        [CLANG, "-std=c++17", "-g", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
         "-I" + os.path.join(ROOT, "audio-forge_amd", "csrc"), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert expect in run.stdout


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the ROCm clang++ is not installed")
def test_owner_types_against_a_fake_runtime(tmp_path):
    _build_and_run(tmp_path, "resources_main", "resources: ok")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="the ROCm clang++ is not installed")
def test_suppressor_host_against_a_fake_runtime(tmp_path):
    _build_and_run(tmp_path, "suppressor_host_main", "suppressor host: ok")
