"""The execution forms of round 3 against the forms they replaced, bit for bit (audio and block rows): one chain launch per
call following a ready counter (behind the suppressor; behind the systolic EQ when the suppressor is off), the lane-per-stream
EQ kernel, against one chain launch per window with the systolic EQ, and against the EQ inside the chain kernel.  The switches
are read once per process, so every variant is a short child process of `tools/ab_fullchain.py` (70 streams, 2.3 s, two calls,
a coefficient crossfade opening the stream); the parity of the default forms with the oracle is what every other GPU test checks.
The tool pins the chain kernel (at 70 streams AUTO runs the stage pipeline, where all three variants would be the same form),
and each run's kernel id and launch counts are asserted: the comparison is between the forms it names."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "ab_fullchain.py")


def _run(out: str, tag: str, mode: str, **env: str) -> None:
    child_env = dict(os.environ, AB_MODE=mode, AB_OUT_DIR=out, **env)
    done = subprocess.run([sys.executable, TOOL, tag], env=child_env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]


def _forms(out: str, tag: str):
    with np.load(os.path.join(out, f"abfc_{tag}.npz")) as z:
        return z["kernel"].tolist(), z["chain_launches"].tolist(), z["launches"].tolist()


CALLS = (130 * 480, 100 * 480)  # the tool's two calls
KERNEL_PHASED = 2


def _same(out: str, a: str, b: str) -> None:
    done = subprocess.run([sys.executable, TOOL, "cmp", a, b], env=dict(os.environ, AB_OUT_DIR=out), capture_output=True,
                          text=True, timeout=120)
    assert done.returncode == 0, done.stdout + done.stderr[-1000:]


@pytest.mark.parametrize("mode", ["full", "full+automakeup", "dynamics", "dynamics+automakeup", "full+steep"])
def test_one_launch_forms_equal_the_per_window_forms(mode, tmp_path):
    out = str(tmp_path)
    tag = mode.replace("+", "_")
    tags = [f"t_{tag}_default", f"t_{tag}_per_window", f"t_{tag}_eq_in_chain"]
    try:
        _run(out, tags[0], mode)
        kernel, chain, launches = _forms(out, tags[0])
        assert kernel == [KERNEL_PHASED] * 2 and chain == [1, 1], (kernel, chain)  # one chain launch per call
        if not mode.startswith("full"):
            # the no-suppressor one-launch branch (the EQ kernel per 9600-sample window + its counter publish + the chain launch;
            # with auto-makeup that branch's EQ kernel also leaves the block powers the chain launch reads)
            assert launches == [1 + 2 * math.ceil(n / 9600) for n in CALLS], launches
        _run(out, tags[1], mode, AF_CHAIN_PERSISTENT="0", AF_EQ_STREAM="0")
        kernel, chain, launches = _forms(out, tags[1])
        assert kernel == [KERNEL_PHASED] * 2, kernel
        if mode.startswith("full"):
            assert min(chain) > 1, chain  # one chain launch per suppressor window
        else:
            # the EQ inside the call's chain launch (auto-makeup: behind its pre-pass, and the rows merged): no EQ windows
            assert max(launches) <= 3, launches
        _same(out, tags[0], tags[1])
        if mode.startswith("full"):
            _run(out, tags[2], mode, AF_EQ_OFFLOAD="0")
            kernel, chain, _ = _forms(out, tags[2])
            assert kernel == [KERNEL_PHASED] * 2 and min(chain) > 1, (kernel, chain)
            _same(out, tags[0], tags[2])
    finally:  # (26 MB each)
        for t in tags:
            path = os.path.join(out, f"abfc_{t}.npz")
            if os.path.exists(path):
                os.remove(path)


def test_serial_streams_create_run_and_exit_cleanly(tmp_path):
    """AF_SERIAL_STREAMS: the engine's side streams alias the caller's and must not be destroyed with the engine.  One engine is
    created, runs one call (64 streams, suppressor on) and is closed in a child process (tests/switch_child.py), which must
    exit with status 0 and return what the same call returns here, without the switch."""
    import switch_child

    out = str(tmp_path / "serial.npz")
    done = subprocess.run([sys.executable, switch_child.__file__, "full_chain_one_call", out], env=dict(os.environ, AF_SERIAL_STREAMS="1"),
                          capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, (done.returncode, done.stderr[-2000:])
    want = switch_child.full_chain_one_call()
    with np.load(out) as z:
        assert z["y"].shape == want["y"].shape
        assert np.array_equal(z["y"].view(np.uint32), want["y"].view(np.uint32)), f"max abs {np.abs(z['y'] - want['y']).max():.3e}"
        assert z["rows"].tobytes() == want["rows"].tobytes()
