"""The noise gate stage's interface without a GPU: symbols, defaults, clamping of the live controls, the mode check, and the
gated pre-pass kernel's resources on gfx950 (no scratch; its dynamic LDS request is bounded by a static_assert in the
source)."""
import os
import pathlib
import re
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "audioforge_mi.h"
CSRC = ROOT / "audio-forge_amd" / "csrc"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NEW = ["af_engine_set_gate_enabled", "af_gate_set_threshold", "af_gate_set_attack_time", "af_gate_set_release_time",
       "af_gate_set_mode", "af_gate_threshold_db", "af_engine_gate_enabled", "af_engine_read_gate_state"]


def test_symbols_in_header_library_and_signatures():
    from mic_eq_mi import _lib

    text = HEADER.read_text()
    lib = _lib.load()
    for name in NEW:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert {"af_gate_threshold_db", "af_engine_gate_enabled"} <= _lib.VALUE_FUNCTIONS


@pytest.fixture()
def engine():
    from mic_eq_mi import mic_eq_core as core

    eng = core.Engine(48_000.0, 3)  # no process call: nothing touches a device
    yield eng
    eng.close()


def test_defaults(engine):
    assert engine.engine_gate_enabled() == 0
    assert engine.gate_threshold_db() == -40.0
    st = engine.gate_state()
    assert st["current_gain"].tolist() == [0.0, 0.0, 0.0]
    assert st["chatter_events"].tolist() == [0, 0, 0]
    assert not st["is_open"].any() and not st["auto_relax_active"].any()


def test_enable_toggles(engine):
    engine.set_gate_enabled(1)
    assert engine.engine_gate_enabled() == 1
    engine.set_gate_enabled(0)
    assert engine.engine_gate_enabled() == 0


@pytest.mark.parametrize("value,want", [(-90.0, -80.0), (-5.0, -10.0), (-33.5, -33.5), (float("nan"), -40.0),
                                        (float("inf"), -40.0), (float("-inf"), -40.0)])
def test_threshold_clamps_or_ignores(engine, value, want):
    engine.gate_set_threshold(value)
    assert engine.gate_threshold_db() == want


def test_time_controls_accept_non_finite_and_out_of_range(engine):
    for v in (0.0, 1e9, float("nan"), -1.0):
        engine.gate_set_attack_time(v)
        engine.gate_set_release_time(v)
    engine.gate_set_threshold(-20.0)  # setters stay live: no AF_ERR_STATE
    assert engine.gate_threshold_db() == -20.0


def test_invalid_mode_raises(engine):
    for mode in (0, 1, 2):
        engine.gate_set_mode(mode)
    with pytest.raises(ValueError, match="Invalid gate mode"):
        engine.gate_set_mode(3)
    with pytest.raises(ValueError, match="Invalid gate mode"):
        engine.gate_set_mode(-1)


def test_read_gate_state_accepts_null_pointers(engine):
    from mic_eq_mi import _lib

    assert engine._lib.af_engine_read_gate_state(engine._h, None, None, None, 3) == _lib.AF_OK
    assert engine._lib.af_engine_read_gate_state(engine._h, None, None, None, 4) == _lib.AF_ERR_INVALID_ARGUMENT


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_gated_prepass_resources(tmp_path):
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-x", "hip",
                          str(CSRC / "af_prepass.hip"), "-S", "--cuda-device-only", "-o", str(tmp_path / "rn.s"),
                          "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=CSRC, check=True)
    blocks = re.split(r"remark: Function Name: ", res.stderr)
    gate = [b for b in blocks if b.startswith("_ZN2af26supp_prefilter_gate_kernel")]
    assert len(gate) == 3, "expected the kernel with and without the suppressor's roles (and the raw protocol)"
    for b in gate:
        assert int(re.search(r"ScratchSize \[bytes/lane\]: (\d+)", b).group(1)) == 0, b[:80]
