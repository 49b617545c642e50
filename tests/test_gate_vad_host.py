"""Host surface of the VAD-fused gate modes (no GPU): symbols, defaults, clamps, refusals, and the new kernels' resources
from the compiler's remarks."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
CSRC = ROOT / "audio-forge_amd" / "csrc"
NEW = ("af_gate_set_vad_auto_gate_enabled", "af_gate_set_vad_threshold", "af_gate_set_hold_time", "af_gate_set_margin",
       "af_gate_set_auto_threshold", "af_gate_read_vad_controls", "af_gate_set_vad_evidence", "af_engine_read_gate_vad_state",
       "af_engine_read_gate_vad_decisions")


@pytest.fixture(scope="module")
def core():
    from mic_eq_mi import mic_eq_core

    return mic_eq_core


def test_symbols_in_header_library_and_signatures():
    from mic_eq_mi import _lib

    header = (ROOT / "include" / "audioforge_mi.h").read_text()
    lib = C.CDLL(str(ROOT / "audio-forge_amd" / "libaudioforge_mi.so"))
    for name in NEW:
        assert re.search(rf"\b{name}\(", header), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_defaults(core):
    eng = core.Engine(48_000.0, 5)
    c = eng.gate_vad_controls()
    assert c == {"vad_threshold": pytest.approx(0.48), "hold_ms": 200.0, "margin_db": 10.0, "auto_threshold": True, "attached": False}
    st = eng.gate_vad_state()
    assert (st["noise_floor_db"] == np.float32(-60.0)).all() and (st["noise_floor_reliability"] == 0).all()
    assert (st["gate_state"] == 0).all() and not st["held_open"].any() and not st["fused_open"].any()
    assert (st["fused_score"] == 0).all() and (st["probability"] == 0).all()
    eng.close()


def test_clamps_and_non_finite_values(core):
    eng = core.Engine(48_000.0, 2)
    for setter, key, lo, hi, inside in (("gate_set_vad_threshold", "vad_threshold", 0.0, 1.0, 0.25),
                                        ("gate_set_hold_time", "hold_ms", 0.0, 500.0, 120.0),
                                        ("gate_set_margin", "margin_db", 0.0, 20.0, 6.5)):
        getattr(eng, setter)(inside)
        assert eng.gate_vad_controls()[key] == pytest.approx(inside)
        getattr(eng, setter)(hi + 7.0)
        assert eng.gate_vad_controls()[key] == hi
        getattr(eng, setter)(lo - 7.0)
        assert eng.gate_vad_controls()[key] == lo
        getattr(eng, setter)(inside)
        for bad in (float("nan"), float("inf"), float("-inf")):
            getattr(eng, setter)(bad)
            assert eng.gate_vad_controls()[key] == pytest.approx(inside), (setter, bad)
    eng.gate_set_auto_threshold(0)
    eng.gate_set_vad_auto_gate_enabled(1)
    c = eng.gate_vad_controls()
    assert c["attached"] and not c["auto_threshold"]
    eng.gate_set_vad_auto_gate_enabled(0)
    assert not eng.gate_vad_controls()["attached"]
    with pytest.raises(ValueError):
        eng.gate_set_vad_evidence(np.zeros((3, 5), np.float32))
    eng.close()


def test_bad_evidence_arguments_are_refused(core):
    from mic_eq_mi import _lib

    eng = core.Engine(48_000.0, 2)
    p = np.zeros(4, np.float32)
    # (the refusal of a block count that does not fit the call, with the pending input unchanged, needs a process call and
    # hence a device: tests/test_gpu_gate_vad.py::test_evidence_of_the_wrong_length_is_refused_before_anything_is_touched)
    assert eng._lib.af_gate_set_vad_evidence(eng._h, p.ctypes.data_as(C.POINTER(C.c_float)), None, 4, 0) != 0
    assert eng._lib.af_gate_set_vad_evidence(eng._h, None, None, 4, 0) != 0
    assert eng._lib.af_gate_set_vad_evidence(eng._h, None, None, -1, 0) != 0
    assert eng._lib.af_gate_set_vad_evidence(eng._h, None, None, 0, 0) == 0
    eng.close()


def _resource_remarks():
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-x", "hip",
           "--cuda-device-only", "-c", "af_prepass.hip", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    text = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True, check=True).stderr
    res, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            res[name] = {}
        for key in ("ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "VGPRs"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                res[name][key] = int(m.group(1))
    return res


def test_new_kernels_resources():
    """Scratch-free, and a bounded LDS request.  The control pass's tiles are static and show in the remarks; the per-sample
    pass's request is dynamic (kVadGateLds), which the remarks do not show: a static_assert beside it holds it to one CU's
    160 KiB, so a build that exists has passed it."""
    res = _resource_remarks()
    per_sample = {n: r for n, r in res.items() if n.startswith("_ZN2af23vad_gate_prepass_kernel")}
    control = {n: r for n, r in res.items() if n.startswith("_ZN2af23vad_gate_control_kernel")}
    init = {n: r for n, r in res.items() if n.startswith("_ZN2af21vad_plane_init_kernel")}
    assert len(per_sample) == 3 and len(control) == 1 and len(init) == 1, (list(per_sample), list(control), list(init))
    for name, r in {**per_sample, **control, **init}.items():
        assert r["ScratchSize [bytes/lane]"] == 0, (name, r)
    assert 0 < next(iter(control.values()))["LDS Size [bytes/block]"] <= 64 * 1024
    for r in per_sample.values():
        assert r["LDS Size [bytes/block]"] == 0, r  # nothing static on top of the dynamic request
    # the gated pre-pass of the expander path is still the three instantiations it was
    assert len([n for n in res if n.startswith("_ZN2af26supp_prefilter_gate_kernel")]) == 3
