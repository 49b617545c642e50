"""Argument contract of the input mixdown's entry points (include/audioforge_mi.h, "input mixdown" and "multichannel input
of an engine") and of the Python classes on them.  Everything here is refused or answered on the host: no device is used."""
import ctypes as C

import numpy as np
import pytest

from mic_eq_mi import _lib
from mic_eq_mi import mic_eq_core as core


@pytest.fixture(scope="module")
def L():
    return _lib.load()


def _create(L, channels, mode, streams, device=0):
    h = C.c_void_p()
    rc = L.af_mixdown_create(channels, mode, streams, device, C.byref(h))
    return rc, h, _lib.last_error() if rc else ""


@pytest.mark.parametrize("args, code, message", [
    ((0, 0, 4), _lib.AF_ERR_INVALID_ARGUMENT, "n_channels must be >= 1"),
    ((-2, 0, 4), _lib.AF_ERR_INVALID_ARGUMENT, "n_channels must be >= 1"),
    ((9, 0, 4), _lib.AF_ERR_UNSUPPORTED, "at most 8"),
    ((64, 4, 4), _lib.AF_ERR_UNSUPPORTED, "64 input channels"),
    ((2, 5, 4), _lib.AF_ERR_INVALID_ARGUMENT, "unknown input channel mode 5"),
    ((2, -1, 4), _lib.AF_ERR_INVALID_ARGUMENT, "unknown input channel mode -1"),
    ((2, 4, 0), _lib.AF_ERR_INVALID_ARGUMENT, "n_streams must be positive"),
    ((2, 4, 4, -1), _lib.AF_ERR_INVALID_ARGUMENT, "device"),
])
def test_create_refuses_bad_arguments(L, args, code, message):
    rc, h, err = _create(L, *args)
    assert rc == code and message in err and not h.value


def test_create_needs_an_out_pointer(L):
    assert L.af_mixdown_create(2, 0, 1, 0, None) == _lib.AF_ERR_INVALID_ARGUMENT


def test_create_accepts_one_to_eight_channels_and_every_mode(L):
    for channels in range(1, 9):
        for mode in range(5):
            rc, h, _ = _create(L, channels, mode, 3)
            assert rc == _lib.AF_OK and h.value
            assert L.af_mixdown_channels(h) == channels and L.af_mixdown_mode(h) == mode
            L.af_mixdown_destroy(h)


def test_set_mode_is_live_and_refuses_unknown_values(L):
    rc, h, _ = _create(L, 2, 0, 2)
    assert rc == _lib.AF_OK
    for mode in (4, 3, 2, 1, 0):
        assert L.af_mixdown_set_mode(h, mode) == _lib.AF_OK and L.af_mixdown_mode(h) == mode
    for bad in (5, -1, 255):
        assert L.af_mixdown_set_mode(h, bad) == _lib.AF_ERR_INVALID_ARGUMENT
        assert f"unknown input channel mode {bad}" in _lib.last_error()
        assert L.af_mixdown_mode(h) == 0  # unchanged
    assert L.af_mixdown_set_mode(None, 0) == _lib.AF_ERR_INVALID_ARGUMENT and "mixdown is null" in _lib.last_error()
    L.af_mixdown_destroy(h)


def test_push_argument_checks_come_before_any_device_work(L):
    rc, h, _ = _create(L, 2, 4, 2)
    x = np.zeros((2, 8, 2), dtype=np.float32)
    y = np.zeros((2, 8), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    xp, yp = x.ctypes.data_as(fp), y.ctypes.data_as(fp)
    assert L.af_mixdown_push_host(None, xp, 8, 8, yp, 8) == _lib.AF_ERR_INVALID_ARGUMENT
    assert L.af_mixdown_push_host(h, xp, -1, 8, yp, 8) == _lib.AF_ERR_INVALID_ARGUMENT
    assert L.af_mixdown_push_host(h, xp, 8, 7, yp, 8) == _lib.AF_ERR_INVALID_ARGUMENT and "in_stride" in _lib.last_error()
    assert L.af_mixdown_push_host(h, xp, 8, 8, yp, 7) == _lib.AF_ERR_INVALID_ARGUMENT and "out_stride" in _lib.last_error()
    assert L.af_mixdown_push_host(h, None, 8, 8, yp, 8) == _lib.AF_ERR_INVALID_ARGUMENT and "null buffer" in _lib.last_error()
    assert L.af_mixdown_push_device(h, None, 8, 8, None, 8, None) == _lib.AF_ERR_INVALID_ARGUMENT
    x[1, 3, 1] = np.inf
    assert L.af_mixdown_push_host(h, xp, 8, 8, yp, 8) == _lib.AF_ERR_NON_FINITE and _lib.last_error() == "samples must be finite"
    assert L.af_mixdown_push_host(h, xp, 0, 0, yp, 0) == _lib.AF_OK  # an empty callback is nothing
    # before a first push the diagnostics are the fresh ones, answered from the host
    corr = np.zeros(2, dtype=np.float32)
    warn = np.ones(2, dtype=np.uint64)
    strat = np.ones(2, dtype=np.int32)
    assert L.af_mixdown_read_diagnostics(h, corr.ctypes.data_as(fp), warn.ctypes.data_as(C.POINTER(C.c_uint64)),
                                         strat.ctypes.data_as(C.POINTER(C.c_int32)), None, None, 2) == _lib.AF_OK
    assert np.isnan(corr).all() and not warn.any() and not strat.any()
    assert L.af_mixdown_read_diagnostics(h, None, None, None, None, None, 3) == _lib.AF_ERR_INVALID_ARGUMENT
    a, b = C.c_double(1.0), C.c_double(1.0)
    assert L.af_mixdown_last_kernel_ms(h, C.byref(a), C.byref(b)) == _lib.AF_OK and (a.value, b.value) == (0.0, 0.0)
    assert L.af_mixdown_reset(h) == _lib.AF_OK and L.af_mixdown_reset(None) == _lib.AF_ERR_INVALID_ARGUMENT
    L.af_mixdown_destroy(h)
    L.af_mixdown_destroy(None)


def test_python_mixdown_argument_checks():
    with pytest.raises(ValueError, match="unknown input channel mode 'stereo'"):
        core.Mixdown(2, "stereo")
    with pytest.raises(ValueError, match="unknown input channel mode"):
        core.Mixdown(2, 7)
    with pytest.raises(ValueError, match="unknown input channel mode"):
        core.Mixdown(2, 1.0)
    with pytest.raises(NotImplementedError, match="at most 8"):
        core.Mixdown(9, "average")
    with pytest.raises(ValueError, match="n_channels"):
        core.Mixdown(0)
    m = core.Mixdown(3, "phase_safe_mono", n_streams=2)
    assert m.mode == 4
    m.set_mode("max_rms")
    assert m.mode == 3
    with pytest.raises(ValueError):
        m.set_mode("loudest")
    assert m.mode == 3
    for bad in (np.zeros((2, 8), np.float32), np.zeros((2, 8, 2), np.float32), np.zeros((3, 8, 3), np.float32)):
        with pytest.raises(ValueError, match="interleaved frames"):
            m.push(bad)
    x = np.zeros((2, 4, 3), np.float32)
    x[0, 0, 0] = np.nan
    with pytest.raises(ValueError, match="samples must be finite"):
        m.push(x)
    d = m.diagnostics()
    assert set(d) == {"stereo_correlation", "phase_warning_count", "strategy", "estimated_delay", "polarity_flipped"}
    assert all(v.shape == (2,) for v in d.values()) and np.isnan(d["stereo_correlation"]).all()
    assert {core.INPUT_CHANNEL_MODE_IDS[k] for k in ("average", "left", "right", "max_rms", "phase_safe_mono")} == set(range(5))
    m.close()
    m.close()


def test_engine_setters_before_and_after_start(L):
    e = core.Engine(48_000.0, 3)
    with pytest.raises(ValueError, match="n_channels must be >= 1"):
        e.set_input_channels(0, "average")
    with pytest.raises(NotImplementedError, match="at most 8"):
        e.set_input_channels(12, "average")
    with pytest.raises(ValueError, match="unknown input channel mode"):
        e.set_input_channels(2, 9)
    with pytest.raises(ValueError, match="unknown input channel mode"):
        e.set_input_channel_mode(5)  # also with mono input
    e.set_input_channel_mode("left")
    d = e.input_phase()  # mono input: nothing measured
    assert np.isnan(d["stereo_correlation"]).all() and not d["strategy"].any() and not d["polarity_flipped"].any()
    e.set_input_channels(2, "phase_safe_mono")
    e.set_input_channel_mode("average")
    e.set_input_channel_mode(4)
    with pytest.raises(ValueError, match="unknown input channel mode 6"):
        e.set_input_channel_mode(6)
    # the one-shot entry points name the streaming one, as with I/O rates set
    x = np.zeros((3, 16), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    rc = L.af_engine_process_host(e._h, x.ctypes.data_as(fp), x.ctypes.data_as(fp), 16, _lib.LAYOUT_TIME_MAJOR)
    assert rc == _lib.AF_ERR_UNSUPPORTED
    assert _lib.last_error() == "this engine takes multichannel input (af_engine_set_input_channels): use af_engine_stream_host"
    rc = L.af_engine_process_device(e._h, None, None, 16, 16, _lib.LAYOUT_STREAM_MAJOR, None)
    assert rc == _lib.AF_ERR_UNSUPPORTED and "af_engine_stream_host" in _lib.last_error()
    # shapes are checked in Python before the library is called
    with pytest.raises(ValueError, match="interleaved frames"):
        e.stream(np.zeros((3, 16), dtype=np.float32))
    with pytest.raises(ValueError, match="interleaved frames"):
        e.stream(np.zeros((3, 16, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="expected 3 streams"):
        e.stream(np.zeros((2, 16, 2), dtype=np.float32))
    bad = np.zeros((3, 16, 2), dtype=np.float32)
    bad[2, 15, 1] = np.nan
    with pytest.raises(ValueError, match="samples must be finite"):
        e.stream(bad)  # refused before the engine starts
    assert e.stream_plan(480) == (480, 480, 480)  # the plan keeps counting frames
    e.set_input_channels(1, "average")  # off again: still a configuration-time call
    with pytest.raises(ValueError, match="3-D input"):
        e.stream(np.zeros((3, 16, 2), dtype=np.float32))
    assert L.af_engine_set_input_channels(None, 2, 0) == _lib.AF_ERR_INVALID_ARGUMENT
    assert L.af_engine_set_input_channel_mode(None, 0) == _lib.AF_ERR_INVALID_ARGUMENT
    assert L.af_engine_read_input_phase(e._h, None, None, None, None, None, 2) == _lib.AF_ERR_INVALID_ARGUMENT
    e.close()
