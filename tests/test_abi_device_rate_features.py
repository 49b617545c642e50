"""CPU checks of the device-rate speech features' C ABI (af_device_rate_features_*) and of the `device_rate` keyword: the rates
it takes and the ones it refuses with their reasons, and every refusal before any HIP call (this runs where there is no GPU: a
HIP call would answer AF_ERR_BACKEND instead)."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import speech_features_rates_oracle as RO

INVALID, UNSUPPORTED = -1, -5
HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "audioforge_mi.h"
NAMES = ("create", "destroy", "frames", "chunks", "resampled_length", "sibilance_bins", "set_frame_model", "get_frame_model",
         "set_scratch_bytes", "analyze_host", "analyze_device", "last_kernel_ms", "debug_resample_host")


@pytest.fixture(scope="module")
def L():
    from mic_eq_mi import _lib

    return _lib.load()


def create(L, fs, streams=4, speech=400_000, noise=100_000, device=0):
    h = C.c_void_p()
    return L.af_device_rate_features_create(fs, streams, speech, noise, device, C.byref(h)), h


def test_every_declared_symbol_is_exported_and_bound(L):
    from mic_eq_mi import _lib

    declared = set(re.findall(r"\b(af_device_rate_features_[a-z_]+)\s*\(", HEADER.read_text()))
    assert declared == {"af_device_rate_features_" + name for name in NAMES}
    for name in declared:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None, name
    assert {"af_device_rate_features_" + name for name in ("destroy", "frames", "chunks", "resampled_length", "sibilance_bins")} <= _lib.VALUE_FUNCTIONS


def test_create_takes_the_listed_rates_and_names_the_rule_a_refused_one_breaks(L):
    for fs in RO.RATES:
        rc, h = create(L, fs)
        assert rc == 0 and h.value, fs
        g = RO.geometry(fs)
        assert L.af_device_rate_features_sibilance_bins(h) == (89 if fs == 16_000 else 181)
        for n in (0, g["frame"] - 1, g["frame"], 3 * g["hop"] - 1, 3 * g["hop"], 170 * g["hop"] + 123):
            assert L.af_device_rate_features_frames(h, n) == (RO.frames(fs, n) if n > 0 else 0), (fs, n)
            n48 = -(-n * g["up"] // g["down"])
            assert L.af_device_rate_features_resampled_length(h, n) == n48 and L.af_device_rate_features_chunks(h, n) == -(-n48 // 960), (fs, n)
        L.af_device_rate_features_destroy(h)
    assert L.af_device_rate_features_frames(None, 5000) == 0 and L.af_device_rate_features_sibilance_bins(None) == 0
    for fs, reason in ((11_025, "whole, even"), (47_999, "whole, even"), (192_000, "above the 3840 samples"), (8000, "below 16000 Hz"),
                       (64_000, "not one of the listed rates")):
        rc, h = create(L, fs)
        message = L.af_last_error().decode()
        assert rc == UNSUPPORTED and not h.value and str(fs) in message and reason in message and "44100" in message, (fs, message)
    assert create(L, 0)[0] == INVALID and create(L, 44_100, streams=0)[0] == INVALID
    assert create(L, 44_100, speech=1763)[0] == INVALID and "1764" in L.af_last_error().decode()
    assert create(L, 44_100, noise=-1)[0] == INVALID and create(L, 44_100, device=-1)[0] == INVALID
    assert L.af_device_rate_features_create(44_100, 4, 96_000, 0, 0, None) == INVALID


def test_analyze_and_the_tap_refuse_before_any_hip_call(L):
    from mic_eq_mi import _lib

    rc, h = create(L, 44_100, streams=2, speech=4000, noise=3000)
    assert rc == 0
    fp, dp, bp, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    x = np.zeros((3, 4000), dtype=np.float32)
    level, v = np.zeros(3), np.zeros((3, 4))
    px, pl, pv = x.ctypes.data_as(fp), level.ctypes.data_as(dp), v.ctypes.data_as(dp)
    out = _lib.SpeechFeaturesOutputs()
    ok = dict(h=h, speech=px, n=4000, B=2, stride=4000, level=pl, vad=None, n_vad=0, noise=px, m=3000, ns=4000)

    def call(fn, o=C.byref(out), **kw):
        a = dict(ok, **kw)
        return fn(a["h"], a["speech"], a["n"], a["B"], a["stride"], a["level"], a["vad"], a["n_vad"], a["noise"], a["m"], a["ns"], o)

    for fn in (L.af_device_rate_features_analyze_host, L.af_device_rate_features_analyze_device):
        assert call(fn, h=None) == INVALID and call(fn, o=None) == INVALID
        assert call(fn, speech=None) == INVALID and call(fn, level=None) == INVALID
        assert call(fn, B=0) == INVALID
        assert call(fn, B=3) == INVALID and "max_streams 2" in L.af_last_error().decode()
        assert call(fn, n=1763, stride=1763) == INVALID and "one analysis frame of 1764" in L.af_last_error().decode()
        assert call(fn, n=4001, stride=4001) == INVALID and "max_speech_samples" in L.af_last_error().decode()
        assert call(fn, stride=3999) == INVALID
        assert call(fn, vad=pv) == INVALID and call(fn, n_vad=4) == INVALID
        assert call(fn, noise=None) == INVALID
        assert call(fn, m=3001) == INVALID and call(fn, ns=2999) == INVALID and call(fn, m=-1) == INVALID
    flags = np.zeros((2, 3), dtype=np.uint8)
    y, mask, counts = np.zeros((2, 4354)), np.zeros((2, 4354), dtype=np.uint8), np.zeros((2, 5), dtype=np.int32)
    tap = L.af_device_rate_features_debug_resample_host
    good = [h, px, 4000, 2, 4000, flags.ctypes.data_as(bp), y.ctypes.data_as(dp), mask.ctypes.data_as(bp), counts.ctypes.data_as(ip)]
    for at in (0, 1, 5, 6, 7, 8):
        assert tap(*[None if i == at else a for i, a in enumerate(good)]) == INVALID, at
    for at, value in ((2, 1763), (2, 4001), (3, 0), (3, 3), (4, 3999)):
        assert tap(*[value if i == at else a for i, a in enumerate(good)]) == INVALID, (at, value)
    rc, h48 = create(L, 48_000, streams=2, speech=4000, noise=0)
    assert rc == 0 and tap(h48, *good[1:]) == INVALID and "does not resample" in L.af_last_error().decode()
    L.af_device_rate_features_destroy(h48)
    assert L.af_device_rate_features_set_scratch_bytes(None, 1 << 20) == INVALID and L.af_device_rate_features_set_scratch_bytes(h, 0) == INVALID
    assert L.af_device_rate_features_set_scratch_bytes(h, 1 << 20) == 0
    ms = (C.c_double * 6)(*([-1.0] * 6))
    assert L.af_device_rate_features_last_kernel_ms(None, ms, 6) == INVALID and L.af_device_rate_features_last_kernel_ms(h, None, 6) == INVALID
    assert L.af_device_rate_features_last_kernel_ms(h, ms, 5) == INVALID
    assert L.af_device_rate_features_last_kernel_ms(h, ms, 6) == 0 and list(ms) == [0.0] * 6  # before any call
    L.af_device_rate_features_destroy(h)


def test_frame_model_round_trip(L):
    rc, h = create(L, 32_000)
    dp = C.POINTER(C.c_double)
    intercept, w = C.c_double(), np.zeros(6)
    assert L.af_device_rate_features_get_frame_model(h, C.byref(intercept), w.ctypes.data_as(dp)) == 0
    assert intercept.value == -14.745480728063148 and w[1] == 5.220098953258285
    new = np.array([0.5, -1.0, 2.0, 0.0, 3.5, 1e-3])
    assert L.af_device_rate_features_set_frame_model(h, -2.25, new.ctypes.data_as(dp)) == 0
    assert L.af_device_rate_features_get_frame_model(h, C.byref(intercept), w.ctypes.data_as(dp)) == 0
    assert intercept.value == -2.25 and np.array_equal(w, new)
    assert L.af_device_rate_features_set_frame_model(h, float("nan"), new.ctypes.data_as(dp)) == INVALID
    assert L.af_device_rate_features_set_frame_model(None, 0.0, new.ctypes.data_as(dp)) == INVALID
    assert L.af_device_rate_features_get_frame_model(None, C.byref(intercept), w.ctypes.data_as(dp)) == INVALID
    L.af_device_rate_features_destroy(h)


def test_the_device_rate_keyword_opts_in():
    import mic_eq_mi
    from mic_eq_mi import mic_eq_core as core

    assert core.SPEECH_FEATURES_RATES == RO.RATES
    x = np.zeros((2, 4000), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="44100"):  # the default is what it was
        mic_eq_mi.SpeechFeatures(44_100, 2, 4000, 0)
    with pytest.raises(NotImplementedError, match="11025.*whole, even"):
        mic_eq_mi.SpeechFeatures(11_025, 2, 4000, 0, device_rate=True)
    with pytest.raises(NotImplementedError, match="47999"):
        mic_eq_mi.measure_speech_features_batch(x, 47_999, [-60.0, -60.0], device_rate=True)
    with pytest.raises(NotImplementedError, match="192000"):
        mic_eq_mi.recommend_voice_chain_batch(np.zeros((2, 400_000), np.float32), np.zeros((2, 800_000), np.float32), 192_000, device_rate=True)
    with pytest.raises(ValueError, match="one analysis frame of 1764"):
        mic_eq_mi.measure_speech_features_batch(x[:, :1000], 44_100, [-60.0, -60.0], device_rate=True)
    with pytest.raises(ValueError, match="Voice capture was too short"):
        mic_eq_mi.recommend_voice_chain_batch(np.zeros((2, 96_000), np.float32), np.zeros((2, 100_000), np.float32), 44_100, device_rate=True)
    sf = mic_eq_mi.SpeechFeatures(44_100, 2, 4000, 4000, device_rate=True)
    assert (sf.frames(4000), sf.chunks(4000), sf.resampled_length(4000), sf.sibilance_bins) == (3, 5, 4354, 181)
    with pytest.raises(ValueError, match="noise_rms_db"):
        sf.analyze(x, [-60.0])
    with pytest.raises(ValueError, match="active_frames"):
        sf.resample(x, np.zeros((2, 2), dtype=np.uint8))
    sf.close()
    old = mic_eq_mi.SpeechFeatures(48_000, 2, 4000, 0)
    assert old.resampled_length(4000) == 4000
    with pytest.raises(ValueError, match="device_rate=True"):
        old.resample(x, np.zeros((2, 3), dtype=np.uint8))
    old.close()
