"""CPU checks of the speech-feature measurement's C ABI and Python operators: every refusal happens before any HIP call (this runs
where there is no GPU: a HIP call would answer AF_ERR_BACKEND instead)."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

INVALID, UNSUPPORTED = -1, -5
NEW_OPERATORS = ("measure_speech_features_batch", "recommend_voice_chain", "recommend_voice_chain_batch", "configure_voice_chain")
HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "audioforge_mi.h"


@pytest.fixture(scope="module")
def L():
    from mic_eq_mi import _lib

    return _lib.load()


def test_every_declared_symbol_is_exported_and_bound(L):
    from mic_eq_mi import _lib

    declared = set(re.findall(r"\b(af_speech_features_[a-z_]+)\s*\(", HEADER.read_text()))
    assert declared == {"af_speech_features_" + name for name in (
        "create", "destroy", "frames", "chunks", "sibilance_bins", "set_frame_model", "get_frame_model", "analyze_host",
        "analyze_device", "last_kernel_ms")}
    for name in declared:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None, name
    assert {"af_speech_features_destroy", "af_speech_features_frames", "af_speech_features_chunks",
            "af_speech_features_sibilance_bins"} <= _lib.VALUE_FUNCTIONS


def test_struct_mirrors_have_the_headers_layout():
    from mic_eq_mi import _lib

    import speech_features_oracle as SO

    assert C.sizeof(_lib.SpeechFeaturesRow) == 10 * 4 + 24 * 8 == C.sizeof(SO.Row)
    assert [f[0] for f in _lib.SpeechFeaturesRow._fields_] == [f[0] for f in SO.Row._fields_]
    assert _lib.SpeechFeaturesRow.active_duration_s.offset == 40 and _lib.SpeechFeaturesRow.adaptive_floor_db.offset == 40 + 23 * 8
    assert C.sizeof(_lib.SpeechFeaturesOutputs) == 15 * C.sizeof(C.c_void_p)


def test_create_takes_48_khz_only(L):
    h = C.c_void_p()
    assert L.af_speech_features_create(48_000, 4, 96_000, 48_000, 0, C.byref(h)) == 0 and h.value
    assert L.af_speech_features_sibilance_bins(h) == 181 and L.af_speech_features_sibilance_bins(None) == 0
    L.af_speech_features_destroy(h)
    for fs in (44_100, 16_000, 96_000, 47_999):
        h = C.c_void_p()
        assert L.af_speech_features_create(fs, 4, 96_000, 48_000, 0, C.byref(h)) == UNSUPPORTED and not h.value, fs
        message = L.af_last_error().decode()
        assert str(fs) in message and "48000" in message and "resampl" in message, message  # the rate and the reason
    h = C.c_void_p()
    assert L.af_speech_features_create(0, 4, 96_000, 0, 0, C.byref(h)) == INVALID
    assert L.af_speech_features_create(48_000, 0, 96_000, 0, 0, C.byref(h)) == INVALID
    assert L.af_speech_features_create(48_000, 4, 1919, 0, 0, C.byref(h)) == INVALID
    assert L.af_speech_features_create(48_000, 4, 96_000, -1, 0, C.byref(h)) == INVALID
    assert L.af_speech_features_create(48_000, 4, 96_000, 0, -1, C.byref(h)) == INVALID
    assert L.af_speech_features_create(48_000, 4, 96_000, 0, 0, None) == INVALID
    assert [L.af_speech_features_frames(n) for n in (0, 1919, 1920, 2879, 2880, 201_600)] == [0, 0, 1, 1, 2, 209]
    assert [L.af_speech_features_chunks(n) for n in (0, 1, 960, 961, 2879, 201_600)] == [0, 1, 1, 2, 3, 210]


def test_analyze_refuses_before_any_hip_call(L):
    from mic_eq_mi import _lib

    h = C.c_void_p()
    assert L.af_speech_features_create(48_000, 2, 4000, 3000, 0, C.byref(h)) == 0
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    x = np.zeros((3, 4000), dtype=np.float32)
    level, v = np.zeros(3), np.zeros((3, 4))
    px, pl, pv = x.ctypes.data_as(fp), level.ctypes.data_as(dp), v.ctypes.data_as(dp)
    out = _lib.SpeechFeaturesOutputs()
    ok = dict(h=h, speech=px, n=4000, B=2, stride=4000, level=pl, vad=None, n_vad=0, noise=px, m=3000, ns=4000)

    def call(fn, o=C.byref(out), **kw):
        a = dict(ok, **kw)
        return fn(a["h"], a["speech"], a["n"], a["B"], a["stride"], a["level"], a["vad"], a["n_vad"], a["noise"], a["m"], a["ns"], o)

    for fn in (L.af_speech_features_analyze_host, L.af_speech_features_analyze_device):
        assert call(fn, h=None) == INVALID
        assert call(fn, o=None) == INVALID
        assert call(fn, speech=None) == INVALID and call(fn, level=None) == INVALID
        assert call(fn, B=0) == INVALID
        assert call(fn, B=3) == INVALID and "max_streams 2" in L.af_last_error().decode()  # above the handle's
        assert call(fn, n=1919, stride=1919) == INVALID and "shorter than one analysis frame" in L.af_last_error().decode()
        assert call(fn, n=4001, stride=4001) == INVALID and "max_speech_samples" in L.af_last_error().decode()
        assert call(fn, stride=3999) == INVALID
        assert call(fn, vad=pv) == INVALID and call(fn, n_vad=4) == INVALID  # a posterior array and its length go together
        assert call(fn, noise=None) == INVALID  # n_noise without noise
        assert call(fn, m=3001) == INVALID and call(fn, ns=2999) == INVALID and call(fn, m=-1) == INVALID
    ms = (C.c_double * 5)(*([-1.0] * 5))
    assert L.af_speech_features_last_kernel_ms(None, ms, 5) == INVALID and L.af_speech_features_last_kernel_ms(h, None, 5) == INVALID
    assert L.af_speech_features_last_kernel_ms(h, ms, 4) == INVALID
    assert L.af_speech_features_last_kernel_ms(h, ms, 5) == 0 and list(ms) == [0.0] * 5  # before any call
    L.af_speech_features_destroy(h)


def test_smooth_rows_argument_contract(L):
    h = C.c_void_p()
    assert L.af_voice_spectrum_create(48_000, 256, 0, C.byref(h)) == 0
    dp = C.POINTER(C.c_double)
    rows = np.zeros((2, 129))
    p = rows.ctypes.data_as(dp)
    assert L.af_voice_spectrum_smooth_rows(None, p, 2, p) == INVALID and L.af_voice_spectrum_smooth_rows(h, None, 2, p) == INVALID
    assert L.af_voice_spectrum_smooth_rows(h, p, 2, None) == INVALID and L.af_voice_spectrum_smooth_rows(h, p, 0, p) == INVALID
    L.af_voice_spectrum_destroy(h)
    import mic_eq_mi

    vs = mic_eq_mi.VoiceSpectrum(48_000, 256)
    with pytest.raises(ValueError, match="129"):
        vs.smooth(np.zeros((2, 128)))
    vs.close()
    with pytest.raises(ValueError, match="Room-noise capture was too short"):
        mic_eq_mi.recommend_voice_chain_batch(np.zeros((2, 48_000), np.float32), np.zeros((2, 200_000), np.float32), 48_000)
    with pytest.raises(ValueError, match="Voice capture was too short"):
        mic_eq_mi.recommend_voice_chain_batch(np.zeros((2, 96_000), np.float32), np.zeros((2, 100_000), np.float32), 48_000)
    with pytest.raises(NotImplementedError, match="44100"):
        mic_eq_mi.recommend_voice_chain_batch(np.zeros((2, 96_000), np.float32), np.zeros((2, 200_000), np.float32), 44_100)


def test_frame_model_setter_round_trip(L):
    h = C.c_void_p()
    assert L.af_speech_features_create(48_000, 1, 1920, 0, 0, C.byref(h)) == 0
    dp = C.POINTER(C.c_double)
    intercept, w = C.c_double(), np.zeros(6)
    assert L.af_speech_features_get_frame_model(h, C.byref(intercept), w.ctypes.data_as(dp)) == 0
    assert intercept.value == -14.745480728063148  # the published model, deesser_fusion.py:30-41
    assert w.tolist() == [1.4074734365324453, 5.220098953258285, 2.427808017651834, 1.1022350583682425, 4.160012489488813,
                          2.4617269295476714]
    new = np.array([0.5, -1.0, 2.0, 0.0, 3.5, 1e-3])
    assert L.af_speech_features_set_frame_model(h, -2.25, new.ctypes.data_as(dp)) == 0
    assert L.af_speech_features_get_frame_model(h, C.byref(intercept), w.ctypes.data_as(dp)) == 0
    assert intercept.value == -2.25 and np.array_equal(w, new)
    bad = new.copy()
    bad[3] = np.nan
    assert L.af_speech_features_set_frame_model(h, -2.25, bad.ctypes.data_as(dp)) == INVALID
    assert L.af_speech_features_set_frame_model(h, float("inf"), new.ctypes.data_as(dp)) == INVALID
    assert L.af_speech_features_set_frame_model(h, 0.0, None) == INVALID and L.af_speech_features_set_frame_model(None, 0.0, new.ctypes.data_as(dp)) == INVALID
    assert L.af_speech_features_get_frame_model(h, C.byref(intercept), w.ctypes.data_as(dp)) == 0 and np.array_equal(w, new)  # a refusal changes nothing
    L.af_speech_features_destroy(h)


def test_python_operators_exist_and_refuse():
    import mic_eq_mi

    for name in NEW_OPERATORS:
        fn = getattr(mic_eq_mi, name)
        assert callable(fn) and fn is not mic_eq_mi._missing_core and name in mic_eq_mi.__all__ and name in mic_eq_mi._OPERATORS
    assert "SpeechFeatures" in mic_eq_mi.__all__ and mic_eq_mi.SpeechFeatures is not None
    with pytest.raises(ImportError, match="unavailable or missing this API"):  # what every operator is without the library
        mic_eq_mi._missing_core()
    x = np.zeros((2, 4000), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="44100"):
        mic_eq_mi.measure_speech_features_batch(x, 44_100, [-60.0, -60.0])
    with pytest.raises(ValueError, match=r"\[n_streams, n\]"):
        mic_eq_mi.measure_speech_features_batch(x[0], 48_000, [-60.0])
    with pytest.raises(ValueError, match="shorter than one analysis frame"):
        mic_eq_mi.measure_speech_features_batch(x[:, :1000], 48_000, [-60.0, -60.0])
    sf = mic_eq_mi.SpeechFeatures(48_000, 2, 4000, 4000)
    with pytest.raises(ValueError, match="noise_rms_db"):
        sf.analyze(x, [-60.0])
    with pytest.raises(ValueError, match="vad_probabilities"):
        sf.analyze(x, [-60.0, -60.0], vad_probabilities=np.zeros((3, 5)))
    with pytest.raises(ValueError, match="noise_audio"):
        sf.analyze(x, [-60.0, -60.0], noise_audio=x[:1])
    with pytest.raises(ValueError, match="six values"):
        sf.set_frame_model(0.0, [1.0, 2.0])
    assert sf.frames(4000) == 3 and sf.chunks(4000) == 5 and sf.sibilance_bins == 181
    sf.close()


def test_operators_raise_import_error_without_the_library(tmp_path):
    """A fresh interpreter whose AF_LIB_PATH names no file: the package imports, says the core is missing, and every new operator
    is the degradation path (ImportError), with no CPU fallback behind it."""
    import os
    import subprocess
    import sys

    package = pathlib.Path(__file__).resolve().parents[1] / "audio-forge_amd"
    code = (f"import sys; sys.path.insert(0, {str(package)!r}); import mic_eq_mi\n"
            "assert not mic_eq_mi.CORE_AVAILABLE and mic_eq_mi.SpeechFeatures is None\n"
            f"for name in {NEW_OPERATORS!r}:\n"
            "    try:\n"
            "        getattr(mic_eq_mi, name)(None, None, 48000)\n"
            "    except ImportError as error:\n"
            "        assert 'unavailable or missing this API' in str(error), error\n"
            "    else:\n"
            "        raise SystemExit(name + ' did not raise ImportError')\n"
            "print('ok')\n")
    env = dict(os.environ, AF_LIB_PATH=str(tmp_path / "no_such_library.so"))
    done = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0 and done.stdout.strip() == "ok", done.stderr[-2000:]
