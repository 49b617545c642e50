"""CPU checks of the reliability statistics' C ABI and Python operators: every refusal happens before any HIP call (this runs
where there is no GPU: a HIP call would answer AF_ERR_BACKEND instead)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

INVALID, STATE = -1, -4
FIELDS = ("freqs", "median_spectrum_db", "window_spectra_db", "voiced_window_ratio", "snr_db", "spectral_repeatability",
          "spectral_tilt_db_per_octave", "residual_confidence", "used_single_spectrum_fallback", "measurement_coverage",
          "outlier_rejection_ratio", "vad_probability_used", "vad_active_window_ratio", "spectral_snr_db", "noise_spectrum_db",
          "noise_reference_source", "measurement_uncertainty_db", "phonetic_coverage", "effective_measurement_blocks")  # spectrum.py:37-55


@pytest.fixture(scope="module")
def L():
    from mic_eq_mi import _lib

    return _lib.load()


def test_set_and_read_refuse_before_any_hip_call(L):
    from mic_eq_mi import _lib

    h = C.c_void_p()
    assert L.af_voice_spectrum_create(48_000, 256, 0, C.byref(h)) == 0
    out = _lib.VoiceSpectrumReliabilityOutputs()
    assert L.af_voice_spectrum_set_reliability(None, 1) == INVALID
    assert L.af_voice_spectrum_read_reliability(None, C.byref(out)) == INVALID
    assert L.af_voice_spectrum_read_reliability(h, None) == INVALID
    assert L.af_voice_spectrum_read_reliability(h, C.byref(out)) == STATE  # no call has been made
    assert "reliability" in L.af_last_error().decode()
    assert L.af_voice_spectrum_set_reliability(h, 1) == 0
    assert L.af_voice_spectrum_read_reliability(h, C.byref(out)) == STATE  # the switch alone computes nothing
    assert L.af_voice_spectrum_set_reliability(h, 0) == 0
    ms = (C.c_double * 5)(*([-1.0] * 5))
    assert L.af_voice_spectrum_last_reliability_kernel_ms(None, ms, 5) == INVALID
    assert L.af_voice_spectrum_last_reliability_kernel_ms(h, None, 5) == INVALID
    assert L.af_voice_spectrum_last_reliability_kernel_ms(h, ms, 4) == INVALID
    assert L.af_voice_spectrum_last_reliability_kernel_ms(h, ms, 5) == 0 and list(ms) == [0.0] * 5  # before any call
    L.af_voice_spectrum_destroy(h)


def test_struct_mirrors_have_the_headers_layout():
    from mic_eq_mi import _lib

    assert C.sizeof(_lib.VoiceSpectrumReliabilityRow) == 7 * 8 + 6 * 4
    assert _lib.VoiceSpectrumReliabilityRow.voiced.offset == 56 and _lib.VoiceSpectrumReliabilityRow.used_closest_windows.offset == 72
    assert C.sizeof(_lib.VoiceSpectrumReliabilityOutputs) == 7 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.VoiceSpectrumRow) == 40 and C.sizeof(_lib.VoiceSpectrumOutputs) == 10 * 8  # unchanged


def test_python_operators_exist_and_refuse():
    import mic_eq_mi

    for name in ("analyze_voice_spectrum", "analyze_voice_spectrum_batch"):
        fn = getattr(mic_eq_mi, name)
        assert callable(fn) and fn is not mic_eq_mi._missing_core and name in mic_eq_mi.__all__ and name in mic_eq_mi._OPERATORS
    assert "VoiceSpectrumResult" in mic_eq_mi.__all__
    with pytest.raises(ValueError, match=r"Audio too short for FFT: need 4096 samples, got 4095 \(0\.09 seconds\)"):
        mic_eq_mi.analyze_voice_spectrum(np.zeros(4095, dtype=np.float32))
    with pytest.raises(ValueError, match=r"Audio too short for FFT: need 512 samples, got 100 \(0\.00 seconds\)"):
        mic_eq_mi.analyze_voice_spectrum_batch(np.zeros((3, 100), dtype=np.float32), 48_000, 512)
    audio = np.zeros(8192, dtype=np.float32)
    with pytest.raises(NotImplementedError, match="noise_spectrum_override"):
        mic_eq_mi.analyze_voice_spectrum(audio, noise_spectrum_override=(np.arange(4.0), np.zeros(4)))
    with pytest.raises(NotImplementedError, match="noise_reference_source_override"):
        mic_eq_mi.analyze_voice_spectrum(audio, noise_reference_source_override="room_tone")


def test_result_dataclass_has_the_references_fields_and_defaults():
    import mic_eq_mi

    R = mic_eq_mi.VoiceSpectrumResult
    assert tuple(f.name for f in dataclasses.fields(R)) == FIELDS
    z = np.zeros(3)
    r = R(freqs=z, median_spectrum_db=z, window_spectra_db=z[None], voiced_window_ratio=0.5, snr_db=0.0, spectral_repeatability=z,
          spectral_tilt_db_per_octave=0.0, residual_confidence=0.0, used_single_spectrum_fallback=False)
    assert (r.measurement_coverage, r.outlier_rejection_ratio, r.vad_probability_used, r.vad_active_window_ratio) == (1.0, 0.0, False, 0.0)
    assert r.spectral_snr_db is None and r.noise_spectrum_db is None and r.measurement_uncertainty_db is None
    assert (r.noise_reference_source, r.phonetic_coverage, r.effective_measurement_blocks) == ("unavailable", 0.0, 0.0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        r.snr_db = 1.0
