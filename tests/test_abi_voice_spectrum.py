"""CPU checks of the voice spectrum C ABI: every refusal happens before any HIP call (this runs where there is no GPU: a HIP
call would answer AF_ERR_BACKEND instead), and the host-only entry points answer like the reference."""
import ctypes as C

import numpy as np
import pytest

import voice_spectrum_stimulus as VS

INVALID, NON_FINITE, STATE, UNSUPPORTED = -1, -3, -4, -5


@pytest.fixture(scope="module")
def L():
    from mic_eq_mi import _lib

    return _lib.load()


def create(L, nperseg=256, fs=48_000, device=0):
    h = C.c_void_p()
    return L.af_voice_spectrum_create(fs, nperseg, device, C.byref(h)), h


def err(L):
    return L.af_last_error().decode()


@pytest.mark.parametrize("nperseg", [0, 255, 300, 16384, -256, 128])
def test_unsupported_nperseg_is_refused(L, nperseg):
    rc, h = create(L, nperseg)
    assert rc == UNSUPPORTED and not h.value
    assert "powers of two from 256 to 8192" in err(L)


@pytest.mark.parametrize("nperseg", [256, 512, 1024, 2048, 4096, 8192])
def test_supported_nperseg_gives_bins_and_frames(L, nperseg):
    rc, h = create(L, nperseg)
    assert rc == 0
    assert L.af_voice_spectrum_bins(h) == nperseg // 2 + 1
    for n in (0, nperseg - 1, nperseg, nperseg + nperseg // 2 - 1, 2 * nperseg, VS.main_length(nperseg)):
        want = 0 if n < nperseg else (n - nperseg) // (nperseg // 2) + 1
        assert L.af_voice_spectrum_frames(h, n) == want
    L.af_voice_spectrum_destroy(h)


def test_create_argument_contract(L):
    assert L.af_voice_spectrum_create(48_000, 256, 0, None) == INVALID
    assert create(L, 256, fs=0)[0] == INVALID
    assert create(L, 256, device=-1)[0] == INVALID
    L.af_voice_spectrum_destroy(None)
    assert L.af_voice_spectrum_bins(None) == 0 and L.af_voice_spectrum_frames(None, 4096) == 0


def test_analyze_refuses_bad_arguments_before_any_hip_call(L):
    from mic_eq_mi import _lib

    rc, h = create(L, 256)
    assert rc == 0
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    audio = np.zeros((2, 600), dtype=np.float32)
    vad = np.zeros((2, 4))
    noise = np.zeros((2, 300), dtype=np.float32)
    out = _lib.VoiceSpectrumOutputs()
    a, v, z, o = audio.ctypes.data_as(fp), vad.ctypes.data_as(dp), noise.ctypes.data_as(fp), C.byref(out)
    for entry in (L.af_voice_spectrum_analyze_host, L.af_voice_spectrum_analyze_device):
        if entry is L.af_voice_spectrum_analyze_device:
            a, z = C.c_void_p(audio.ctypes.data), C.c_void_p(noise.ctypes.data)  # never dereferenced: refused first
        assert entry(None, a, 600, 2, 600, None, 0, None, 0, 0, o) == INVALID
        assert entry(h, None, 600, 2, 600, None, 0, None, 0, 0, o) == INVALID
        assert entry(h, a, 600, 2, 600, None, 0, None, 0, 0, None) == INVALID
        assert entry(h, a, 600, 0, 600, None, 0, None, 0, 0, o) == INVALID
        assert entry(h, a, 600, 2, 599, None, 0, None, 0, 0, o) == INVALID and "stride" in err(L)
        assert entry(h, a, 255, 2, 600, None, 0, None, 0, 0, o) == INVALID
        assert err(L) == "Audio too short for FFT: need 256 samples, got 255 (0.01 seconds)"
        assert entry(h, a, 600, 2, 600, v, 0, None, 0, 0, o) == INVALID and "n_vad" in err(L)  # an array without a count
        assert entry(h, a, 600, 2, 600, None, 4, None, 0, 0, o) == INVALID
        assert entry(h, a, 600, 2, 600, None, 0, z, 300, 299, o) == INVALID and "noise_stride" in err(L)
        assert entry(h, a, 600, 2, 600, None, 0, z, -1, 300, o) == INVALID
        assert entry(h, a, 600, 2, 600, None, 0, None, 300, 300, o) == INVALID
    audio[1, 17] = np.nan
    assert L.af_voice_spectrum_analyze_host(h, audio.ctypes.data_as(fp), 600, 2, 600, None, 0, None, 0, 0, o) == NON_FINITE
    assert err(L) == "audio must contain only finite samples"
    audio[1, 17] = 0.0
    noise[0, 5] = np.inf
    assert L.af_voice_spectrum_analyze_host(h, audio.ctypes.data_as(fp), 600, 2, 600, None, 0, noise.ctypes.data_as(fp), 300, 300,
                                            o) == NON_FINITE
    L.af_voice_spectrum_destroy(h)


def test_read_windows_and_timer_before_any_call(L):
    rc, h = create(L, 256)
    count, ms = C.c_int32(-1), C.c_double(-1.0)
    assert L.af_voice_spectrum_read_windows(None, 0, None, None, None, 0, C.byref(count)) == INVALID
    assert L.af_voice_spectrum_read_windows(h, 0, None, None, None, 0, C.byref(count)) == STATE
    assert L.af_voice_spectrum_last_kernel_ms(h, C.byref(ms)) == 0 and ms.value == 0.0
    assert L.af_voice_spectrum_last_kernel_ms(h, None) == INVALID
    L.af_voice_spectrum_destroy(h)


def test_octave_bands_equal_the_reference(L):
    dp = C.POINTER(C.c_double)
    fx = VS.fixture()
    for fraction in (2, 3, 6, 12):
        want = fx[f"octave{fraction}"]
        n = C.c_int32()
        assert L.af_voice_spectrum_octave_bands(fraction, None, None, None, 0, C.byref(n)) == 0 and n.value == want.shape[1]
        got = np.zeros((3, n.value))
        assert L.af_voice_spectrum_octave_bands(fraction, got[0].ctypes.data_as(dp), got[1].ctypes.data_as(dp), got[2].ctypes.data_as(dp),
                                                n.value, C.byref(n)) == 0
        assert np.array_equal(got, want), fraction
        assert L.af_voice_spectrum_octave_bands(fraction, got[0].ctypes.data_as(dp), None, None, n.value - 1, C.byref(n)) == INVALID
    assert L.af_voice_spectrum_octave_bands(0, None, None, None, 0, C.byref(n)) == INVALID


def test_python_operators_exist_and_refuse_short_audio():
    import mic_eq_mi

    for name in ("compute_voice_spectrum", "compute_voice_spectrum_batch", "measure_voice_spectra"):
        fn = getattr(mic_eq_mi, name)
        assert callable(fn) and fn is not mic_eq_mi._missing_core and name in mic_eq_mi.__all__ and name in mic_eq_mi._OPERATORS
    with pytest.raises(ValueError, match=r"Audio too short for FFT: need 4096 samples, got 4095 \(0\.09 seconds\)"):
        mic_eq_mi.compute_voice_spectrum(np.zeros(4095, dtype=np.float32))
    with pytest.raises(ValueError, match=r"Audio too short for FFT: need 512 samples, got 100 \(0\.00 seconds\)"):
        mic_eq_mi.measure_voice_spectra(np.zeros((3, 100), dtype=np.float32), 48_000, 512)
    with pytest.raises(NotImplementedError, match="powers of two"):
        mic_eq_mi.compute_voice_spectrum(np.zeros(4000, dtype=np.float32), 48_000, 300)
