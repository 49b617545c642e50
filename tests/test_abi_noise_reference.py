"""CPU checks of the room-noise reference analysis' C ABI, the noise-spectrum override's setter and the Python operators: every
refusal happens before any HIP call (this runs where there is no GPU: a HIP call would answer AF_ERR_BACKEND instead)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

INVALID, UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def L():
    from mic_eq_mi import _lib

    return _lib.load()


def test_struct_mirrors_have_the_headers_layout():
    from mic_eq_mi import _lib

    import noise_reference_oracle as NO

    assert C.sizeof(_lib.NoiseReferenceRow) == 4 * 4 + 19 * 8 + 3 * 8 + 6 * 4 == C.sizeof(NO.Row)
    assert _lib.NoiseReferenceRow.quality_score.offset == 16 and _lib.NoiseReferenceRow.finite_samples.offset == 168
    assert _lib.NoiseReferenceRow.in_capture_noise_frame_count.offset == 192
    assert [f[0] for f in _lib.NoiseReferenceRow._fields_] == [f[0] for f in NO.Row._fields_]
    assert C.sizeof(_lib.NoiseReferenceOutputs) == 13 * C.sizeof(C.c_void_p)
    assert C.sizeof(_lib.VoiceSpectrumRow) == 40 and C.sizeof(_lib.VoiceSpectrumOutputs) == 10 * 8  # unchanged


def test_create_accepts_the_rates_of_the_issue_and_refuses_the_rest(L):
    for fs, frame in ((8000, 1600), (16_000, 3200), (22_050, 4410), (24_000, 4800), (32_000, 6400), (44_100, 8820), (48_000, 9600),
                      (2560, 512), (100, 512), (3000, 600), (3150, 630), (4410, 882), (96_000, 19_200)):
        h = C.c_void_p()
        assert L.af_noise_reference_create(fs, 0, C.byref(h)) == 0, fs
        assert L.af_noise_reference_frame_size(h) == frame
        assert L.af_noise_reference_bins(h, 10 * frame) == frame // 2 + 1 and L.af_noise_reference_bins(h, frame) == frame // 2 + 1
        assert L.af_noise_reference_bins(h, frame - 1) == (frame - 1) // 2 + 1  # the grid of a capture below one frame
        assert L.af_noise_reference_bins(h, 0) == 2 and L.af_noise_reference_bins(h, 1) == 2 and L.af_noise_reference_bins(h, 5) == 3
        assert L.af_noise_reference_frames(h, frame - 1) == 0 and L.af_noise_reference_frames(h, frame) == 1
        assert L.af_noise_reference_frames(h, frame + frame // 2 - 1) == 1 and L.af_noise_reference_frames(h, 2 * frame) == 3
        L.af_noise_reference_destroy(h)
    for fs, word in ((11_025, "odd"), (2750, "prime factor above 7"), (192_000, "LDS"), (2_000_000, "does not fit")):
        h = C.c_void_p()
        assert L.af_noise_reference_create(fs, 0, C.byref(h)) == UNSUPPORTED and not h.value, fs
        message = L.af_last_error().decode()
        assert str(fs) in message and word in message, message  # the message names the sample rate
    h = C.c_void_p()
    assert L.af_noise_reference_create(0, 0, C.byref(h)) == INVALID
    assert L.af_noise_reference_create(48_000, -1, C.byref(h)) == INVALID
    assert L.af_noise_reference_create(48_000, 0, None) == INVALID
    assert L.af_noise_reference_frame_size(None) == 0 and L.af_noise_reference_bins(None, 100) == 0 and L.af_noise_reference_frames(None, 100) == 0


def test_analyze_refuses_before_any_hip_call(L):
    from mic_eq_mi import _lib

    h = C.c_void_p()
    assert L.af_noise_reference_create(3000, 0, C.byref(h)) == 0
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    x = np.zeros((2, 1000), dtype=np.float32)
    v = np.zeros((2, 4), dtype=np.float64)
    px, pv = x.ctypes.data_as(fp), v.ctypes.data_as(dp)
    out = _lib.NoiseReferenceOutputs()
    ok = dict(h=h, noise=px, n_noise=1000, B=2, ns=1000, speech=px, n_speech=1000, ss=1000, nv=None, nnv=0, sv=None, nsv=0)

    def call(fn=L.af_noise_reference_analyze_host, o=C.byref(out), **kw):
        a = dict(ok, **kw)
        return fn(a["h"], a["noise"], a["n_noise"], a["B"], a["ns"], a["speech"], a["n_speech"], a["ss"], a["nv"], a["nnv"], a["sv"],
                  a["nsv"], None, None, o)

    for fn in (L.af_noise_reference_analyze_host, L.af_noise_reference_analyze_device):
        assert call(fn, h=None) == INVALID
        assert call(fn, o=None) == INVALID
        assert call(fn, B=0) == INVALID
        assert call(fn, ns=999) == INVALID and call(fn, n_noise=-1) == INVALID
        assert call(fn, noise=None) == INVALID
        assert call(fn, ss=999) == INVALID
        assert call(fn, speech=None) == INVALID  # n_speech without speech
        assert call(fn, nv=pv) == INVALID and call(fn, nnv=4) == INVALID  # a posterior array and its length go together
        assert call(fn, sv=pv) == INVALID and call(fn, nsv=4) == INVALID
    ms = (C.c_double * 4)(*([-1.0] * 4))
    assert L.af_noise_reference_last_kernel_ms(None, ms, 4) == INVALID and L.af_noise_reference_last_kernel_ms(h, None, 4) == INVALID
    assert L.af_noise_reference_last_kernel_ms(h, ms, 3) == INVALID
    assert L.af_noise_reference_last_kernel_ms(h, ms, 4) == 0 and list(ms) == [0.0] * 4  # before any call
    L.af_noise_reference_destroy(h)


def test_noise_override_setter_contract(L):
    h = C.c_void_p()
    assert L.af_voice_spectrum_create(48_000, 256, 0, C.byref(h)) == 0
    dp = C.POINTER(C.c_double)
    f, s = np.arange(4.0), np.zeros((3, 4))
    pf, ps = f.ctypes.data_as(dp), s.ctypes.data_as(dp)
    assert L.af_voice_spectrum_set_noise_override(None, pf, ps, 4, 3, 4, 0) == INVALID
    assert L.af_voice_spectrum_set_noise_override(h, None, ps, 4, 3, 4, 0) == INVALID
    assert L.af_voice_spectrum_set_noise_override(h, pf, ps, 0, 3, 4, 0) == INVALID
    assert L.af_voice_spectrum_set_noise_override(h, pf, ps, 4, 0, 4, 0) == INVALID
    assert L.af_voice_spectrum_set_noise_override(h, pf, ps, 4, 3, 3, 0) == INVALID
    assert L.af_voice_spectrum_set_noise_override(h, pf, ps, 4, 3, 4, 0) == 0
    assert L.af_voice_spectrum_set_noise_override(h, pf, ps, 4, 0, 0, 1) == 0  # shared: one row, stream count and stride unused
    assert L.af_voice_spectrum_set_noise_override(h, pf, ps, 1, 3, 4, 0) == 0  # a single point is stored; analyze lets it fall through
    assert L.af_voice_spectrum_set_noise_override(h, None, None, 0, 0, 0, 0) == 0  # clear
    # a per-stream override for another stream count is refused before any device work
    from mic_eq_mi import _lib

    assert L.af_voice_spectrum_set_noise_override(h, pf, ps, 4, 3, 4, 0) == 0
    x = np.zeros((2, 1024), dtype=np.float32)
    out = _lib.VoiceSpectrumOutputs()
    rc = L.af_voice_spectrum_analyze_host(h, x.ctypes.data_as(C.POINTER(C.c_float)), 1024, 2, 1024, None, 0, None, 0, 0, C.byref(out))
    assert rc == INVALID and "3 streams" in L.af_last_error().decode()
    L.af_voice_spectrum_destroy(h)


def test_python_operators_exist_and_refuse():
    import mic_eq_mi

    for name in ("analyze_noise_reference", "analyze_noise_reference_batch", "analyze_voice_capture_batch", "analyze_voice_spectrum_batch"):
        fn = getattr(mic_eq_mi, name)
        assert callable(fn) and fn is not mic_eq_mi._missing_core and name in mic_eq_mi.__all__ and name in mic_eq_mi._OPERATORS
    for name in ("NoiseReference", "NoiseReferenceAnalysis", "CaptureMetadata"):
        assert name in mic_eq_mi.__all__ and getattr(mic_eq_mi, name) is not None
    x = np.zeros((2, 4000), dtype=np.float32)
    with pytest.raises(NotImplementedError, match="11025"):
        mic_eq_mi.analyze_noise_reference_batch(x, x, 11_025)
    with pytest.raises(ValueError, match="sample_rate must be positive"):
        mic_eq_mi.analyze_noise_reference(x[0], None, 0)
    with pytest.raises(ValueError, match=r"\[n_streams, n_noise\]"):
        mic_eq_mi.analyze_noise_reference_batch(x[0], None, 3000)
    with pytest.raises(ValueError, match="one value or one per stream"):
        mic_eq_mi.analyze_noise_reference_batch(x, x, 3000, noise_metadata=[{}, {}, {}])
    with pytest.raises(TypeError, match="capture metadata"):
        mic_eq_mi.analyze_noise_reference_batch(x, x, 3000, noise_metadata=[3, 4])
    nr = mic_eq_mi.NoiseReference(3000)
    with pytest.raises(ValueError, match="speech_audio"):
        nr.analyze(x, x[:1])
    with pytest.raises(ValueError, match="noise_vad_probabilities"):
        nr.analyze(x, x, noise_vad_probabilities=np.zeros((3, 5)))
    with pytest.raises(ValueError, match="capture_age_s"):
        nr.analyze(x, x, capture_age_s=[1.0])
    assert nr.frame_size == 600 and nr.frames(4000) == 12 and nr.bins(4000) == 301 and nr.bins(7) == 4
    assert np.array_equal(nr.frequencies(4000), np.fft.rfftfreq(600, 1.0 / 3000)) and np.array_equal(nr.frequencies(7), np.fft.rfftfreq(7, 1.0 / 3000))
    nr.close()
    vs = mic_eq_mi.VoiceSpectrum(48_000, 256)
    with pytest.raises(ValueError, match="noise_override"):
        vs.set_noise_override((np.arange(4.0), np.zeros(5)))
    vs.close()
    # the single-capture form keeps refusing the override
    with pytest.raises(NotImplementedError, match="noise_spectrum_override"):
        mic_eq_mi.analyze_voice_spectrum(np.zeros(8192, dtype=np.float32), noise_spectrum_override=(np.arange(4.0), np.zeros(4)))


def test_dataclasses_have_the_references_fields():
    import mic_eq_mi

    M, A = mic_eq_mi.CaptureMetadata, mic_eq_mi.NoiseReferenceAnalysis
    assert tuple(f.name for f in dataclasses.fields(M)) == ("captured_at_unix_s", "input_device", "sample_rate", "channel_mode", "channel_count")
    assert tuple(f.name for f in dataclasses.fields(A)) == ("status", "quality_score", "usable", "conservative", "reasons", "guidance", "metrics",
                                                            "frequencies", "explicit_spectrum_db", "conservative_spectrum_db",
                                                            "in_capture_spectrum_db", "conservative_noise_rms_db")
    assert M.coerce(None) == M() and M.coerce(M(input_device="a")).input_device == "a"
    m = M.coerce({"captured_at_unix_s": float("inf"), "input_device": "  ", "sample_rate": "48000", "channel_mode": " left ", "channel_count": 2.0})
    assert m == M(None, None, 48_000, "left", 2)
    with pytest.raises(dataclasses.FrozenInstanceError):
        m.sample_rate = 1
    z = np.zeros(3)
    a = A("usable", 0.9, True, False, ["r"], ["g"], {"duration_s": 2.0}, z, z, z)
    assert a.in_capture_spectrum_db is None and a.conservative_noise_rms_db == -120.0
    d = a.diagnostics()
    assert d == {"status": "usable", "quality_score": 0.9, "usable": True, "conservative": False, "reasons": ["r"], "guidance": ["g"],
                 "metrics": {"duration_s": 2.0}}
    assert d["reasons"] is not a.reasons and d["metrics"] is not a.metrics
