"""CPU checks of the second-passage measurements' boundary: the symbols and their ctypes signatures, the argument errors that
come before any GPU work, and the Python operator's argument contract.  No device is touched."""
import ctypes as C

import numpy as np
import pytest

import setup_verification_oracle as O


@pytest.fixture(scope="module")
def L():
    from mic_eq_mi import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def lib_module():
    from mic_eq_mi import _lib

    return _lib


def _create(L, rate=48_000, nperseg=2048, streams=4, device=0):
    handle = C.c_void_p()
    return L.af_setup_verification_create(rate, nperseg, streams, device, C.byref(handle)), handle


def test_symbols_signatures_and_version(L, lib_module):
    for name in ("af_setup_verification_create", "af_setup_verification_destroy", "af_setup_verification_measure_host",
                 "af_setup_verification_measure_device"):
        assert name in lib_module.SIGNATURES and hasattr(L, name)
    assert L.af_version() >= 101
    assert C.sizeof(lib_module.SetupVerificationRow) == 344 == O.ROW_DTYPE.itemsize
    assert [n for n, _ in lib_module.SetupVerificationRow._fields_] == [n for n, _ in O.Row._fields_]
    assert C.sizeof(lib_module.SetupVerificationAudio) == 32
    assert lib_module.TARGET_PRESETS == O.PRESETS and lib_module.SETUP_SIGNALS == O.SIGNALS


def test_create_argument_errors(L, lib_module):
    rc, _ = _create(L, rate=44_100)
    assert rc == lib_module.AF_ERR_UNSUPPORTED and "48000" in lib_module.last_error()
    with pytest.raises(NotImplementedError):
        lib_module.check(rc)
    for kwargs in (dict(nperseg=2047), dict(nperseg=0), dict(streams=0), dict(device=-1)):
        rc, _ = _create(L, **kwargs)
        assert rc == lib_module.AF_ERR_INVALID_ARGUMENT, kwargs
    rc, _ = _create(L, nperseg=32_768)
    assert rc == lib_module.AF_ERR_UNSUPPORTED
    assert L.af_setup_verification_create(48_000, 2048, 4, 0, None) == lib_module.AF_ERR_INVALID_ARGUMENT
    L.af_setup_verification_destroy(None)  # a null handle is fine, as free(NULL)


def test_measure_argument_errors_come_before_any_gpu_work(L, lib_module):
    rc, h = _create(L)
    assert rc == 0
    bins, B = 1025, 4
    spectra = np.zeros((B, bins))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    d = spectra.ctypes.data_as(dp)
    presets = np.zeros(B, dtype=np.int32)
    p = presets.ctypes.data_as(ip)
    audio = (lib_module.SetupVerificationAudio * 5)()
    rows = (lib_module.SetupVerificationRow * B)()
    x = np.zeros((B, 100), dtype=np.float32)

    def host(handle=h, n=B, a=d, b=d, c=d, stride=bins, snr=None, snr_stride=bins, ids=p, signals=audio, out=rows):
        return L.af_setup_verification_measure_host(handle, n, a, b, c, stride, snr, snr_stride, ids, signals, out)

    bad = lib_module.AF_ERR_INVALID_ARGUMENT
    assert host(handle=None) == bad
    assert host(n=0) == bad and host(n=5) == bad
    assert host(a=None) == bad and host(b=None) == bad and host(c=None) == bad
    assert host(stride=bins - 1) == bad
    assert host(snr=d, snr_stride=bins - 1) == bad
    assert host(ids=None) == bad and host(signals=None) == bad and host(out=None) == bad
    presets[2] = 4
    assert host() == bad and "Unknown target preset: 4" in lib_module.last_error()
    presets[2] = -1
    assert host() == bad
    presets[2] = 0
    audio[2].samples, audio[2].stride, audio[2].length = x.ctypes.data, 99, 100
    assert host() == bad and "stride" in lib_module.last_error()
    audio[2].stride = 100
    lengths = np.array([100, 0, 101, 5], dtype=np.int64)
    audio[2].lengths = lengths.ctypes.data_as(C.POINTER(C.c_int64))
    assert host() == bad and "stream 2" in lib_module.last_error()
    lengths[2] = -1
    assert host() == bad
    # the device entry point runs the same checks first
    assert L.af_setup_verification_measure_device(h, B, None, None, None, bins, None, bins, p, audio, None, None) == bad
    L.af_setup_verification_destroy(h)


def test_python_argument_contract():
    import mic_eq_mi
    from mic_eq_mi import setup_verification as SV

    assert callable(mic_eq_mi.measure_setup_verification_batch) and mic_eq_mi.measure_setup_verification_batch is not mic_eq_mi._missing_core
    assert mic_eq_mi.SetupVerification is SV.SetupVerification
    assert SV.ROW_DTYPE == O.ROW_DTYPE
    with pytest.raises(ValueError, match="Unknown target preset: warm"):
        SV.preset_ids("warm", 2)
    with pytest.raises(ValueError, match="one per stream"):
        SV.preset_ids(["flat"], 2)
    assert SV.preset_ids(["flat", "podcast"], 2).tolist() == [3, 1]
    with pytest.raises(NotImplementedError):
        SV.SetupVerification(44_100, 2048, 4)
    with pytest.raises(NotImplementedError):
        SV.measure_setup_verification_batch(np.zeros((1, 1025)), np.zeros((1, 1025)), np.zeros((1, 1025)), 44_100, "flat")
    h = SV.SetupVerification(48_000, 2048, 4)
    spectra = np.zeros((2, 1025))
    with pytest.raises(ValueError, match="three spectra"):
        h.measure(spectra, spectra, np.zeros((2, 1024)), "flat")
    with pytest.raises(ValueError, match="spectral SNR"):
        h.measure(spectra, spectra, spectra, "flat", np.zeros((1, 1025)))
    with pytest.raises(ValueError, match="Unknown target preset"):
        h.measure(spectra, spectra, spectra, ["flat", "bright"])
    with pytest.raises(ValueError, match="2 streams of audio"):
        h.measure(spectra, spectra, spectra, "flat", verification=np.zeros((3, 10), dtype=np.float32))
    with pytest.raises(ValueError, match="n_streams"):
        h.measure(np.zeros((5, 1025)), np.zeros((5, 1025)), np.zeros((5, 1025)), "flat")
    h.close()
    h.close()


def test_python_rules_operator_returns_the_references_dicts():
    """decide_voice_setup_verification on the hand-made cases: the reference's decisions, reasons, key sets and numbers."""
    import pathlib

    import mic_eq_mi
    import setup_verification_rules_stimulus as RS
    from mic_eq_mi import setup_verification as SV

    golden = np.load(pathlib.Path(__file__).resolve().parent / "golden" / "setup_verification.npz")
    for index, (name, overrides, _) in enumerate(RS.CASES):
        c = RS.case(overrides)
        row = np.zeros(1, dtype=SV.ROW_DTYPE)[0]
        for k, signal in enumerate(O.SIGNALS):
            row["rms_db"][k] = c["rms"][signal]
        peak = float(np.float32(c["peak"]))
        row["non_finite"][2], row["clipped_0999"][2] = int(c["non_finite"]), int(peak >= 0.999)
        row["clipped_1"][3] = int(float(np.float32(c["rendered_peak"])) >= 1.0)
        row["spectral_target_error_before_db"], row["spectral_target_error_after_db"] = c["error_before"], c["error_after"]
        row["shape_delta_db"] = c["shape_delta"]
        got = mic_eq_mi.decide_voice_setup_verification(
            row, dict(c["sim"], simulation_backend=c["backend"]), {"compressor_settings": c["compressor"], "deesser_settings": c["deesser"]},
            verification_samples=c["samples"], before_snr_db=c["snr_before"], after_snr_db=c["snr_after"],
            loudness_variation_before_db=c["spread_before"], loudness_variation_after_db=c["spread_after"])
        assert got["decision"] == str(golden["rules/decisions"][index]), name
        assert got["reasons"] == [str(golden["rules/reasons"][index])], name
        assert sorted(got) == str(golden["rules/keys"][index]).split("|"), name
        if "snr_change_db" in got:
            assert [got[key] for key in RS.NUMBER_KEYS] == golden["rules/numbers"][index].tolist(), name
            assert [got["limiter_activity_events"], int(got["clipped"])] == golden["rules/flags"][index].tolist(), name
    # a recommend_voice_chain_batch record names its settings `compressor` and `deesser`
    c = RS.case({"sim": {"compressor_gain_reduction_p95_db": 6.0}})
    row = np.zeros(1, dtype=SV.ROW_DTYPE)[0]
    for k, signal in enumerate(O.SIGNALS):
        row["rms_db"][k] = c["rms"][signal]
    kwargs = dict(verification_samples=c["samples"], before_snr_db=30.0, after_snr_db=29.0, loudness_variation_before_db=1.0,
                  loudness_variation_after_db=1.0)
    sim = dict(c["sim"], simulation_backend="rust")
    assert mic_eq_mi.decide_voice_setup_verification(row, sim, {"compressor": {"target_p95_reduction_db": 5.5}}, **kwargs)["decision"] == "accept"
    assert mic_eq_mi.decide_voice_setup_verification(row, sim, {"compressor": {}}, **kwargs)["decision"] == "reduce"


def test_verify_operator_argument_contract_needs_no_device():
    import mic_eq_mi

    x = np.zeros((2, 200_000), dtype=np.float32)
    for fn in (mic_eq_mi.verify_voice_setup_batch, mic_eq_mi.validate_voice_setup_verification):
        assert callable(fn) and fn is not mic_eq_mi._missing_core
    with pytest.raises(NotImplementedError):
        mic_eq_mi.verify_voice_setup_batch(x, x, x, 44_100, {}, "flat")
    with pytest.raises(ValueError, match="expected noise"):
        mic_eq_mi.verify_voice_setup_batch(x[:1], x, x, 48_000, {}, "flat")
    with pytest.raises(ValueError, match="one per stream"):
        mic_eq_mi.verify_voice_setup_batch(x, x, x, 48_000, [{}], "flat")
    with pytest.raises(ValueError, match="Unknown target preset: warm"):
        mic_eq_mi.verify_voice_setup_batch(x, x, x, 48_000, {}, "warm")
    with pytest.raises(ValueError, match="10 frequencies"):
        mic_eq_mi.verify_voice_setup_batch(x, x, x, 48_000, {"eq_settings": {"band_freqs": [100.0]}}, "flat")
    early = {"decision": "retry", "reasons": ["verification passage was too short"], "perceptual_validation": False}
    assert mic_eq_mi.verify_voice_setup_batch(x, x, x[:, :143_999], 48_000, {}, "flat") == [early, early]  # :1484, before any GPU work
    assert mic_eq_mi.validate_voice_setup_verification(x[0], x[0], x[0, :100_000], 48_000, {}, "flat") == early


def test_offline_validation_symbols_and_the_keyword_defaults_to_off(L, lib_module):
    import inspect

    import mic_eq_mi

    for name in ("af_setup_offline_validation", "af_setup_offline_reason_text", "af_setup_verification_decide"):
        assert name in lib_module.SIGNATURES and hasattr(L, name)
    assert C.sizeof(lib_module.SetupOfflineInputs) == 152 and C.sizeof(lib_module.SetupOfflineResult) == 64
    bad = lib_module.AF_ERR_INVALID_ARGUMENT
    i, r = lib_module.SetupOfflineInputs(), lib_module.SetupOfflineResult()
    assert L.af_setup_offline_validation(None, C.byref(r)) == bad and L.af_setup_offline_validation(C.byref(i), None) == bad
    assert L.af_setup_offline_validation(C.byref(i), C.byref(r)) == 0
    assert not r.offline_validation_passed and not r.apply_recommended and r.weak_capture  # nothing simulated, nothing measured
    assert L.af_setup_offline_reason_text(5) == b"Auto-EQ abstained from this capture" and L.af_setup_offline_reason_text(6) is None
    parameter = inspect.signature(mic_eq_mi.recommend_voice_chain_batch).parameters["offline_validation"]
    assert parameter.default is False and parameter.kind is inspect.Parameter.KEYWORD_ONLY
