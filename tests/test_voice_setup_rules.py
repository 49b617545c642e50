"""The recommendation rules (csrc/af_voice_setup_math.h, reached through tests/ref/speech_features_ref.c and through the
library's af_voice_setup_recommend) against what the reference's _recommend_gate_settings, _recommend_deesser_settings and
_recommend_compressor_settings returned for the main batch of the stimulus on its made-up spectrum inputs
(tests/golden/speech_features.npz).  Booleans, gate_mode and profiles are equal.  Numeric settings differ only by the rounding
of the features they are computed from and of NumPy's pairwise band means; MEASURED_SETTINGS is the largest difference seen,
and four times that is allowed.  No GPU is needed: the rules run on the host."""
import numpy as np
import pytest

import speech_features_oracle as SO
import speech_features_stimulus as SS
from test_speech_features_ref import restated

NUMBERS = ("speech_floor_db", "speech_body_db", "speech_frame_peak_db", "speech_snr_db", "snr_confidence", "capture_confidence",
           "gate_threshold_db", "gate_vad_threshold", "gate_vad_hold_time_ms", "gate_vad_pre_gain", "gate_margin_db",
           "deesser_auto_amount", "deesser_low_cut_hz", "deesser_high_cut_hz", "deesser_ratio", "deesser_max_reduction_db",
           "deesser_sibilance_excess_db", "deesser_peak_hz", "deesser_frame_evidence_confidence", "deesser_detection_probability",
           "compressor_threshold_db", "compressor_ratio", "compressor_attack_ms", "compressor_release_ms", "compressor_makeup_gain_db",
           "compressor_base_release_ms", "compressor_target_lufs", "compressor_target_p95_db", "compressor_target_median_db",
           "compressor_peak_cap_db", "compressor_noise_reference_reliability")
FLAGS = ("gate_mode", "gate_auto_threshold_enabled", "deesser_enabled", "deesser_frame_evidence_available", "deesser_invalid_evidence",
         "compressor_auto_makeup_enabled", "compressor_profile")
MEASURED_SETTINGS = 1.2e-13  # the largest |restatement - reference| over every numeric setting of every stream, as measured here


def compare(rows, worst=0.0):
    fx = SS.fixture()
    for s, got in enumerate(rows):
        for j, field in enumerate(FLAGS):
            assert int(got[field]) == int(fx["main/setup_flags"][s, j]), (s, field)
        for j, field in enumerate(NUMBERS):
            worst = max(worst, abs(float(got[field]) - float(fx["main/setup_numbers"][s, j])))
        worst = max(worst, float(np.max(np.abs(np.asarray(got["deesser_clip_features"]) - fx["main/setup_clip_features"][s]))))
    return worst


def test_rules_match_the_reference_fixture():
    rows = [SO.recommend(r, **SS.setup_inputs(s)) for s, r in enumerate(restated("main"))]
    worst = compare(rows)
    print(f"largest |restatement - reference| over the recommended settings: {worst:.3e}")
    assert worst <= 4 * MEASURED_SETTINGS
    fx = SS.fixture()
    flags = fx["main/setup_flags"]
    assert set(flags[:, 2]) == {0, 1} and {(p, m) for p, m in zip(flags[:, 6], flags[:, 5])} == {(p, m) for p in range(4) for m in (0, 1)}
    assert float(fx["setup_nearest_decision"]) > SS.MARGIN


def test_the_library_entry_gives_the_restatements_bits():
    """af_voice_setup_recommend is the same text behind an argument check: equal fields, through the Python operator."""
    import mic_eq_mi

    rows = restated("main")
    features = {name: np.array([r[name] for r in rows]) for name, _ in SO.Row._fields_}
    features["frame_db"] = np.stack([r["frame_db"] for r in rows])
    features["active_frame_mask"] = np.stack([r["active_frame_mask"] for r in rows])
    for s in (0, 1, 2, 7, 33, 66):
        k = SS.setup_inputs(s)
        want = SO.recommend(rows[s], **k)
        got = mic_eq_mi.recommend_voice_chain(features, s, k.pop("freqs"), k.pop("smoothed_spectrum_db"), **k)
        assert set(got) >= {"gate", "deesser", "compressor", "deesser_diagnostics", "compressor_diagnostics", "capture_confidence"}
        assert got["capture_confidence"] == want["capture_confidence"] and got["speech_body_db"] == want["speech_body_db"]
        gate, de, co, diag = got["gate"], got["deesser"], got["compressor"], got["deesser_diagnostics"]
        assert set(gate) == {"enabled", "threshold_db", "attack_ms", "release_ms", "gate_mode", "vad_threshold", "vad_hold_time_ms",
                             "vad_pre_gain", "auto_threshold_enabled", "gate_margin_db"}
        assert set(de) == {"enabled", "auto_enabled", "auto_amount", "low_cut_hz", "high_cut_hz", "threshold_db", "ratio", "attack_ms",
                           "release_ms", "max_reduction_db"}
        assert gate["threshold_db"] == want["gate_threshold_db"] and gate["gate_mode"] == want["gate_mode"] and isinstance(gate["gate_mode"], int)
        assert de["enabled"] is bool(want["deesser_enabled"]) and de["high_cut_hz"] == want["deesser_high_cut_hz"]
        assert diag["detection_probability"] == want["deesser_detection_probability"] and diag["peak_hz"] == want["deesser_peak_hz"]
        assert list(diag["clip_features"].values()) == list(want["deesser_clip_features"])
        assert co["ratio"] == want["compressor_ratio"] and co["dynamics_intensity"] == SO.PROFILES[want["compressor_profile"]]
        assert co["auto_makeup_enabled"] is bool(want["compressor_auto_makeup_enabled"]) and co["makeup_gain_db"] == want["compressor_makeup_gain_db"]
        assert got["compressor_diagnostics"]["target_median_reduction_db"] == want["compressor_target_median_db"]


def test_enable_threshold_is_a_parameter_and_unknown_names_fall_back():
    r = restated("main")[1]
    k = SS.setup_inputs(1)
    k["noise_status"] = "usable"
    base = SO.recommend(r, **k)
    assert base["deesser_enabled"] == 1 and base["deesser_detection_probability"] < 0.99
    assert SO.recommend(r, **k, enable_probability_threshold=0.99)["deesser_enabled"] == 0
    assert SO.recommend(r, **dict(k, noise_status="invalid"))["deesser_enabled"] == 0  # invalid evidence, :563-567
    other = SO.recommend(r, **dict(k, dynamics_intensity="no such profile", target_preset="no such preset"))
    assert other["compressor_profile"] == 1 and other["compressor_target_lufs"] == -18.0
    assert SO.recommend(r, **dict(k, vad_available=False))["gate_mode"] == 0


def test_argument_contract_of_the_library_entry():
    import ctypes as C

    from mic_eq_mi import _lib

    L = _lib.load()
    inputs, out = _lib.VoiceSetupInputs(), _lib.VoiceSetupRecommendation()
    L.af_voice_setup_default_inputs(C.byref(inputs))
    assert (inputs.vad_available, inputs.dynamics_intensity, inputs.target_lufs) == (1, 1, -16.0)
    assert (inputs.custom_target_p95_db, inputs.custom_peak_cap_db, inputs.enable_probability_threshold) == (3.5, 8.0, 0.4935253581578833)
    assert L.af_voice_setup_recommend(None, C.byref(out)) == -1 and L.af_voice_setup_recommend(C.byref(inputs), None) == -1
    assert L.af_voice_setup_recommend(C.byref(inputs), C.byref(out)) == -1 and "required" in L.af_last_error().decode()
    with pytest.raises(ValueError, match="equal-length"):
        import mic_eq_mi

        rows = restated("one_window")
        features = {name: np.array([r[name] for r in rows]) for name, _ in SO.Row._fields_}
        features.update(frame_db=np.stack([r["frame_db"] for r in rows]), active_frame_mask=np.stack([r["active_frame_mask"] for r in rows]))
        mic_eq_mi.recommend_voice_chain(features, 0, np.arange(4.0), np.zeros(5), residual_confidence=0.5, snr_db=12.0,
                                        used_single_spectrum_fallback=False, noise_quality_score=0.9, noise_status="usable",
                                        conservative_noise_rms_db=-60.0)
