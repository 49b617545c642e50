"""From two captures to settings the engine takes: recommend_voice_chain_batch on the six whole capture pairs of the stimulus
(the voice captures and posteriors of streams 0, 1, 2, 7, 33 and 66 of the main batch, each with 2 s of room tone) against what
the reference's analyze_voice_setup itself returned for them (tests/golden/speech_features.npz, chain/...: its native VAD helper
replaced by the stimulus' posteriors, its Auto-EQ optimiser left out), under its default arguments and under a custom dynamics
profile on another preset.  Then the recommended gate, de-esser and compressor dicts go unchanged into an Engine's setters and
one 0.5 s call on those settings returns finite audio.

Booleans, gate_mode and profile names are equal.  Numeric settings are within ALLOWED: 1e-12, plus four times what
tests/test_voice_setup_rules.py measured between restatement and reference for the rules on given inputs, plus what
tests/test_gpu_voice_reliability.py allows the inputs that come from the spectrum (the median spectrum, in dB, and
residual_confidence; no setting moves faster than any of its inputs: every slope of the rules is at most 1 in these units).
The test prints its largest difference before it asserts."""
import numpy as np
import pytest

import signals as S
import speech_features_stimulus as SS
from test_gpu_voice_reliability import FIXTURE_TOL
from test_voice_setup_rules import MEASURED_SETTINGS

pytestmark = pytest.mark.gpu

PROFILES = ("gentle", "balanced", "dense", "custom")
ALLOWED = 1e-12 + 4 * MEASURED_SETTINGS + FIXTURE_TOL["median_spectrum_db"] + FIXTURE_TOL["residual_confidence"]
KEYS = {"gate", "deesser", "compressor", "deesser_diagnostics", "compressor_diagnostics", "capture_confidence", "features"}


@pytest.fixture(scope="module")
def recommendations():
    import mic_eq_mi

    c = SS.chain_batch()
    return [mic_eq_mi.recommend_voice_chain_batch(c["noise"], c["speech"], SS.FS, vad_probabilities=c["vad"],
                                                  noise_vad_probabilities=c["noise_vad"], **arguments) for arguments in SS.CHAIN_ARGUMENTS]


def numbers_and_flags(rec):
    """The values of one pair in the order of the fixture's chain/<a>/numbers and chain/<a>/flags."""
    gate, de, co, diag, features = rec["gate"], rec["deesser"], rec["compressor"], rec["deesser_diagnostics"], rec["features"]
    numbers = [rec["capture_confidence"], rec["speech_floor_db"], rec["speech_body_db"], rec["speech_snr_db"], rec["conservative_noise_rms_db"],
               rec["noise_referenced_snr_db"], features["short_term_lufs"], features["loudness_range_db"], diag["sibilance_excess_db"],
               diag["peak_hz"], diag["detection_probability"], diag["frame_evidence_confidence"],
               gate["threshold_db"], gate["vad_threshold"], gate["vad_hold_time_ms"], gate["vad_pre_gain"], gate["gate_margin_db"],
               de["auto_amount"], de["low_cut_hz"], de["high_cut_hz"], de["ratio"], de["max_reduction_db"],
               co["threshold_db"], co["ratio"], co["attack_ms"], co["release_ms"], co["makeup_gain_db"], co["base_release_ms"],
               co["target_lufs"], co["target_p95_reduction_db"], co["peak_reduction_cap_db"], co["noise_reference_reliability"]]
    flags = [gate["gate_mode"], gate["auto_threshold_enabled"], de["enabled"], co["auto_makeup_enabled"]]
    return numbers, flags


def test_recommendations_match_the_references_analyze_voice_setup(recommendations):
    fx = SS.fixture()
    c = SS.chain_batch()
    for key in ("speech", "vad", "noise", "noise_vad"):
        assert str(fx[f"chain/{key}_sha256"]) == SS.fingerprint(c[key])["sha256"], key
    worst, where = 0.0, None
    for a, results in enumerate(recommendations):
        assert len(results) == len(SS.CHAIN_STREAMS)
        for i, rec in enumerate(results):
            assert set(rec) >= KEYS
            numbers, flags = numbers_and_flags(rec)
            assert [int(v) for v in flags] == fx[f"chain/{a}/flags"][i].tolist(), (a, i)
            assert rec["compressor"]["dynamics_intensity"] == PROFILES[int(fx[f"chain/{a}/profiles"][i])], (a, i)
            assert rec["noise_reference_status"] == str(fx[f"chain/{a}/status"][i]), (a, i)
            assert isinstance(rec["deesser"]["enabled"], bool) and isinstance(rec["gate"]["gate_mode"], int)
            assert rec["gate"]["gate_mode"] == 1 and rec["features"]["vad_probability_used"]
            d = np.abs(np.array(numbers) - fx[f"chain/{a}/numbers"][i])
            if d.max() > worst:
                worst, where = float(d.max()), (a, i, int(d.argmax()))
    print(f"largest |GPU - reference| over the recommended settings: {worst:.3e} at {where} (allowed {ALLOWED:.3e})")
    assert worst <= ALLOWED
    enabled = [rec["deesser"]["enabled"] for rec in recommendations[0]]
    makeup = [rec["compressor"]["auto_makeup_enabled"] for rec in recommendations[0]]
    assert any(enabled) and not all(enabled) and any(makeup) and not all(makeup)


def test_smoothing_of_given_spectra_is_the_windows_pass():
    """VoiceSpectrum.smooth (af_voice_spectrum_smooth_rows) against the restatement's smoothing, on the grid the operator uses and
    on a short one, at the bound tests/test_gpu_voice_spectrum.py holds the smoothed windows to (1e-12 dB)."""
    import voice_spectrum_oracle as VO
    from mic_eq_mi import mic_eq_core as core

    rng = np.random.default_rng(5)
    for nperseg, rows in ((4096, 3), (256, 70)):
        K = nperseg // 2 + 1
        db = -40.0 - 12.0 * np.log2(np.arange(1, K + 1) / 40.0)[None, :] * 0.3 + 3.0 * rng.standard_normal((rows, K))
        vs = core.VoiceSpectrum(SS.FS, nperseg)
        got, one = vs.smooth(db), vs.smooth(db[1])
        vs.close()
        want = np.stack([VO.smooth(row, SS.FS, nperseg) for row in db])
        worst = float(np.max(np.abs(got - want)))
        print(f"nperseg {nperseg}: largest |GPU - restatement| of the smoothing: {worst:.3e}")
        assert got.shape == db.shape and worst <= 1e-12 and np.array_equal(one, got[1])


def test_without_posteriors_the_energy_fallback_runs_and_the_gate_stays_vad_assisted():
    import mic_eq_mi

    c = SS.chain_batch()
    plain = mic_eq_mi.recommend_voice_chain_batch(c["noise"][:2], c["speech"][:2], SS.FS)
    off = mic_eq_mi.recommend_voice_chain_batch(c["noise"][:2], c["speech"][:2], SS.FS, vad_probabilities=c["vad"][:2], vad_available=False)
    for a, b in zip(plain, off):
        assert not a["features"]["vad_probability_used"] and a["gate"]["gate_mode"] == 1 and a["gate"]["auto_threshold_enabled"] is True
        assert not b["features"]["vad_probability_used"] and b["gate"]["gate_mode"] == 0 and b["gate"]["auto_threshold_enabled"] is False
        assert a["gate"]["threshold_db"] == b["gate"]["threshold_db"] and a["compressor"] == b["compressor"]  # the posteriors were ignored


def test_an_engine_takes_the_recommended_settings_and_runs(recommendations):
    from mic_eq_mi import mic_eq_core as core

    n_streams, n = 4, 24_000  # 0.5 s
    x = SS.chain_batch()["speech"][:n_streams, 40_000:40_000 + n]
    for rec in recommendations[0]:
        eng = core.Engine(float(SS.FS), n_streams)
        core.configure_auto_eq_chain(eng, float(SS.FS), S.LIMITER_BANDS, S.limiter_settings(2.0))
        eng.set_prefilter_enabled(1, 1)
        core.configure_voice_chain(eng, rec)  # every setter accepts its value: a refusal raises
        assert eng.engine_gate_enabled() == 1 and abs(eng.gate_threshold_db() - rec["gate"]["threshold_db"]) < 1e-9
        controls = eng.gate_vad_controls()
        assert controls["vad_threshold"] == float(np.float32(rec["gate"]["vad_threshold"]))  # the controller keeps f32
        assert controls["hold_ms"] == float(np.float32(rec["gate"]["vad_hold_time_ms"])) and controls["auto_threshold"] == rec["gate"]["auto_threshold_enabled"]
        got = eng.process(x)
        eng.close()
        assert got.shape == x.shape and np.all(np.isfinite(got))
