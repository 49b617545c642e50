"""verify_voice_setup_batch on whole captures (setup_verification_stimulus.run_batch(): the six chain pairs of the speech-feature
stimulus, each with a second passage and settings along the issue's table) against what the reference's own
validate_voice_setup_verification answered with the CPU oracle as its renderer (tests/golden/setup_verification.npz, runs/...).

Decisions, reasons, key sets, limiter_activity_events and clipped are equal.  Numbers:
  before side (no rendering): 1e-12 (kernels against the restatement) + 4 x MEASURED of tests/test_setup_verification_ref.py
    (restatement against the reference) + what the analyses in front are allowed: the shape error is an RMS of centred
    differences of the median spectrum, so it moves by at most twice a bin's deviation, 2 x (1e-12 + 4 x 2.984e-13)
    (tests/test_gpu_voice_reliability.py with tests/test_voice_reliability_ref.py's MEASURED); the loudness spread is a speech
    feature of the loudness family, 1e-12 + 4 x 1.1e-14 (tests/test_gpu_speech_features.py).
  levels: _rms_db twice, 2 x (1e-12 + 4 x 1.8e-15).
  snr_change_db: snr_db twice; per side 1e-12 (1 + P / (P - N)) <= 3e-12 while the speech is 3 dB over the noise, + 4 x 5.684e-14.
  band medians of the spectral SNR: a median moves by at most a bin's deviation, 1e-12 x 100 (the amplification of the SNR formula
    for bins at least 0.05 dB over the noise) + 4 x 1.027e-10.
  after side: the same plus the CHAIN TERM, what the engine's float32 rendering against the oracle's moves each field, measured
    on an MI355X per field as |operator on the oracle's render - operator on the engine's render| over these cases: the rendered
    audio came out bit-equal, so every audio-derived field and every gain-reduction statistic measured 0; the two fields that read
    the float32 level keys of the simulation dict measured relative_noise_floor_change_db 3.815e-6 and output_true_peak_db
    1.907e-6.  The bound is four times the measurement.
The smallest distance of a compared quantity from its threshold over the cases is 0.15 dB (runs/margins), more than ten times
the largest bound here.

Also: one stream alone gives the bytes it gives inside the batch; validate_voice_setup_verification equals row 0; a stream that
exits early ("clipped") does not stop the batch; the short passage exits as the reference's.  (The room tones are rendered in a
call of their own, so there is no joint render to compare with.)"""
import pathlib

import numpy as np
import pytest

import setup_verification_stimulus as SV
from test_setup_verification_ref import MEASURED

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "setup_verification.npz"
NUMBERS = ("spectral_target_error_before_db", "spectral_target_error_after_db", "loudness_variation_before_db",
           "loudness_variation_after_db", "noise_floor_change_db", "relative_noise_floor_change_db", "snr_change_db",
           "compressor_gain_reduction_median_db", "compressor_gain_reduction_p95_db", "compressor_gain_reduction_peak_db",
           "deesser_gain_reduction_median_db", "deesser_gain_reduction_p95_db", "output_true_peak_db")
BANDS = ("low", "body", "presence", "sibilance")
CHAIN_TERM = {"relative_noise_floor_change_db": 3.815e-6, "output_true_peak_db": 1.907e-6}  # measured; every other field: 0
SHAPE = 1e-12 + 4 * MEASURED["shape_error_db"] + 2 * (1e-12 + 4 * 2.984e-13)
LOUDNESS = 1e-12 + 4 * 1.1e-14
LEVELS = 2 * (1e-12 + 4 * MEASURED["rms_db"])
ALLOWED = {"spectral_target_error_before_db": SHAPE, "spectral_target_error_after_db": SHAPE, "loudness_variation_before_db": LOUDNESS,
           "loudness_variation_after_db": LOUDNESS, "noise_floor_change_db": LEVELS,
           "relative_noise_floor_change_db": LEVELS + 4 * CHAIN_TERM["relative_noise_floor_change_db"],
           "snr_change_db": 2 * (3e-12 + 4 * 5.684e-14), "compressor_gain_reduction_median_db": 0.0,
           "compressor_gain_reduction_p95_db": 0.0, "compressor_gain_reduction_peak_db": 0.0, "deesser_gain_reduction_median_db": 0.0,
           "deesser_gain_reduction_p95_db": 0.0, "output_true_peak_db": 4 * CHAIN_TERM["output_true_peak_db"]}
BAND_ALLOWED = 1e-12 * 100 + 4 * 1.027e-10


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def batch():
    return SV.run_batch()


@pytest.fixture(scope="module")
def results(batch):
    import mic_eq_mi

    return mic_eq_mi.verify_voice_setup_batch(batch["noise"], batch["original"], batch["verification"], SV.FS, batch["setups"], batch["presets"])


def test_decisions_reasons_keys_and_flags_equal_the_references(golden, results):
    assert golden["runs/names"].tolist() == [c[0] for c in SV.RUN_CASES]
    decisions = golden["runs/decisions"].tolist()
    assert all(decisions.count(d) >= 2 for d in ("accept", "reduce", "rollback", "retry"))
    for k, got in enumerate(results):
        name = SV.RUN_CASES[k][0]
        assert got["decision"] == decisions[k] and got["reasons"] == [str(golden["runs/reasons"][k])], name
        assert sorted(got) == str(golden["runs/keys"][k]).split("|"), name
        if "snr_change_db" in got:
            assert [got["limiter_activity_events"], int(got["clipped"])] == golden["runs/flags"][k].tolist(), name
            assert got["simulation_backend"] == "rust" and got["perceptual_validation"] is False
    assert results[9] == {"decision": "retry", "reasons": ["verification passage was non-finite or clipped"], "perceptual_validation": False}
    assert results[2]["limiter_activity_events"] > 0 and results[3]["limiter_activity_events"] > 0


def test_numbers_are_within_the_bounds(golden, results):
    worst = dict.fromkeys(NUMBERS + ("bands",), 0.0)
    for k, got in enumerate(results):
        if "snr_change_db" not in got:
            continue
        for j, key in enumerate(NUMBERS):
            worst[key] = max(worst[key], abs(got[key] - float(golden["runs/numbers"][k][j])))
        want = {name: float(v) for name, v in zip(BANDS, golden["runs/bands"][k]) if not np.isnan(v)}
        assert set(got["frequency_dependent_snr_db"]) == set(want)
        for name, value in want.items():
            worst["bands"] = max(worst["bands"], abs(got["frequency_dependent_snr_db"][name] - value))
    for key, value in worst.items():
        print(f"largest |operator - reference| {key}: {value:.3e} (allowed {BAND_ALLOWED if key == 'bands' else ALLOWED[key]:.3e})")
    assert float(np.nanmin(golden["runs/margins"])) >= 10 * max(max(ALLOWED.values()), BAND_ALLOWED)
    for key in NUMBERS:
        assert worst[key] <= ALLOWED[key], (key, worst[key])
    assert worst["bands"] <= BAND_ALLOWED


def test_one_stream_alone_equals_its_row_in_the_batch(batch, results):
    import mic_eq_mi

    for k in (0, 6):  # an accepted stream, and the one with the caller's EQ
        alone = mic_eq_mi.verify_voice_setup_batch(batch["noise"][k:k + 1], batch["original"][k:k + 1], batch["verification"][k:k + 1],
                                                   SV.FS, [batch["setups"][k]], [batch["presets"][k]])
        assert alone[0] == results[k], SV.RUN_CASES[k][0]
    single = mic_eq_mi.validate_voice_setup_verification(batch["noise"][0], batch["original"][0], batch["verification"][0], SV.FS,
                                                         batch["setups"][0], batch["presets"][0])
    assert single == results[0]
    short = mic_eq_mi.validate_voice_setup_verification(batch["noise"][0], batch["original"][0], batch["verification"][0][:SV.SHORT_SAMPLES],
                                                        SV.FS, batch["setups"][0], "broadcast")
    assert short == {"decision": "retry", "reasons": ["verification passage was too short"], "perceptual_validation": False}
