"""tests/ref/speech_features_ref.c (the kernels' arithmetic restated, with csrc/af_speech_features_math.h behind it) against what
the reference's _vad_masked_speech_features returned for the same stimuli (tests/golden/speech_features.npz, written by
tools/gen_golden_speech_features.py).  Counts, masks, indices and peak_hz are equal.  Continuous fields differ only by rounding:
NumPy sums pairwise and transforms with pocketfft, the restatement sums in the kernels' orders.  MEASURED holds the largest
difference seen per field family; the tests allow four times that (the convention of DESIGN 4.17-4.18), and the GPU tests add
the same allowance to their own bound.  Every test prints what it measured before it asserts."""
import functools

import numpy as np
import pytest

import speech_features_oracle as SO
import speech_features_stimulus as SS

SCALARS = ("active_duration_s", "active_ratio", "vad_active_frame_ratio", "short_term_lufs", "momentary_lufs",
           "active_loudness_spread_db", "loudness_range_db", "sibilance_excess_db", "band_low_db", "band_body_db", "band_presence_db",
           "band_sibilance_db", "confidence", "frame_probability_p90", "frame_probability_top_mean", "temporal_score",
           "absolute_hf_strength_p90", "noise_reliability_p90", "excess_p90_db", "temporal_contrast_db", "candidate_frame_ratio",
           "candidate_snr_db", "peak_hz")
COUNTS = ("frames", "active_frames", "spectral_frames", "vad_probability_used", "short_term_window_count", "loudness_window_count",
          "evidence_available")
FAMILY = dict.fromkeys(("active_duration_s", "active_ratio", "vad_active_frame_ratio", "peak_hz"), "exact")
FAMILY.update(dict.fromkeys(("short_term_lufs", "momentary_lufs", "active_loudness_spread_db", "loudness_range_db"), "loudness"))
FAMILY.update(dict.fromkeys(("sibilance_excess_db", "band_low_db", "band_body_db", "band_presence_db", "band_sibilance_db", "excess_p90_db",
                             "temporal_contrast_db", "candidate_snr_db", "frame_db"), "level_db"))
FAMILY.update(dict.fromkeys(("temporal_score", "absolute_hf_strength_p90", "noise_reliability_p90", "frame_feature_rows"), "feature"))
FAMILY.update(dict.fromkeys(("confidence", "frame_probability_p90", "frame_probability_top_mean", "candidate_frame_ratio",
                             "frame_probabilities"), "probability"))
# the largest |restatement - reference| per family over every stream of every batch, as measured by this file
MEASURED = {"exact": 0.0, "loudness": 1.1e-14, "level_db": 9.2e-14, "feature": 2.0e-13, "probability": 1.4e-14}
FRAME_STREAMS = (0, 1, 2, 64, 66)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's results for every stream of a batch, computed once and shared."""
    b = SS.batch(name)
    return [SO.analyze(b["speech"][s], b["noise_rms_db"][s], None if b["vad"] is None else b["vad"][s],
                       None if b["noise"] is None else b["noise"][s]) for s in range(b["speech"].shape[0])]


def compare_with_fixture(name, rows, per_frame, worst):
    """rows[s]: field -> value of stream s; per_frame(s, field) -> array.  Equal fields are asserted, the others fill `worst`."""
    fx = SS.fixture()
    counts, scalars = fx[f"{name}/counts"], fx[f"{name}/scalars"]
    for s, got in enumerate(rows):
        where = (name, s)
        if counts[s, 0] < 0:
            assert got["non_finite"] == 1, where
            continue
        assert got["non_finite"] == 0, where
        for j, field in enumerate(COUNTS):
            assert int(got[field]) == int(counts[s, j]), where + (field,)
        for j, field in enumerate(SCALARS):
            want = scalars[s, j]
            if np.isnan(want):  # a key the reference's dict does not have without evidence
                continue
            family = FAMILY[field]
            worst[family] = max(worst[family], abs(float(got[field]) - float(want)))
        if name == "main" and s in FRAME_STREAMS:
            assert np.array_equal(per_frame(s, "active_frame_mask").astype(bool), fx[f"main/{s}/active_frame_mask"]), where
            assert np.array_equal(per_frame(s, "frame_indices"), fx[f"main/{s}/frame_indices"]), where
            for field in ("frame_db", "frame_probabilities", "frame_feature_rows"):
                d = np.abs(per_frame(s, field) - fx[f"main/{s}/{field}"])
                worst[FAMILY[field]] = max(worst[FAMILY[field]], float(d.max()) if d.size else 0.0)


@pytest.mark.parametrize("name", list(SS.BATCHES))
def test_restatement_matches_the_reference_fixture(name):
    rows = restated(name)
    worst = dict.fromkeys(MEASURED, 0.0)
    compare_with_fixture(name, rows, lambda s, field: rows[s][field], worst)
    print(f"{name}: largest |restatement - reference|:", {k: f"{v:.3e}" for k, v in worst.items()})
    for family, value in worst.items():
        assert value <= 4 * MEASURED[family], (name, family, value)


def test_the_fixture_rests_on_the_conditions_its_generator_asserted():
    fx = SS.fixture()
    assert float(fx["nearest_decision"]) > SS.MARGIN and float(fx["runner_up"]) > 1e-9 and float(fx["floor_ratio"]) > 1e6
    assert list(fx["batches"]) == list(SS.BATCHES)


def test_frame_model_parameters_change_the_probabilities_only():
    b = SS.batch("one_window")
    base = SO.analyze(b["speech"][1], b["noise_rms_db"][1], b["vad"][1], b["noise"][1])
    model = np.array([-3.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    other = SO.analyze(b["speech"][1], b["noise_rms_db"][1], b["vad"][1], b["noise"][1], model=model)
    assert np.array_equal(base["frame_feature_rows"], other["frame_feature_rows"]) and base["momentary_lufs"] == other["momentary_lufs"]
    x = other["frame_feature_rows"]
    want = 1.0 / (1.0 + np.exp(-(model[0] + x @ model[1:])))
    assert np.max(np.abs(other["frame_probabilities"] - want)) < 1e-15
    assert not np.array_equal(base["frame_probabilities"], other["frame_probabilities"])


def test_a_capture_below_one_frame_is_refused():
    with pytest.raises(ValueError):
        SO.analyze(np.zeros(1919, dtype=np.float32), -60.0)
