"""The stimuli of tests/voice_reliability_stimulus.py are the arrays tools/gen_golden_voice_reliability.py ran the reference
over, and the conditions the parity tests rest on hold in the fixture it wrote."""
import numpy as np

import voice_reliability_stimulus as RS
import voice_spectrum_stimulus as VS

MARGIN_DB = 1e-6


def test_stimuli_have_the_fixtures_fingerprints():
    fx = RS.fixture()
    cases = RS.cases()
    assert [c["name"] for c in cases] == list(fx["cases"])
    for case in cases:
        one = RS.fixture_case(case["name"])
        audio = case["audio"][RS.fixture_streams(case)]
        frames = (audio.shape[1] - case["nperseg"]) // (case["nperseg"] // 2) + 1
        assert tuple(one["shape"]) == audio.shape + (case["nperseg"], frames), case["name"]
        assert np.array_equal(one["streams"], RS.fixture_streams(case)), case["name"]
        assert VS.fingerprint(audio)["sha256"] == str(one["sha256"]), case["name"]


def test_long_batch_is_three_streams_of_199_frames():
    audio = RS.long_batch()
    assert audio.shape == (3, 100 * 256 + 37) and (audio.shape[1] - 256) // 128 + 1 == 199 and audio.dtype == np.float32


def test_the_generators_conditions_hold_in_the_fixture():
    effective = RS.SCALARS.index("effective_measurement_blocks")
    nearest, at_least_12, fractional, closest, clamp = np.inf, 0, 0, 0, 0
    for case in RS.cases():
        fx = RS.fixture_case(case["name"])
        full = list(fx["full_streams"])
        for i in range(fx["scalars"].shape[0]):
            if fx["flags"][i, 0]:  # the fallback return: none of the second half's decisions
                assert np.isnan(fx["distance"][i]).all() and not fx["inlier_mask"][i].any()
                continue
            voiced = fx["voiced_mask"][i].astype(bool)
            assert np.array_equal(np.isnan(fx["distance"][i]), ~voiced)
            nearest = min(nearest, RS.cutoff_margin(fx["distance"][i][voiced]))
            eff = fx["scalars"][i, effective]
            at_least_12 += eff >= 12.0
            fractional += eff != round(eff)
            closest += int(fx["counts"][i, 4])
            snr = fx["full_spectra"][full.index(i), 3] if i in full else fx["checkpoints"][i, 3]
            clamp += bool(np.any(snr == -60.0))
    assert nearest > MARGIN_DB and nearest == float(RS.fixture()["nearest_cutoff_db"])
    assert at_least_12 >= 1 and fractional >= 4 and closest >= 2 and clamp >= 1, (at_least_12, fractional, closest, clamp)
