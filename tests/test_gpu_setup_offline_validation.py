"""recommend_voice_chain_batch(offline_validation=True) on the six chain pairs of tests/speech_features_stimulus.py, under the two
argument sets of the chain fixture, without EQ settings and with the caller's EQ of tests/setup_verification_stimulus.py, against
the diagnostics of the reference's own analyze_voice_setup (tests/golden/setup_verification.npz, offline/...; its Auto-EQ call
raised or handed the caller's EQ back, its simulate_candidate_chain was the CPU oracle).

Flags (weak_capture, apply_recommended, offline_validation_passed) and the whole uncertainty_reasons lists are equal.  The
confidences are within the bound tests/test_gpu_voice_chain_recommendation.py holds the recommended settings to (they are
Lipschitz maps of the same inputs with constants below 1, and a weighted geometric mean of values in [0.03, 1]).  Without the
keyword the return is what it is today.  A recommendation goes into an engine through configure_voice_chain, and
verify_voice_setup_batch on a second passage gives the reference's decisions for its own recommendation, "accept" among them."""
import pathlib

import numpy as np
import pytest

import setup_verification_stimulus as SV
import signals as S
import speech_features_stimulus as SS
from test_gpu_voice_chain_recommendation import ALLOWED

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "setup_verification.npz"
NUMBERS = ("setup_confidence", "recommendation_uncertainty", "capture_confidence", "eq_confidence", "gate_confidence",
           "deesser_confidence", "compressor_confidence")
KEYS = {"setup_confidence", "recommendation_uncertainty", "confidence_semantics", "uncertainty_reasons", "weak_capture", "apply_recommended",
        "capture_confidence", "eq_confidence", "gate_confidence", "deesser_confidence", "compressor_confidence", "offline_validation_passed",
        "offline_validation"}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def chain():
    return SS.chain_batch()


def _recommend(c, arguments, **more):
    import mic_eq_mi

    return mic_eq_mi.recommend_voice_chain_batch(c["noise"], c["speech"], SS.FS, vad_probabilities=c["vad"],
                                                 noise_vad_probabilities=c["noise_vad"], **arguments, **more)


@pytest.fixture(scope="module")
def flat_records(chain):
    return [_recommend(chain, arguments, offline_validation=True) for arguments in SS.CHAIN_ARGUMENTS]


def _compare(golden, records, a, mode):
    worst = 0.0
    for s, rec in enumerate(records):
        d = rec["diagnostics"]
        assert set(d) == KEYS and d["confidence_semantics"] == "bounded_quality_score"
        assert [int(d["weak_capture"]), int(d["apply_recommended"]), int(d["offline_validation_passed"])] == golden[f"offline/{a}/{mode}/flags"][s].tolist(), (a, mode, s)
        assert d["uncertainty_reasons"] == [r for r in str(golden[f"offline/{a}/{mode}/reasons"][s]).split("|") if r], (a, mode, s)
        assert d["offline_validation"]["simulation_backend"] == "rust"
        for key, want in zip(NUMBERS, golden[f"offline/{a}/{mode}/numbers"][s]):
            worst = max(worst, abs(d[key] - float(want)))
    return worst


def test_diagnostics_without_eq_settings_match_the_references(golden, flat_records):
    worst = max(_compare(golden, records, a, "flat") for a, records in enumerate(flat_records))
    print(f"largest |GPU - reference| over the confidences, flat bands: {worst:.3e} (allowed {ALLOWED:.3e})")
    assert all("Auto-EQ abstained from this capture" in rec["diagnostics"]["uncertainty_reasons"] for rec in flat_records[0])
    assert worst <= ALLOWED


def test_diagnostics_with_the_callers_eq_match_the_references(golden, chain):
    eq = [SV.offline_eq(s) for s in range(chain["speech"].shape[0])]
    worst, seen = 0.0, set()
    for a, arguments in enumerate(SS.CHAIN_ARGUMENTS):
        records = _recommend(chain, arguments, offline_validation=True, eq_settings=eq)
        worst = max(worst, _compare(golden, records, a, "eq"))
        for s, rec in enumerate(records):
            assert rec["diagnostics"]["eq_confidence"] == eq[s]["analysis_confidence"]
            seen.update({("apply", rec["diagnostics"]["apply_recommended"]), ("passed", rec["diagnostics"]["offline_validation_passed"])})
    print(f"largest |GPU - reference| over the confidences, caller's EQ: {worst:.3e} (allowed {ALLOWED:.3e})")
    assert worst <= ALLOWED and ("apply", True) in seen and ("apply", False) in seen


def test_without_the_keyword_the_return_is_todays(chain, flat_records):
    plain = _recommend(chain, SS.CHAIN_ARGUMENTS[0])
    for base, rec in zip(plain, flat_records[0]):
        assert "diagnostics" not in base and set(rec) - set(base) == {"diagnostics"}
        for key in base:
            if key == "features":
                assert set(base[key]) == set(rec[key])
                assert all(np.array_equal(np.asarray(base[key][k]), np.asarray(rec[key][k])) for k in base[key] if not isinstance(base[key][k], dict))
            else:
                assert base[key] == rec[key], key


def test_recommend_configure_verify_round_trip(golden, chain, flat_records):
    import mic_eq_mi
    from mic_eq_mi import mic_eq_core as core

    records = flat_records[0]
    eng = core.Engine(float(SS.FS), len(records))
    core.configure_auto_eq_chain(eng, float(SS.FS), S.LIMITER_BANDS, S.limiter_settings(2.0))
    core.configure_voice_chain(eng, records[0])  # every setter accepts its value: a refusal raises
    eng.close()
    second = np.ascontiguousarray(chain["speech"][:, ::-1])
    verdicts = mic_eq_mi.verify_voice_setup_batch(chain["noise"], chain["speech"], second, SS.FS, records, SS.CHAIN_ARGUMENTS[0]["target_preset"])
    want = golden["offline/roundtrip_decisions"].tolist()
    assert [v["decision"] for v in verdicts] == want and "accept" in want
