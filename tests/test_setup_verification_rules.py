"""The rules of the second-passage verification (svm_decide of csrc/af_setup_verification_math.h) on the hand-made cases of
tests/setup_verification_rules_stimulus.py, held to what the reference's own validate_voice_setup_verification answered on the same
numbers (tests/golden/setup_verification.npz, rules() of tools/gen_golden_setup_verification.py): each side of each threshold in
the ladder's order, two rungs tripped at once, absent keys and their defaults, the early exits.  No GPU.

Decisions, reasons, key sets, counts and flags are equal.  The numbers are the inputs passed through, or differences of two of
them taken in the reference's order: equal bits."""
import ctypes as C
import pathlib

import numpy as np
import pytest

import setup_verification_oracle as O
import setup_verification_rules_stimulus as RS

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "setup_verification.npz"


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_fixture_covers_the_cases_and_the_ladder(golden):
    assert golden["rules/names"].tolist() == [name for name, _, _ in RS.CASES]
    assert golden["rules/decisions"].tolist() == [expected for _, _, expected in RS.CASES]  # the ladder as written, and the reference
    assert set(golden["rules/decisions"].tolist()) == {"accept", "reduce", "rollback", "retry"}
    assert len(set(golden["rules/reasons"].tolist())) == 7
    assert {"rollback_beats_reduce", "retry_beats_rollback"} <= set(golden["rules/names"].tolist())


@pytest.mark.parametrize("index", range(len(RS.CASES)), ids=[name for name, _, _ in RS.CASES])
def test_rules_equal_the_references(golden, index):
    name, overrides, _ = RS.CASES[index]
    got = O.decide(RS.case(overrides))
    assert got["decision"] == str(golden["rules/decisions"][index])
    assert got["reasons"] == [str(golden["rules/reasons"][index])]
    assert sorted(got) == str(golden["rules/keys"][index]).split("|")
    if set(got) - RS.EARLY_KEYS - {"simulation_backend"}:
        assert [got[key] for key in RS.NUMBER_KEYS] == golden["rules/numbers"][index].tolist()
        assert [got["limiter_activity_events"], int(got["clipped"])] == golden["rules/flags"][index].tolist()
    else:
        assert np.all(np.isnan(golden["rules/numbers"][index]))


def test_the_library_runs_the_same_rules():
    """af_setup_verification_decide and af_setup_verification_reason_text are the header's functions behind argument checks."""
    from mic_eq_mi import _lib

    L = _lib.load()
    row, e, out = _lib.SetupVerificationRow(), _lib.SetupVerificationEvidence(), _lib.SetupVerificationResult()
    e.sample_rate, e.verification_samples, e.backend_is_rust = 48_000.0, 201_600, 1
    for k, level in enumerate((-60.0, -20.0, -21.0, -19.0, -58.5)):
        row.rms_db[k] = level
    row.spectral_target_error_before_db, row.spectral_target_error_after_db, row.shape_delta_db = 3.0, 2.5, 1.0
    assert L.af_setup_verification_decide(C.byref(row), C.byref(e), C.byref(out)) == 0
    assert (out.decision, out.reason, out.early_exit) == (2, 2, 0)  # every simulation key absent: 120 dB of reduction, rollback
    e.present = (1 << 13) - 1
    e.compressor_gain_reduction_p95_db, e.compressor_gain_reduction_db, e.output_true_peak_db = 3.0, 5.0, -1.75
    e.limiter_effective_ceiling_db, e.output_rms_db, e.input_rms_db = -1.5, -19.0, -21.0
    e.target_p95_reduction_db, e.peak_reduction_cap_db, e.deesser_max_reduction_db = 3.5, 8.0, 6.0
    assert L.af_setup_verification_decide(C.byref(row), C.byref(e), C.byref(out)) == 0
    assert (out.decision, out.reason, out.early_exit) == (0, 0, 0) and out.relative_noise_floor_change_db == -0.5
    e.verification_samples = 143_999
    assert L.af_setup_verification_decide(C.byref(row), C.byref(e), C.byref(out)) == 0
    assert (out.decision, out.reason, out.early_exit) == (3, 4, 1)
    for index, text in enumerate(O.lib().svr_reason_text(i) for i in range(7)):
        assert L.af_setup_verification_reason_text(index) == text and text
    assert L.af_setup_verification_reason_text(7) is None and L.af_setup_verification_reason_text(-1) is None
    bad = _lib.AF_ERR_INVALID_ARGUMENT
    assert L.af_setup_verification_decide(None, C.byref(e), C.byref(out)) == bad
    assert L.af_setup_verification_decide(C.byref(row), None, C.byref(out)) == bad
    assert L.af_setup_verification_decide(C.byref(row), C.byref(e), None) == bad
    e.sample_rate = 0.0
    assert L.af_setup_verification_decide(C.byref(row), C.byref(e), C.byref(out)) == bad


# ---- the offline validation and the confidences, voice_setup.py:1265-1364
OFFLINE_MEASURED = 0.0  # largest |restatement - reference| over the confidences: the same operations in the same order; 1e-12 + 4 x allowed
OFFLINE_NUMBERS = ("setup_confidence", "recommendation_uncertainty", "capture_confidence", "eq_confidence", "gate_confidence",
                   "deesser_confidence", "compressor_confidence")


def test_offline_validation_rules_equal_the_references(golden):
    """The reference's analyze_voice_setup on the six chain pairs, two argument sets, without EQ, with the caller's EQ
    (analysis_confidence on all, apply_recommended False / True / absent) and with a renderer that is not the native one: flags and
    reason lists equal, confidences within rounding.  The cases hold both offline_validation_passed values, weak captures (the 0.49
    cap) and the x0.90 of an advisory backend."""
    import setup_verification_stimulus as SV

    worst, seen = 0.0, set()
    for a in (0, 1):
        for mode in ("flat", "eq", "advisory"):
            inputs, validation = golden[f"offline/{a}/{mode}/inputs"], golden[f"offline/{a}/{mode}/validation"]
            for s in range(inputs.shape[0]):
                got = O.offline_validation(inputs[s], validation[s], SV.offline_eq(s) if mode == "eq" else None, mode != "advisory")
                flags = golden[f"offline/{a}/{mode}/flags"][s].tolist()
                assert [got["weak_capture"], got["apply_recommended"], got["offline_validation_passed"]] == flags, (a, mode, s)
                want = str(golden[f"offline/{a}/{mode}/reasons"][s]).split("|")
                own = int(inputs[s][11])  # the noise reference's own reasons lead the list
                assert got["reasons"] == [r for r in want[own:] if r], (a, mode, s, got["reasons"], want)
                numbers = dict(zip(OFFLINE_NUMBERS, golden[f"offline/{a}/{mode}/numbers"][s]))
                for key in OFFLINE_NUMBERS:
                    if key != "capture_confidence":
                        worst = max(worst, abs(got[key] - float(numbers[key])))
                seen.update({("passed", flags[2]), ("weak", flags[0]), ("apply", flags[1]), ("mode", mode)})
                if flags[0]:
                    assert got["setup_confidence"] <= 0.49
                if mode == "advisory":
                    assert "offline DSP validation is advisory without the Rust extension" in got["reasons"]
                if mode == "flat":
                    assert got["reasons"][-1] == "Auto-EQ abstained from this capture" and not got["apply_recommended"]
    print(f"largest |confidence - reference| = {worst:.3e}")
    assert {("passed", 0), ("passed", 1), ("weak", 0), ("weak", 1), ("apply", 0), ("apply", 1)} <= seen
    assert worst <= 1e-9 and worst <= 1e-12 + 4 * OFFLINE_MEASURED


def test_advisory_backend_scales_the_setup_confidence(golden):
    for s in range(6):
        i, v = golden["offline/0/flat/inputs"][s], golden["offline/0/flat/validation"][s]
        rust, advisory = O.offline_validation(i, v, None, True), O.offline_validation(i, v, None, False)
        if not rust["weak_capture"]:
            assert advisory["setup_confidence"] == rust["setup_confidence"] * 0.90
        assert advisory["offline_validation_passed"] == rust["offline_validation_passed"]
