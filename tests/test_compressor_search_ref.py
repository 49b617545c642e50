"""The compressor calibration search of csrc/af_compressor_search_math.h (the header the library's host half runs) on the CPU,
against what the reference's own _calibrate_compressor_threshold did on the same captures (tests/golden/compressor_search.npz,
written by tools/gen_golden_compressor_search.py with the CPU oracle answering the reference's simulations).

tests/ref/compressor_search_ref.c puts the header behind a C interface.  Every simulation is the CPU oracle's BLOCK PROCESSOR run
block by block (tests/chain_oracle.py), its per-block rows folded by the header's csm_fold -- the arithmetic cs_fold_kernel
does on the device -- and the search runs on those results.  The candidate sequence, the winner and the flags must be equal.
The fold differs from the oracle's own (which the fixture holds) in its f32 log10 alone: the header rounds an f64 log10 once,
the oracle calls the host's log10f, one ulp apart for a few arguments in a hundred.  The restatement alone shows the largest
differences MEASURED_SCORE (objectives, relative) and MEASURED_NUMBER (numeric diagnostics, dB) against the fixture, printed
below before they are asserted; the tests allow four times those.

Also here: the per-capture masks of the same header against numpy's, and its round(x, 6)."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import compressor_search_oracle as CO
import compressor_search_stimulus as CS
import compressor_sweep_stimulus as SW

# largest |restatement - reference| measured here over the finite objectives of every evaluated candidate of the fixture
# (relative to the objective) and over the winners' numeric diagnostics (dB; one ulp of a level between 16 and 32 dB)
MEASURED_SCORE = 3.636e-09
MEASURED_NUMBER = 4.768e-07
SCORE_ALLOWED = 4 * MEASURED_SCORE
NUMBER_ALLOWED = 4 * MEASURED_NUMBER


def flat_settings(deesser: dict, compressor: dict, values) -> dict:
    """The settings dict the reference's search hands the chain for one candidate (voice_setup.py:798-816 through
    auto_eq_parts/headroom.py:42-84): auto-makeup off (and then makeup 0), the search's fixed limiter."""
    auto = bool(compressor.get("auto_makeup_enabled", False))
    d = {f"deesser_{k}": v for k, v in deesser.items()}
    d.update({"compressor_enabled": True, "compressor_threshold_db": float(values[0]), "compressor_ratio": float(values[1]),
              "compressor_attack_ms": float(values[2]), "compressor_release_ms": float(values[3]),
              "compressor_makeup_gain_db": 0.0 if auto else float(compressor.get("makeup_gain_db", 0.0)),
              "compressor_adaptive_release": bool(compressor.get("adaptive_release", False)),
              "compressor_base_release_ms": float(compressor.get("base_release_ms", 50.0)), "compressor_auto_makeup_enabled": False,
              "compressor_target_lufs": float(compressor.get("target_lufs", -18.0)),
              "compressor_sidechain_highpass_enabled": bool(compressor.get("sidechain_highpass_enabled", True)),
              "limiter_enabled": True, "limiter_ceiling_db": -1.5, "limiter_release_ms": 80.0, "limiter_careful_output_enabled": True})
    return d


@pytest.fixture(scope="module")
def searches(oracle):
    audio = CS.captures()
    bands = list(zip(CS.EQ_SETTINGS["band_freqs"], CS.EQ_SETTINGS["band_gains"], CS.EQ_SETTINGS["band_qs"]))
    out = []
    with ThreadPoolExecutor(8) as pool:  # (the oracle runs outside the interpreter lock)
        for c, (name, level, deesser, compressor, targets) in enumerate(CS.CASES):
            def simulate(values, c=c, deesser=deesser, compressor=compressor):
                return list(pool.map(lambda v: CO.fold(CO.oracle_rows(audio[c], float(CS.FS), bands, flat_settings(deesser, compressor, v))),
                                     values))
            out.append(CO.run_search(compressor, targets, simulate))
    return out


def test_candidate_sequence_winner_and_flags_equal_the_references(searches):
    import hashlib

    fx = CS.fixture()
    assert str(fx["audio_sha256"]) == hashlib.sha256(CS.captures().astype("<f4").tobytes()).hexdigest()
    assert {"expanded_local_step", "expanded_halton", "threshold_only_kept", "no_feasible", "grid_point_duplicate"} <= set(fx["classes"].tolist())
    worst, worst_number = 0.0, 0.0
    for c, (name, *_rest) in enumerate(CS.CASES):
        got, compressor, targets = searches[c], CS.CASES[c][3], CS.CASES[c][4]
        want_values, want_scores = fx[f"{c}/evaluated"], fx[f"{c}/scores"]
        feasible, expanded_selected, peak_cap_passed, iterations, candidate_count = (int(v) for v in fx[f"{c}/flags"])
        assert np.array_equal(got["evaluated"], want_values), name
        assert np.array_equal(np.isfinite(got["scores"]), np.isfinite(want_scores)), name
        finite = np.isfinite(want_scores)
        if finite.any():
            worst = max(worst, float(np.max(np.abs(got["scores"][finite] - want_scores[finite]) / np.abs(want_scores[finite]))))
        assert got["feasible"] == bool(feasible) and got["winner"] == int(fx[f"{c}/winner"]), name
        assert len(got["evaluated"]) + (1 if feasible else 0) == iterations, name
        numbers = dict(zip(CS.DIAGNOSTIC_NUMBERS, fx[f"{c}/numbers"]))
        if not feasible:
            assert name == "no_feasible" and len(got["evaluated"]) == 50
            continue
        assert got["expanded_selected"] == bool(expanded_selected) and candidate_count == iterations, name
        winner = got["simulations"][got["winner"]]
        assert (winner["compressor_gain_reduction_db"] <= targets[2] + 1.0e-6) == bool(peak_cap_passed)
        assert np.array_equal(got["evaluated"][got["winner"]], fx[f"{c}/calibrated"]), name
        mine = {"measured_median_gain_reduction_db": winner["compressor_gain_reduction_median_db"],
                "measured_p95_gain_reduction_db": winner["compressor_gain_reduction_p95_db"],
                "measured_peak_gain_reduction_db": winner["compressor_gain_reduction_db"],
                "active_reduction_ratio": winner["compressor_gain_reduction_active_ratio"],
                "active_output_gain_db": winner["active_output_gain_db"], "silence_output_gain_db": winner["silence_output_gain_db"],
                "compressor_pumping_score_db": winner["compressor_pumping_score_db"], "output_true_peak_db": winner["output_true_peak_db"],
                "pre_limiter_true_peak_headroom_db": winner["pre_limiter_true_peak_headroom_db"]}
        for key, value in mine.items():
            worst_number = max(worst_number, abs(value - numbers[key]))
        for key, value in (("total_objective", got["scores"][got["winner"]]), ("incumbent_objective", got["incumbent_objective"]),
                           ("threshold_only_objective", got["threshold_only_objective"]),
                           ("expanded_candidate_objective", got["scores"][got["expanded"]])):
            if value != numbers[key]:
                worst = max(worst, abs(value - numbers[key]) / abs(numbers[key]))
    print(f"largest |restatement - reference|: objectives {worst:.3e} relative (allowed {SCORE_ALLOWED:.3e}), "
          f"numeric diagnostics {worst_number:.3e} dB (allowed {NUMBER_ALLOWED:.3e})")
    assert worst <= SCORE_ALLOWED and worst_number <= NUMBER_ALLOWED
    names = dict(zip(CS.NAMES, searches))
    assert names["local_step"]["winner"] >= 50 and names["local_step"]["expanded_selected"]
    assert 34 <= names["halton"]["winner"] < 50 and names["halton"]["expanded_selected"]  # a Halton point over its own +- steps
    kept = names["threshold_only"]
    assert not kept["expanded_selected"] and kept["scores"][kept["expanded"]] < kept["scores"][kept["winner"]]
    assert len(names["grid_point"]["evaluated"]) == 65 and len(names["local_step"]["evaluated"]) == 66


def test_fold_of_oracle_rows_against_the_oracles_own_fold(oracle):
    """csm_fold on the block processor's rows against simulate_auto_eq_chain's dict for every capture's incumbent: counts and
    what takes no logarithm equal, the dB values within two ulp of the levels they are differences of (below 128 dB)."""
    audio = CS.captures()
    bands = list(zip(CS.EQ_SETTINGS["band_freqs"], CS.EQ_SETTINGS["band_gains"], CS.EQ_SETTINGS["band_qs"]))
    exact = ("limiter_effective_ceiling_db", "limiter_gain_reduction_db", "true_peak_limiter_gain_reduction_db", "compressor_gain_reduction_db",
             "deesser_gain_reduction_db", "compressor_gain_reduction_median_db", "compressor_gain_reduction_p95_db",
             "compressor_gain_reduction_active_ratio", "silence_output_gain_db", "deesser_gain_reduction_median_db",
             "deesser_gain_reduction_p95_db", "true_peak_limited_events", "non_finite_output", "active_analysis_block_count",
             "processed_samples")
    for c, (name, level, deesser, compressor, targets) in enumerate(CS.CASES):
        settings = flat_settings(deesser, compressor, [compressor[k] for k in CS.CONTROLS])
        want = oracle.simulate_auto_eq_chain(audio[c], float(CS.FS), bands, settings)
        got = CO.fold(CO.oracle_rows(audio[c], float(CS.FS), bands, settings))
        for key, value in got.items():
            if key in exact:
                assert value == want[key], (name, key, value, want[key])
            else:
                assert abs(value - want[key]) <= 2 * float(np.spacing(np.float32(127.0))), (name, key, value, want[key])


def test_capture_masks_equal_numpys():
    from mic_eq_mi import mic_eq_core as core

    lengths = core._block_lengths(SW.N, 960)
    for x in SW.captures():
        sq = np.array([np.sum(x[i * 960 : (i + 1) * 960].astype(np.float64) ** 2) for i in range(lengths.size)])
        got = CO.capture_masks(sq, SW.N, 960)
        in_db = core._linear_to_db(np.sqrt(sq / lengths.astype(np.float64)).astype(np.float32))
        threshold = max(max(core._percentile(in_db, 0.20) + np.float32(6.0), core._percentile(in_db, 0.90) - np.float32(24.0)), np.float32(-60.0))
        # two f32 log10 implementations an ulp apart, times 20 and rounded again: two ulp of the level
        assert np.all(np.abs(got["in_db"] - in_db) <= 2 * np.spacing(np.abs(in_db)))
        mine = max(max(core._percentile(got["in_db"], 0.20) + np.float32(6.0), core._percentile(got["in_db"], 0.90) - np.float32(24.0)), np.float32(-60.0))
        assert got["active_threshold_db"] == mine  # the percentile rule itself, on the same levels: equal bits
        assert np.array_equal(got["active"], in_db >= threshold) and np.array_equal(got["audible"], in_db > np.float32(-100.0))
        assert got["active_count"] == np.count_nonzero(got["active"])


def test_round6_is_pythons_round():
    rng = np.random.default_rng(11)
    values = np.concatenate([rng.uniform(-60.0, 400.0, 2000), -55.0 + 1.53125 * np.arange(33), [2.0000005, 1.0000015, -24.3750005, 0.1234565]])
    for v in values:
        assert CO.lib().csr_round6(float(v)) == round(float(v), 6), v
