"""The compressor calibration search on the GPU (af_compressor_search_run behind calibrate_compressor_batch) on the captures of
tests/compressor_search_stimulus.py, against what the reference's _calibrate_compressor_threshold did on them with the CPU
oracle answering its simulations (tests/golden/compressor_search.npz).

The candidate sequence, the winner, expanded_search_selected, peak_cap_passed and iterations are equal.  The numeric
diagnostics are within what tests/test_compressor_search_ref.py allows the header's fold and search on the oracle's rows (four
times what it measured: NUMBER_ALLOWED in dB, SCORE_ALLOWED relative for the objectives) plus what tests/test_gpu_parity.py allows
the gain-reduction traces of the GPU chain against the oracle (1e-6 dB).
The test prints its largest difference before it asserts.  Every winner's verification run equals its first evaluation byte
for byte; a reused handle, and a smaller batch after a larger one, give equal bytes; the capture without a feasible candidate
keeps its settings.

Then the top level: recommend_voice_chain_batch(calibrate_compressor=True) on two of the chain pairs of the speech-feature
stimulus returns the calibrated compressor, configure_voice_chain takes it and audio comes back finite; with the default
arguments the return is what it was."""
import ctypes as C

import numpy as np
import pytest

import compressor_search_stimulus as CS
from test_compressor_search_ref import NUMBER_ALLOWED, SCORE_ALLOWED

pytestmark = pytest.mark.gpu

PARITY = 1e-6  # dB (and objective units: no objective term is steeper than 1.5 per dB)


@pytest.fixture(scope="module")
def calibration():
    import mic_eq_mi

    return mic_eq_mi.calibrate_compressor_batch(CS.captures(), CS.FS, return_search=True, **CS.arguments())


def test_search_equals_the_references(calibration):
    fx = CS.fixture()
    worst, where = 0.0, None
    for c, (name, level, deesser, compressor, targets) in enumerate(CS.CASES):
        calibrated, diagnostics, search = calibration[c]
        feasible, expanded_selected, peak_cap_passed, iterations, candidate_count = (int(v) for v in fx[f"{c}/flags"])
        assert set(diagnostics) == set(fx[f"{c}/keys"].tolist()), name
        assert np.array_equal(search["evaluated"], fx[f"{c}/evaluated"]), name
        assert np.array_equal(np.isfinite(search["scores"]), np.isfinite(fx[f"{c}/scores"])), name
        assert search["winner"] == int(fx[f"{c}/winner"]) and diagnostics["iterations"] == iterations, name
        assert (diagnostics["backend"] == "rust") == bool(feasible), name
        if not feasible:
            assert calibrated == compressor and diagnostics["iterations"] == 50 and name == "no_feasible"
            continue
        assert search["verification_equals_evaluation"], name
        assert diagnostics["expanded_search_selected"] == bool(expanded_selected) and diagnostics["peak_cap_passed"] == bool(peak_cap_passed)
        assert diagnostics["candidate_count"] == candidate_count
        assert [calibrated[k] for k in CS.CONTROLS] == fx[f"{c}/calibrated"].tolist(), name
        assert {k: v for k, v in calibrated.items() if k not in CS.CONTROLS} == {k: v for k, v in compressor.items() if k not in CS.CONTROLS}
        finite = np.isfinite(fx[f"{c}/scores"])
        want_scores = fx[f"{c}/scores"][finite]
        d = float(np.max(np.abs(search["scores"][finite] - want_scores) / (PARITY + SCORE_ALLOWED * np.abs(want_scores))))
        if d > worst:
            worst, where = d, (name, "scores")
        for key, want in zip(CS.DIAGNOSTIC_NUMBERS, fx[f"{c}/numbers"]):
            objective = key.endswith("_objective")
            allowed = PARITY + (SCORE_ALLOWED * abs(want) if objective else NUMBER_ALLOWED)
            d = 0.0 if diagnostics[key] == want else abs(diagnostics[key] - want) / allowed
            if d > worst:
                worst, where = d, (name, key)
    print(f"largest |GPU - reference| over objectives and numeric diagnostics, as a fraction of what is allowed: {worst:.3f} at {where} "
          f"(allowed: {PARITY:.1e} + {NUMBER_ALLOWED:.3e} dB, objectives {PARITY:.1e} + {SCORE_ALLOWED:.3e} relative)")
    assert worst <= 1.0


def test_a_reused_handle_and_a_smaller_batch_give_equal_bytes():
    from mic_eq_mi import compressor_search as cs

    arguments = CS.arguments()
    audio = CS.captures()
    bands = [cs._bands_from_settings(CS.EQ_SETTINGS)] * len(CS.CASES)
    front = [{f"deesser_{k}": v for k, v in d.items()} for d in arguments["deesser_settings"]]
    comp_in, rows = cs.compressor_input_batch(audio, float(CS.FS), bands, front)
    settings = [cs._search_settings(c, p95, median, cap) for c, p95, median, cap in
                zip(arguments["compressor_settings"], arguments["target_p95_db"], arguments["target_median_db"], arguments["peak_cap_db"])]
    as_bytes = lambda results: [C.string_at(C.addressof(r), C.sizeof(r)) for r in results]  # noqa: E731
    search = cs.CompressorSearch(CS.FS)
    try:
        search.load(comp_in, rows)
        first = as_bytes(search.run(settings))
        assert as_bytes(search.run(settings)) == first
        # the verification, independently of the library's own flag: every winner swept alone equals its record in a sweep of
        # all the capture's evaluated candidates, byte for byte
        results = search.run(settings)
        bases = [(0.0 if st["auto_makeup_enabled"] else st["makeup_gain_db"], st["base_release_ms"], st["adaptive_release"],
                  st["sidechain_highpass_enabled"]) for st in settings]
        for c, r in enumerate(results):
            if r.winner < 0:
                continue
            lanes = [(c, *r.evaluated[i]) for i in range(r.evaluated_count)]
            together = search.sweep(lanes, bases)
            alone = search.sweep([lanes[r.winner]], bases)
            assert alone[0].tobytes() == together[r.winner].tobytes(), c
            assert float(alone[0]["compressor_gain_reduction_p95_db"]) == r.measured_p95_gain_reduction_db
        subset = [5, 0, 3]
        search.load(comp_in[subset], rows[:, subset])
        assert as_bytes(search.run([settings[i] for i in subset])) == [first[i] for i in subset]
    finally:
        search.close()


def same(a, b) -> bool:
    """Equality of the nested dicts a recommendation is made of (their leaves may be arrays)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
    return a == b or (isinstance(a, float) and isinstance(b, float) and a != a and b != b)


def test_top_level_returns_the_calibrated_compressor_and_an_engine_takes_it():
    import mic_eq_mi
    import signals as S
    import speech_features_stimulus as SS
    from mic_eq_mi import mic_eq_core as core

    c = SS.chain_batch()
    pair = slice(0, 2)
    arguments = dict(vad_probabilities=c["vad"][pair], noise_vad_probabilities=c["noise_vad"][pair])
    plain = mic_eq_mi.recommend_voice_chain_batch(c["noise"][pair], c["speech"][pair], SS.FS, **arguments)
    off = mic_eq_mi.recommend_voice_chain_batch(c["noise"][pair], c["speech"][pair], SS.FS, calibrate_compressor=False, **arguments)
    got = mic_eq_mi.recommend_voice_chain_batch(c["noise"][pair], c["speech"][pair], SS.FS, calibrate_compressor=True,
                                                eq_settings=CS.EQ_SETTINGS, **arguments)
    without_eq = mic_eq_mi.recommend_voice_chain_batch(c["noise"][pair], c["speech"][pair], SS.FS, calibrate_compressor=True, **arguments)
    for a, b, g, w in zip(plain, off, got, without_eq):
        assert same(a, b) and "compressor_calibration" not in a  # the default return is what it was, key for key
        assert set(g) == set(a) | {"compressor_calibration"}
        assert same({k: v for k, v in g.items() if k not in ("compressor", "compressor_calibration")}, {k: v for k, v in a.items() if k != "compressor"})
        assert w["compressor"] == a["compressor"] and w["compressor_calibration"]["backend"] == "unavailable"
        calibration = g["compressor_calibration"]
        assert calibration["backend"] == "rust" and 51 <= calibration["iterations"] <= 68
        assert set(g["compressor"]) == set(a["compressor"])
        assert [g["compressor"][k] for k in CS.CONTROLS] == [calibration[k] for k in CS.CONTROLS]
        assert -55.0 <= g["compressor"]["threshold_db"] <= -6.0 and calibration["total_objective"] <= calibration["incumbent_objective"]
        engine = core.Engine(float(SS.FS), 2)
        try:
            core.configure_auto_eq_chain(engine, float(SS.FS), S.LIMITER_BANDS, S.limiter_settings(2.0))
            engine.set_prefilter_enabled(1, 1)
            core.configure_voice_chain(engine, g)
            out = engine.process(c["speech"][pair, 40_000:64_000])
        finally:
            engine.close()
        assert out.shape == (2, 24_000) and np.all(np.isfinite(out))
