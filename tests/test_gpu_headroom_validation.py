"""The EQ headroom validation (mic_eq_mi/headroom.py) on the GPU, on the ten captures of tests/headroom_stimulus.py.

Sweep route: the block rows of every (capture, scale) equal, bit for bit, those of a plain Engine that runs the FULL chain
(de-esser, EQ, compressor, limiter, true-peak limiter) on the capture with the scaled bands: the ROW_FIELDS of
tests/test_gpu_compressor_sweep.py.  Its dicts agree with the engine route's as that file holds the fold to
chain_diagnostics: equal, bit-equal, and within its DB_ALLOWED on its DB_KEYS (the fold is the same kernel).

apply_headroom_validation_batch against tests/golden/headroom_validation.npz (the reference's own apply_headroom_validation,
its renders answered by the CPU oracle): the selected scale, the flags, the status, the capped confidences and the scaled gains
are equal.  The numeric keys of ``before`` and ``after`` are the engine's against the oracle's: counts are equal, and the dB
values are within GOLDEN_ALLOWED_DB = four times the largest |GPU - golden| measured on the MI355X on this stimulus
(MEASURED_DB = 3.815e-6 dB below and DESIGN 4.22), which stays under the 1e-3 dB by which every decision of the stimulus clears its threshold
(tests/test_headroom_stimulus.py).  The test prints the largest difference per key before it asserts."""
import pathlib

import numpy as np
import pytest

import headroom_stimulus as HS
from test_gpu_compressor_sweep import BIT_EQUAL_KEYS, DB_ALLOWED, DB_KEYS, EQUAL_KEYS, ROW_FIELDS, same_bits

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "headroom_validation.npz"
SWEEPABLE = [c for c in range(HS.N_CAPTURES) if c != 7]  # capture 7 disables the compressor
COUNT_KEYS = ("true_peak_limited_events", "active_analysis_block_count", "processed_samples", "analysis_block_ms")
# the largest |GPU - golden| over the other numeric keys of before / after, measured on the MI355X on this stimulus
# (silence_level_delta_db: the difference of two levels, an ulp of each; input_rms_db and active_analysis_threshold_db 1.9e-6, the
# peak levels and headrooms 4.8e-7, every gain-reduction key 0)
MEASURED_DB = 3.815e-06
GOLDEN_ALLOWED_DB = 4 * MEASURED_DB
DECISION_MARGIN_DB = 1e-3


@pytest.fixture(scope="module")
def mi():
    import mic_eq_mi

    return mic_eq_mi


@pytest.fixture(scope="module")
def audio():
    return HS.captures()


@pytest.fixture(scope="module")
def swept(mi, audio):
    timing: dict = {}
    r = mi.simulate_candidate_chain_batch(audio[SWEEPABLE], HS.FS, [HS.eq_settings(c) for c in SWEEPABLE],
                                          [HS.chain_settings(c) for c in SWEEPABLE], HS.SCALES, route="sweep", return_rows=True, timing=timing)
    r["timing"] = timing
    return r


@pytest.mark.parametrize("position", range(len(SWEEPABLE)))
def test_sweep_rows_equal_a_plain_engine_run_of_the_full_chain(mi, audio, swept, position):
    from mic_eq_mi import headroom as H
    from mic_eq_mi import mic_eq_core as core

    capture = SWEEPABLE[position]
    flat = H._engine_settings(H._flatten_chain_settings(HS.chain_settings(capture)))
    bands = H._bands_from_settings(HS.eq_settings(capture))
    assert swept["rows"].shape == (21, len(SWEEPABLE), len(HS.SCALES))
    for k, scale in enumerate(HS.SCALES):
        engine = core.Engine(float(HS.FS), 1)
        try:
            core.configure_auto_eq_chain(engine, float(HS.FS), H._scaled_bands(bands, scale), flat)
            engine.process(audio[capture : capture + 1])
            want = engine.block_stats()[:, 0]
        finally:
            engine.close()
        for field in ROW_FIELDS:
            assert same_bits(swept["rows"][field][:, position, k], want[field]), (capture, scale, field)
    rows = swept["rows"][:, position]
    if capture == 4:
        assert rows["deesser_gain_reduction_db"].max() > 0.5
    if capture == 3:
        assert rows["limiter_peak_gain_reduction_db"].max() > 5.0 and rows["true_peak_limited_events"].sum() > 0
    assert set(swept["timing"]) == {"front_end_wall_ms", "lane_eq_kernel_ms", "sweep_kernel_ms", "fold_kernel_ms"}
    assert all(v > 0.0 for v in swept["timing"].values())


def test_sweep_dicts_agree_with_the_engine_route(mi, audio, swept):
    engine = mi.simulate_candidate_chain_batch(audio[SWEEPABLE], HS.FS, [HS.eq_settings(c) for c in SWEEPABLE],
                                               [HS.chain_settings(c) for c in SWEEPABLE], HS.SCALES, route="engine")
    worst, where = 0.0, None
    for position, capture in enumerate(SWEEPABLE):
        for k, scale in enumerate(HS.SCALES):
            got, want = swept["results"][position][k], engine[position][k]
            assert set(got) == set(want) and got["simulation_backend"] == "rust" and got["safety_authority"] == "authoritative"
            for key in EQUAL_KEYS:
                assert got[key] == want[key], (capture, scale, key)
            for key in BIT_EQUAL_KEYS:
                assert np.float32(got[key]).tobytes() == np.float32(want[key]).tobytes(), (capture, scale, key, got[key], want[key])
            for key in DB_KEYS:
                d = abs(got[key] - want[key])
                if d > worst:
                    worst, where = d, (capture, scale, key)
    print(f"largest |sweep - engine| over the dB and pumping fields: {worst:.3e} at {where} (allowed {DB_ALLOWED:.3e})")
    assert worst <= DB_ALLOWED
    assert swept["results"][SWEEPABLE.index(6)][0]["limiter_effective_ceiling_db"] == -3.0  # the second limiter group
    assert swept["results"][0][0]["limiter_effective_ceiling_db"] == -1.5


def test_validation_matches_the_references(mi, audio):
    from mic_eq_mi import headroom as H

    golden = np.load(GOLDEN)
    given = HS.all_eq_settings()
    results = mi.apply_headroom_validation_batch(audio, HS.FS, given, HS.all_chain_settings(), max_lane_eq_bytes=7 * 19_584 * 4 * 4)
    assert given == HS.all_eq_settings()  # the input is not edited
    numeric = golden["numeric_keys"].tolist()
    worst = {key: 0.0 for key in numeric}
    for c, r in enumerate(results):
        v = r["headroom_validation"]
        assert "|".join(sorted(r)) == golden["keys"][c], c
        assert v["gain_scale"] == golden["gain_scale"][c] and r["headroom_gain_scale"] == golden["headroom_gain_scale"][c], c
        assert v["status"] == golden["status"][c], c
        flags = [v["safe"], v["authoritative"], v["advisory"], v["meets_advisory_thresholds"], r["headroom_safe"], r["headroom_advisory"]]
        assert all(type(f) is bool for f in flags) and [int(f) for f in flags] == golden["flags"][c].tolist(), c
        assert r["band_gains"] == golden["band_gains"][c].tolist(), c
        for key, want in zip(("validation_gain_scale", "validation_confidence", "analysis_confidence"), golden["optional"][c]):
            assert (key not in r) if np.isnan(want) else (r[key] == want), (c, key)
        for key in set(given[c]) - {"band_gains", "validation_gain_scale", "validation_confidence", "analysis_confidence"}:
            assert r[key] == given[c][key], (c, key)
        for side in ("before", "after"):
            assert bool(v[side]["non_finite_output"]) == bool(golden["non_finite_output"][c, ("before", "after").index(side)])
            assert v[side]["simulation_backend"] == "rust" and H._is_headroom_safe(v["after"]) == v["meets_advisory_thresholds"]
            for k, key in enumerate(numeric):
                worst[key] = max(worst[key], abs(float(v[side][key]) - float(golden[side][c, k])))
    for key in numeric:
        print(f"largest |GPU - golden| {key}: {worst[key]:.3e}")
    largest = max(worst[key] for key in numeric if key not in COUNT_KEYS)
    print(f"largest over the dB keys: {largest:.3e} (allowed {GOLDEN_ALLOWED_DB:.3e}, decision margin {DECISION_MARGIN_DB:.0e})")
    assert all(worst[key] == 0.0 for key in COUNT_KEYS)
    assert GOLDEN_ALLOWED_DB < DECISION_MARGIN_DB
    assert largest <= GOLDEN_ALLOWED_DB


def test_reference_signatures_are_the_one_stream_calls(mi, audio):
    c = 1
    one = mi.apply_headroom_validation(audio[c], HS.FS, HS.eq_settings(c), HS.chain_settings(c))
    batch = mi.apply_headroom_validation_batch(audio[c : c + 1], HS.FS, HS.eq_settings(c), HS.chain_settings(c))[0]
    sim = mi.simulate_candidate_chain(audio[c], HS.FS, HS.eq_settings(c), HS.chain_settings(c))

    def timeless(d):
        return {k: (timeless(v) if isinstance(v, dict) else v) for k, v in d.items() if k != "candidate_runtime_ms"}

    assert timeless(one) == timeless(batch) and timeless(sim) == timeless(one["headroom_validation"]["before"])
    assert one["headroom_validation"]["gain_scale"] == 0.85


def test_recommendation_validates_the_callers_eq_and_feeds_it_onward(mi):
    import speech_features_stimulus as SS
    from test_gpu_compressor_search import same

    c = SS.chain_batch()
    pair = slice(0, 2)
    arguments = dict(vad_probabilities=c["vad"][pair], noise_vad_probabilities=c["noise_vad"][pair], offline_validation=True)
    eq = {"band_freqs": list(HS.FREQS), "band_gains": [9.0] * 10, "band_qs": [1.0] * 10, "analysis_confidence": 0.9}
    noise, speech = c["noise"][pair], c["speech"][pair]
    plain = mi.recommend_voice_chain_batch(noise, speech, SS.FS, eq_settings=eq, **arguments)
    off = mi.recommend_voice_chain_batch(noise, speech, SS.FS, eq_settings=eq, validate_eq_headroom=False, **arguments)
    got = mi.recommend_voice_chain_batch(noise, speech, SS.FS, eq_settings=eq, validate_eq_headroom=True, **arguments)
    validated = mi.apply_headroom_validation_batch(speech, SS.FS, eq)
    onward = mi.recommend_voice_chain_batch(noise, speech, SS.FS, eq_settings=validated, **arguments)

    def timeless(d):
        if isinstance(d, dict):
            return {k: timeless(v) for k, v in d.items() if k != "candidate_runtime_ms"}
        return [timeless(v) for v in d] if isinstance(d, list) else d

    assert any(v["headroom_gain_scale"] < 1.0 for v in validated), [v["headroom_gain_scale"] for v in validated]
    for a, b, g, v, o in zip(plain, off, got, validated, onward):
        assert same(timeless(a), timeless(b)) and "eq" not in a          # without the keyword the return is today's
        assert set(g) == set(a) | {"eq"}                                 # only `eq` is added ...
        assert same(timeless(g["eq"]), timeless(v)) and g["eq"]["band_gains"] == (np.asarray([9.0] * 10) * v["headroom_gain_scale"]).tolist()
        assert same(timeless({k: x for k, x in g.items() if k != "eq"}), timeless(o))  # ... and the scaled gains go onward
        if v["headroom_gain_scale"] < 1.0:
            assert not same(timeless(g["diagnostics"]["offline_validation"]), timeless(a["diagnostics"]["offline_validation"]))
    with pytest.raises(ValueError, match="needs eq_settings"):
        mi.recommend_voice_chain_batch(noise, speech, SS.FS, validate_eq_headroom=True)
