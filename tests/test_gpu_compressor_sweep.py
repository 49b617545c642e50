"""The compressor candidate sweep (csrc/af_compressor_search.hip) on the GPU: 3 captures x (50 + 16) candidates, 48 333
samples each (tests/compressor_sweep_stimulus.py: side chain on and off, adaptive release on and off, a manual makeup gain,
a de-esser on one capture, 198 lanes = three waves and six lanes).

Rows: every lane's block rows, and its output audio, equal bit for bit those of a plain Engine that runs the FULL chain
(de-esser, EQ, compressor, limiter, true-peak limiter) on the lane's capture with the lane's candidate as its preset; a lane's
rows do not depend on the lanes around it (the batch reversed, and in two halves).

Fold: against mic_eq_core.chain_diagnostics on the same rows.  Counts, masks and non_finite_output are equal.  What is a
maximum or a selected element of the rows (and the f32 lerp between two selected elements) is equal bit for bit.  What goes
through f32 log10 or sqrt (the dB values, headrooms, level medians and the pumping score: the device's log10f / sqrtf against
numpy's) is within DB_ALLOWED = four times the largest difference measured on the MI355X; the test prints what
it measures before it asserts."""
import numpy as np
import pytest

import compressor_sweep_stimulus as CS

pytestmark = pytest.mark.gpu

ROW_FIELDS = ("input_sample_peak", "output_sample_peak", "true_peak_limiter_input_peak", "output_true_peak",
              "limiter_peak_gain_reduction_db", "true_peak_limiter_gain_reduction_db", "compressor_gain_reduction_db",
              "deesser_gain_reduction_db", "input_square_sum", "output_square_sum", "true_peak_limited_events", "non_finite_output",
              "compressor_makeup_gain_db")
EQUAL_KEYS = ("true_peak_limited_events", "non_finite_output", "active_analysis_block_count", "processed_samples", "analysis_block_ms",
              "limiter_effective_ceiling_db")
BIT_EQUAL_KEYS = ("limiter_gain_reduction_db", "true_peak_limiter_gain_reduction_db", "compressor_gain_reduction_db",
                  "deesser_gain_reduction_db", "compressor_gain_reduction_median_db", "compressor_gain_reduction_p95_db",
                  "compressor_gain_reduction_active_ratio", "silence_output_gain_db", "deesser_gain_reduction_median_db",
                  "deesser_gain_reduction_p95_db")
DB_KEYS = ("input_sample_peak_db", "input_rms_db", "output_sample_peak_db", "pre_limiter_true_peak_db", "output_true_peak_db",
           "output_rms_db", "sample_headroom_db", "pre_limiter_true_peak_headroom_db", "true_peak_headroom_db", "active_output_gain_db",
           "silence_level_delta_db", "compressor_pumping_score_db", "active_analysis_threshold_db")
# 4 x 7.629e-06 dB, the largest |device - numpy| over DB_KEYS measured on the MI355X on this stimulus (lane 2,
# silence_level_delta_db: the difference of two levels near -60 dB, two ulp of them; the device rounds an f64 log10 once,
# numpy's f32 log10 is a few ulp off that)
DB_ALLOWED = 4 * 7.629e-06


class Sweep:
    def __init__(self):
        from mic_eq_mi import compressor_search as cs

        self.cs = cs
        self.audio = CS.captures()
        self.settings = [CS.chain_settings(c) for c in range(len(CS.LEVELS))]
        self.lanes = CS.lanes()
        self.comp_in, self.input_rows = cs.compressor_input_batch(self.audio, CS.FS, CS.BANDS, self.settings)
        self.bases = [(st["compressor_makeup_gain_db"], st.get("compressor_base_release_ms", 50.0), st["compressor_adaptive_release"],
                       st["compressor_sidechain_highpass_enabled"]) for st in self.settings]
        self.search = cs.CompressorSearch(CS.FS)
        self.search.load(self.comp_in, self.input_rows)
        self.records = self.search.sweep(self.lanes, self.bases, keep_audio=True)
        self.rows = self.search.rows()
        self.out = self.search.audio()
        self.masks = self.search.masks()

    def run(self, lanes):
        records = self.search.sweep(lanes, self.bases)
        return records, self.search.rows()


@pytest.fixture(scope="module")
def sweep():
    s = Sweep()
    yield s
    s.search.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("capture", range(len(CS.LEVELS)))
def test_rows_and_audio_equal_a_plain_engine_run_of_the_full_chain(sweep, capture):
    from mic_eq_mi import mic_eq_core as core

    assert sweep.rows.shape == (-(-CS.N // 960), len(sweep.lanes)) and len(sweep.lanes) % 64 != 0
    checked = 0
    for lane, (c, *candidate) in enumerate(sweep.lanes):
        if c != capture:
            continue
        engine = core.Engine(float(CS.FS), 1)
        try:
            core.configure_auto_eq_chain(engine, float(CS.FS), CS.BANDS, CS.chain_settings(capture, candidate))
            want_audio = engine.process(sweep.audio[capture : capture + 1])
            want = engine.block_stats()[:, 0]
        finally:
            engine.close()
        for field in ROW_FIELDS:
            assert same_bits(sweep.rows[field][:, lane], want[field]), (lane, candidate, field)
        assert same_bits(sweep.out[lane], want_audio[0]), (lane, candidate)
        checked += 1
    assert checked == CS.PHASE_1 + CS.PHASE_2
    rows = sweep.rows[:, [lane for lane, l in enumerate(sweep.lanes) if l[0] == capture]]
    assert rows["compressor_gain_reduction_db"].max() > 3.0  # the compressor works ...
    if capture == 2:
        assert rows["limiter_peak_gain_reduction_db"].max() > 0.5 and rows["true_peak_limited_events"].sum() > 0  # ... and the limiters
    if capture == 1:
        assert rows["deesser_gain_reduction_db"].max() > 0.0 and rows["compressor_makeup_gain_db"].max() == np.float32(2.5)


def test_a_lanes_rows_do_not_depend_on_its_neighbours(sweep):
    n = len(sweep.lanes)
    records, rows = sweep.run(sweep.lanes[::-1])
    assert same_bits(rows[:, ::-1], sweep.rows) and same_bits(records[::-1], sweep.records)
    half = n // 2 + 7
    for lo, hi in ((0, half), (half, n)):
        records, rows = sweep.run(sweep.lanes[lo:hi])
        assert same_bits(rows, sweep.rows[:, lo:hi]) and same_bits(records, sweep.records[lo:hi])
    records, rows = sweep.run(sweep.lanes)  # a reused handle, and the full batch after smaller ones
    assert same_bits(rows, sweep.rows) and same_bits(records, sweep.records)


def test_fold_against_chain_diagnostics(sweep):
    from mic_eq_mi import mic_eq_core as core

    lengths = core._block_lengths(CS.N, 960)
    worst, where, worst_rms = 0.0, None, 0.0
    for capture in range(len(CS.LEVELS)):  # the host's masks against numpy's on the same rows
        rows = sweep.input_rows[:, capture]
        in_db = core._linear_to_db(np.sqrt(rows["input_square_sum"] / lengths.astype(np.float64)).astype(np.float32))
        threshold = max(max(core._percentile(in_db, 0.20) + np.float32(6.0), core._percentile(in_db, 0.90) - np.float32(24.0)), np.float32(-60.0))
        assert np.array_equal(sweep.masks["active"][capture], in_db >= threshold), capture
        assert np.array_equal(sweep.masks["audible"][capture], in_db > np.float32(-100.0)), capture
        active = np.count_nonzero(sweep.masks["active"][capture])
        assert (active < 3) if capture == 0 else (3 <= active < in_db.size), (capture, active)  # both paths of python_api.rs:618-625
        assert sweep.masks["audible"][capture].all() == (capture != 2)
    for lane, (capture, *candidate) in enumerate(sweep.lanes):
        want = core.chain_diagnostics(sweep.rows[:, lane], lengths, -1.5)
        got = sweep.cs.simulation_dict(sweep.records[lane])
        assert set(got) == set(want)
        record = sweep.records[lane]
        for key in EQUAL_KEYS:
            assert got[key] == want[key], (lane, key)
        for key in BIT_EQUAL_KEYS:
            assert np.float32(got[key]).tobytes() == np.float32(want[key]).tobytes(), (lane, key, got[key], want[key])
        for key, field in (("output_sample_peak", "output_sample_peak"), ("pre_limiter_true_peak", "true_peak_limiter_input_peak"),
                           ("output_true_peak", "output_true_peak")):
            assert record[key].tobytes() == np.float32(sweep.rows[field][:, lane].max()).tobytes(), (lane, key)
        total = 0.0
        for value in sweep.rows["output_square_sum"][:, lane]:
            total += float(value)
        worst_rms = max(worst_rms, abs(float(record["output_rms"]) - float(np.float32(np.sqrt(total / CS.N)))))
        for key in DB_KEYS:
            d = abs(got[key] - want[key])
            if d > worst:
                worst, where = d, (lane, key)
    print(f"largest |device - numpy| over the dB and pumping fields: {worst:.3e} at {where} (allowed {DB_ALLOWED:.3e}); output_rms: {worst_rms:.3e}")
    assert worst <= DB_ALLOWED and worst_rms == 0.0


def test_operator_returns_one_dict_per_candidate(sweep):
    import mic_eq_mi

    lanes = sweep.lanes[:5] + sweep.lanes[-5:]
    r = mic_eq_mi.simulate_compressor_candidates_batch(sweep.audio, CS.FS, CS.BANDS, sweep.settings, lanes, return_rows=True)
    index = list(range(5)) + list(range(len(sweep.lanes) - 5, len(sweep.lanes)))
    assert same_bits(r["rows"], sweep.rows[:, index]) and same_bits(r["records"], sweep.records[index])
    assert len(r["results"]) == 10 and r["results"][0]["processed_samples"] == CS.N and "candidate_runtime_ms" in r["results"][0]
    settings = [dict(st) for st in sweep.settings]
    settings[1]["compressor_auto_makeup_enabled"] = True
    with pytest.raises(NotImplementedError, match="auto-makeup"):
        mic_eq_mi.simulate_compressor_candidates_batch(sweep.audio, CS.FS, CS.BANDS, settings, lanes)
    with pytest.raises(ValueError, match="names capture"):
        sweep.search.sweep([(3, -20.0, 4.0, 5.0, 100.0)], sweep.bases)
