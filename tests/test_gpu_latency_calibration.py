"""The latency calibration (mic_eq_mi/latency_calibration.py) on the GPU against tests/golden/latency_calibration.npz, the
reference's own analyze_latency on the recordings of tests/latency_stimulus.py.

success, message, peak_sample_offset, repetition_count, route_kind and compensation_basis are equal.  The float fields are
within 4 x the largest |GPU - golden| measured on the MI355X on this stimulus, per field: the MEASURED constants below and
DESIGN 4.23.  They stay orders of magnitude under the 1e-4 relative by which every decision of the stimulus clears its threshold
(tests/test_latency_stimulus.py).  The test prints the largest difference per field before it asserts.

The batch of 70 equals the same recordings run one at a time, bit for bit, and analyze_device equals analyze, bit for bit."""
import dataclasses

import numpy as np
import pytest

import latency_oracle as LO
import latency_stimulus as LS

pytestmark = pytest.mark.gpu

# the largest |GPU - golden| per field over the cases and the batch of 70, measured on the MI355X on this stimulus; the fields
# that measured 0 are medians of integer lags plus a clipped -+0.5 (every used burst's parabola saturates), exact in any arithmetic
MEASURED = {
    "measured_round_trip_ms": 0.0,
    "sub_sample_offset": 0.0,
    "confidence": 1.555e-15,  # the cases alone 2.2e-16
    "agreement_ms": 0.0,
    "ambiguity_score": 2.110e-15,  # the cases alone 1.0e-15
    "route_latency_ms": 0.0,
    "applied_compensation_ms": 0.0,
}
DECISION_MARGIN = 1e-4


def allowed(field):
    return 4.0 * MEASURED[field]


@pytest.fixture(scope="module")
def mi():
    import mic_eq_mi

    return mic_eq_mi


@pytest.fixture(scope="module")
def golden():
    return np.load(LS.GOLDEN)


@pytest.fixture(scope="module")
def batch(mi):
    recorded, lengths, akw = LS.batch()
    lc = mi.LatencyCalibration(48_000, LS.probe(), LS.BATCH, LS.LONG)
    results = lc.analyze(recorded, lengths, **akw)
    ms = lc.last_kernel_ms(passes=True)
    lc.close()
    return recorded, lengths, akw, results, ms


def compare(results, golden, prefix, names, worst):
    for i, (name, got) in enumerate(zip(names, results)):
        got = dataclasses.asdict(got)
        for field in LO.DISCRETE_FIELDS:
            assert got[field] == golden[prefix + field][i], (name, field, got[field], golden[prefix + field][i])
        assert got["estimated_one_way_ms"] == 0.0 and got["directional_latency_ms"] is None
        for field in LO.FLOAT_FIELDS:
            worst[field] = max(worst[field], abs(got[field] - float(golden[prefix + field][i])))


def check(worst):
    for field, value in worst.items():
        print(f"largest |GPU - golden| {field}: {value:.3e} (allowed {allowed(field):.3e})")
    for field, value in worst.items():
        assert value <= allowed(field), (field, value)
        assert allowed(field) < 1e-3 * DECISION_MARGIN


def test_probes_are_bit_equal_at_the_four_rates(mi, golden):
    for rate in LS.RATES:
        assert np.array_equal(mi.generate_probe_signal(rate, LS.PROBE_MS[rate]), golden[f"probe_{rate}"])


def test_cases_against_the_reference(mi, golden):
    names = [str(n) for n in golden["names"]]
    assert names == list(LS.CASES)
    results = []
    for name in names:
        rate, _, akw = LS.CASES[name]
        results.append(mi.analyze_latency(LS.probe(rate), LS.recording(name), rate, **akw))
    for name, r in zip(names, results):
        print(f"{name:16s} {r.success!s:5s} {r.measured_round_trip_ms:10.4f} ms conf {r.confidence:.4f} reps {r.repetition_count} {r.message}")
    worst = dict.fromkeys(LO.FLOAT_FIELDS, 0.0)
    compare(results, golden, "case_", names, worst)
    check(worst)
    exact = names.index("silence")  # every sum is exactly 0 in both arithmetics
    for field in LO.FLOAT_FIELDS:
        assert getattr(results[exact], field) == float(golden["case_" + field][exact]), field


def test_batch_of_70_against_the_reference(batch, golden):
    _, _, _, results, ms = batch
    print(f"batch of {LS.BATCH}: {ms[0]:.3f} ms on the device, {ms[1]}")
    worst = dict.fromkeys(LO.FLOAT_FIELDS, 0.0)
    compare(results, golden, "batch_", [f"stream {s}" for s in range(LS.BATCH)], worst)
    check(worst)
    assert len({r.message for r in results}) >= 5  # the exits and the verdicts are all in the batch


def test_batch_equals_one_at_a_time_bit_for_bit(mi, batch):
    recorded, lengths, akw, results, _ = batch
    lc = mi.LatencyCalibration(48_000, LS.probe(), 1, LS.LONG)
    for s in range(LS.BATCH):
        alone = lc.analyze(recorded[s : s + 1, : int(lengths[s])], max_search_ms=akw["max_search_ms"][s])[0]
        assert dataclasses.asdict(alone) == dataclasses.asdict(results[s]), s  # == on floats: the same bits (no NaN, no -0.0 here)
    lc.close()


def test_analyze_device_equals_analyze_bit_for_bit(mi, batch):
    import torch

    recorded, lengths, akw, results, _ = batch
    stride = LS.LONG + 37
    host = np.full((LS.BATCH, stride), 7.0, dtype=np.float32)  # beyond the rows: never read
    host[:, : LS.LONG] = recorded
    d_recorded = torch.from_numpy(host).cuda()
    lc = mi.LatencyCalibration(48_000, LS.probe(), LS.BATCH, LS.LONG)
    got = lc.analyze_device(d_recorded.data_ptr(), stride, LS.BATCH, lengths, **akw)
    lc.close()
    assert [dataclasses.asdict(r) for r in got] == [dataclasses.asdict(r) for r in results]


def test_batch_keywords_per_stream_and_early_exits_do_not_stop_the_batch(mi, golden):
    names = ["clean_short", "bad_window", "bad_route", "non_finite", "too_short", "clean_short"]
    recorded = np.zeros((len(names), LS.SHORT), dtype=np.float32)
    lengths = []
    for s, name in enumerate(names):
        x = LS.recording(name)
        recorded[s, : x.size] = x
        lengths.append(x.size)
    got = mi.analyze_latency_batch(LS.probe(), recorded, 48_000, lengths, max_search_ms=[500.0, 4.0, 500.0, 500.0, 500.0, 500.0],
                                   route_kind=[None, "output_to_input", "input_to_output", "OUTPUT_TO_INPUT ", "", "output_to_input"])
    all_names = [str(n) for n in golden["names"]]
    for name, r in zip(names, got):
        i = all_names.index(name)
        for field in LO.DISCRETE_FIELDS:
            assert getattr(r, field) == golden["case_" + field][i], (name, field)
    assert got[3].message == LO.NON_FINITE_MESSAGE and not got[3].success
    assert dataclasses.asdict(got[0]) == dataclasses.asdict(got[5])
