"""tests/latency_oracle.py (this project's NumPy-only restatement) against tests/golden/latency_calibration.npz, which
tools/gen_golden_latency.py wrote by running the reference's own latency_calibration.py on tests/latency_stimulus.py.

Discrete fields are equal.  The float fields, and the score arrays the file holds for two cases, are within 4 x the largest
difference measured here on the CPU (the constants below; printed before the assertion): the restatement sums a correlation
directly where the reference goes through scipy's FFT, and both take the same NumPy transforms for GCC-PHAT."""
import numpy as np
import pytest

import latency_oracle as LO
import latency_stimulus as LS

# measured on the CPU (NumPy 2, scipy 1.15.3 behind the golden file)
MEASURED_FIELD = {"measured_round_trip_ms": 0.0, "sub_sample_offset": 0.0, "confidence": 3.886e-16, "agreement_ms": 0.0,
                  "ambiguity_score": 5.551e-16, "route_latency_ms": 0.0, "applied_compensation_ms": 0.0}
MEASURED_SCORE = 5.773e-14  # the reference's correlation is scipy's FFT of 2^16 points: its rounding, not the direct sum's
# The PHAT correlation measured 0: the file was written with the same NumPy transforms.  Another NumPy build may round a
# transform differently, so what is allowed is the transform's own rounding, u log2(n) for n = 2^16, not 0.
MEASURED_PHAT = 2.0**-53 * 16


@pytest.fixture(scope="module")
def golden():
    return np.load(LS.GOLDEN)


def compare(rows, golden, prefix, worst):
    for i, row in enumerate(rows):
        for field in LO.DISCRETE_FIELDS:
            assert row[field] == golden[prefix + field][i], (prefix, i, field, row[field], golden[prefix + field][i])
        assert row["estimated_one_way_ms"] == 0.0 and row["directional_latency_ms"] is None
        for field in LO.FLOAT_FIELDS:
            worst[field] = max(worst[field], abs(row[field] - float(golden[prefix + field][i])))


def test_golden_file_is_small_and_holds_data_only(golden):
    assert LS.GOLDEN.stat().st_size < 150_000
    assert all(golden[key].dtype.kind in "fiU" for key in golden.files)
    assert [str(n) for n in golden["names"]] == list(LS.CASES)


def test_probes_are_the_reference_probes_bit_for_bit(golden):
    for rate in LS.RATES:
        got = LO.generate_probe_signal(rate, LS.PROBE_MS[rate])
        assert got.dtype == np.float32 and np.array_equal(got, golden[f"probe_{rate}"])


def test_results_against_the_reference(golden):
    worst = dict.fromkeys(LO.FLOAT_FIELDS, 0.0)
    rows = []
    for name, (rate, _, akw) in LS.CASES.items():
        rows.append(LO.analyze_latency(LS.probe(rate), LS.recording(name), rate, **akw))
    compare(rows, golden, "case_", worst)
    recorded, lengths, akw = LS.batch()
    rows = [LO.analyze_latency(LS.probe(), recorded[s, : lengths[s]], 48_000, max_search_ms=akw["max_search_ms"][s]) for s in range(LS.BATCH)]
    compare(rows, golden, "batch_", worst)
    for field, value in worst.items():
        print(f"largest |oracle - golden| {field}: {value:.3e}")
    for field, value in worst.items():
        assert value <= 4.0 * MEASURED_FIELD[field], (field, value)
    messages = {row["message"] for row in rows}
    assert len(messages) >= 5 and LO.NON_FINITE_MESSAGE in messages


@pytest.mark.parametrize("name", LS.SCORE_CASES)
def test_score_arrays_against_the_reference(golden, name):
    trace = {}
    LO.analyze_latency(LS.probe(), LS.recording(name), 48_000, trace=trace)
    lags = golden[f"scores_{name}_full_lags"]
    at = lags - trace["full_lags"][0]
    assert np.array_equal(trace["full_lags"][at], lags)
    worst = float(np.max(np.abs(trace["full_scores"][at] - golden[f"scores_{name}_full"])))
    worst_phat = 0.0
    for k, entry in enumerate(trace["bursts"]):
        assert np.array_equal(entry["lags"], golden[f"scores_{name}_burst{k}_lags"])
        worst = max(worst, float(np.max(np.abs(entry["scores"] - golden[f"scores_{name}_burst{k}"]))))
        inside = np.isin(entry["lags"], entry["phat_lags"])
        assert np.array_equal(entry["lags"][inside], entry["phat_lags"][np.isin(entry["phat_lags"], entry["lags"])])
        want = golden[f"scores_{name}_phat{k}"][inside]
        got = entry["phat_abs"][np.isin(entry["phat_lags"], entry["lags"])]
        worst_phat = max(worst_phat, float(np.max(np.abs(got - np.abs(want)))))
    print(f"{name}: largest |oracle - golden| score {worst:.3e}, PHAT correlation {worst_phat:.3e}")
    assert worst <= 4.0 * MEASURED_SCORE and worst_phat <= 4.0 * MEASURED_PHAT
