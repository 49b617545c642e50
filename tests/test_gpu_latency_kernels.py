"""The kernels of the latency calibration (csrc/af_latency.hip) through LatencyCalibration.scores() against the NumPy
restatement, tests/latency_oracle.py, on the long shape (33600 samples: a 65536-point transform, the four-step form) and the
short one (4200: 8192 points, one workgroup in LDS):

* the lags of the whole-probe search and of every burst window are equal, and so is the lag range of the PHAT window;
* window_energy is BIT-EQUAL: the device's energy prefix is np.cumsum's sequential sum and the mean under it NumPy's pairwise one;
* the normalised scores and the PHAT correlation inside the windows are within 4 x the largest difference measured on the
  MI355X (MEASURED_* below and DESIGN 4.23; printed before the assertion).  The expectation from the bounds (probe length x u
  for a direct sum, u log n for a transform) is 1e-12 or less.

And the forward transform alone at 2^13 (LDS form), 2^16 and 2^17 real points (four-step form) on seeded noise against
np.fft.rfft, relative to the largest bin."""
import numpy as np
import pytest

import latency_oracle as LO
import latency_stimulus as LS

pytestmark = pytest.mark.gpu

# the largest |GPU - oracle| over both shapes, measured on the MI355X
MEASURED_FULL_SCORE = 3.664e-15
MEASURED_BURST_SCORE = 1.444e-15
MEASURED_PHAT = 8.466e-16
# the largest |GPU - np.fft.rfft| / max |bin| over the three lengths
MEASURED_RFFT = 4.610e-16  # 2^13: 4.610e-16, 2^16: 3.945e-16, 2^17: 4.076e-16
SHAPES = ("clean_long", "clean_short", "dc_offset", "weak_probe")


@pytest.fixture(scope="module")
def mi():
    import mic_eq_mi

    return mic_eq_mi


@pytest.fixture(scope="module")
def measured(mi):
    """-> {case: (device scores, oracle trace)}; the four recordings go through one batch with ragged lengths"""
    recorded = np.zeros((len(SHAPES), LS.LONG), dtype=np.float32)
    lengths = []
    for s, name in enumerate(SHAPES):
        x = LS.recording(name)
        recorded[s, : x.size] = x
        lengths.append(x.size)
    lc = mi.LatencyCalibration(48_000, LS.probe(), len(SHAPES), LS.LONG)
    lc.analyze(recorded, lengths)
    out = {}
    for s, name in enumerate(SHAPES):
        trace = {}
        LO.analyze_latency(LS.probe(), recorded[s, : lengths[s]], 48_000, trace=trace)
        out[name] = (lc.scores(s), trace)
    lc.close()
    return out


@pytest.mark.parametrize("name", SHAPES)
def test_lags_are_equal_and_window_energy_is_bit_equal(measured, name):
    got, trace = measured[name]
    assert np.array_equal(got["full"]["lags"], trace["full_lags"])
    assert got["full"]["window_energy"].tobytes() == trace["full_energy"].tobytes()
    assert len(got["bursts"]) == len(trace["bursts"]) == 4
    for part, want in zip(got["bursts"], trace["bursts"]):
        assert part["offset"] == want["offset"]
        assert np.array_equal(part["lags"], want["lags"])
        assert part["window_energy"].tobytes() == want["energy"].tobytes()
        assert part["lags"].size > 0
        n = 8192 if name == "clean_short" else 65536  # the short shape's last window is cut at n / 2 = 4096, :192-193
        assert np.array_equal(part["phat_lags"], LO.phat_window(np.zeros(n), n, want["lag_min"], want["lag_max"])[0])


def test_scores_and_phat_against_the_oracle(measured):
    worst = {"full": 0.0, "burst": 0.0, "phat": 0.0}
    for name in SHAPES:
        got, trace = measured[name]
        worst["full"] = max(worst["full"], float(np.max(np.abs(got["full"]["scores"] - trace["full_scores"]))))
        rec = LO.normalize_audio(LS.recording(name))
        corr, n = LO.phat_correlation(rec, LO.coded_probe_components(48_000, LS.probe().size)[0])
        for part, want in zip(got["bursts"], trace["bursts"]):
            worst["burst"] = max(worst["burst"], float(np.max(np.abs(part["scores"] - want["scores"]))))
            worst["phat"] = max(worst["phat"], float(np.max(np.abs(part["phat"] - corr[part["phat_lags"] % n]))))
            if "phat_hint" in want:
                assert int(part["phat_lags"][int(np.argmax(np.abs(part["phat"])))]) == want["phat_hint"]
    print(f"largest |GPU - oracle|: whole-probe score {worst['full']:.3e}, burst score {worst['burst']:.3e}, PHAT correlation {worst['phat']:.3e}")
    assert worst["full"] <= 4.0 * MEASURED_FULL_SCORE
    assert worst["burst"] <= 4.0 * MEASURED_BURST_SCORE
    assert worst["phat"] <= 4.0 * MEASURED_PHAT
    assert 4.0 * max(MEASURED_FULL_SCORE, MEASURED_BURST_SCORE, MEASURED_PHAT) < 1e-7  # orders under the 1e-4 decision margin


def test_forward_transform_alone_against_numpy(mi):
    lc = mi.LatencyCalibration(48_000, LS.probe(), 1, LS.LONG)
    worst = {}
    for bits in (13, 16, 17):
        x = np.random.default_rng(bits).standard_normal(1 << bits).astype(np.float32)
        want = np.fft.rfft(x.astype(np.float64))
        got = lc.debug_rfft(x)
        assert got.shape == want.shape
        worst[bits] = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    lc.close()
    print("largest |GPU - np.fft.rfft| / max |bin|: " + ", ".join(f"2^{b}: {v:.3e}" for b, v in worst.items()))
    for bits, value in worst.items():
        assert value <= 4.0 * MEASURED_RFFT, (bits, value)
    assert 4.0 * MEASURED_RFFT < 1e-12
