"""The float64 stage reference (tests/suppressor_stage_ref.py) against the CPU restatement's taps, and the stimulus' self-test.
No GPU.

This validates the reference -- an f32 implementation written independently of it (oracle/af_rnnoise.c, in either
evaluation order) must sit within f32 rounding of it at every stage -- and it measures, per stage, the f32 restatement's own
distance from f64.  That distance, on the same stimulus and metric, is what tests/test_gpu_suppressor_stages.py allows the
device four times of.  The caps below are ten times the figures the stages showed when they were first measured
(independently computed, not teacher-forced: kat_signal at gains 1, 0.02 and 2; 120 frames): sanity only.

Measured here, teacher-forced, eval order 0 / 1, on the 19 read streams x 52 frames of the stimulus (seed-0x5EED weights):
  X 2.3e-7 / 2.3e-7 of peak     P 2.6e-7 / 2.6e-7     Ex 2.8e-7 / 1.2e-6 relative     Ep 2.6e-7 / 6.8e-7
  Exp 3.1e-7 / 8.8e-7           features 3.8e-5 / 3.8e-5 (|feature| up to 83; the worst is the spectral variability, a sum
  of squared cepstral distances)   gains_raw 4.7e-7 / 2.8e-7     output 1.4e-7 / 1.4e-7 of full scale
"""
import numpy as np
import pytest

import suppressor_stage_ref as R
import suppressor_stage_stimulus as T

# ten times the first-measured figures; the output frame has none of its own: it is an f32 960-point transform of a signal that
# peaks at full scale at the most, windowed and added to one more such frame, so it takes the spectra's figure
CAPS = {"X": 2.4e-6, "P": 2.4e-6, "Ex": 1.0e-4, "Ep": 1.0e-4, "Exp": 5.5e-5, "feat": 9.4e-5, "gains_raw": 1.7e-6, "out": 2.4e-6}
CAPS_EXTREME = dict(CAPS, gains_raw=6.4e-6)  # the blob with -128 / +-127 entries: larger pre-activations


@pytest.mark.parametrize("eval_order", [0, 1])
@pytest.mark.parametrize("kind", T.RUNS)
def test_reference_against_the_restatement(oracle, kind, eval_order):
    run = T.restatement(kind, eval_order)
    res = run["result"]
    caps = CAPS_EXTREME if kind == "extreme" else CAPS
    for stage in R.STAGES:
        value, f, s = R.worst(res["err"][stage])
        print(f"{kind} order {eval_order}: {stage:9s} restatement vs f64 {value:.3e} (frame {f}, stream {run['streams'][s]}); "
              f"device bound {R.bound(stage, res):.3e}")
        assert value <= caps[stage], (stage, value, f, run["streams"][s])
    for name, cells in res["fails"].items():
        assert cells == [], (name, cells[:8])
    # a silent frame has no gains: the tap reads zeros there (and nowhere else)
    sil = run["taps"]["silence"] != 0
    assert np.all(run["taps"]["gains"][sil] == 0.0) and np.all(run["taps"]["gains_raw"][sil] == 0.0)
    assert np.all(run["taps"]["gains"][~sil] > 0.0)


def test_stimulus_self_test(oracle):
    """What the GPU tests rely on the stimulus for, from the restatement alone."""
    run = T.restatement("synthetic")
    taps, streams = run["taps"], run["streams"]
    sil = taps["silence"] != 0
    col = {s: i for i, s in enumerate(streams)}
    for s, role in T.ROLES.items():
        count = int(sil[:, col[s]].sum())
        if role in T.SILENT_ROLES:
            assert count >= 10, (s, role, count)
        elif role == "near":
            assert count >= 10, (s, role, count)  # (12 at first measurement)
        else:
            assert count == 0, (s, role, count)
    # the two zeroed spans together
    assert "".join("1" if v else "0" for v in sil[:, col[3]]) == "111" + "0" * 23 + "1" * 10 + "0" * 16
    # a 16-stream network tile in which the silent frames differ between streams, next to streams that are never silent
    tile0 = [col[s] for s in streams if s < 16]
    patterns = {tuple(sil[:, i]) for i in tile0}
    assert len(patterns) >= 3 and tuple(np.zeros(T.N_FRAMES, dtype=bool)) in patterns
    # one of the silent spans crosses a call boundary
    boundaries = np.cumsum(T.CALLS)[:-1]
    assert any(sil[b - 1, col[s]] and sil[b, col[s]] for b in boundaries for s in (3, 5))
    # no frame near the silence threshold (such frames would be left out of the flag check)
    total = np.sum(taps["Ex"].astype(np.float64), axis=2)
    distance = np.abs(total - R.SILENCE_THRESHOLD) / R.SILENCE_THRESHOLD
    print(f"nearest band-energy sums around the 0.04 threshold: {np.min(total[total >= 0.04]):.4g} above, "
          f"{np.max(total[total < 0.04]):.4g} below")
    assert float(distance.min()) > 1e-2 and run["result"]["fails"]["near_threshold"] == []
    # both ends of the pitch range
    pitch = taps["pitch_index"]
    assert np.any(pitch <= 61) and np.any(pitch >= 760) and pitch.min() >= 60 and pitch.max() <= 768


def test_extreme_blob_does_not_saturate_the_network(oracle):
    """The loaded-weights test can only see a wrong weight if the gains are not pinned at 0 or 1."""
    run = T.restatement("extreme")
    blob = np.frombuffer(run["blob"], dtype=np.int8)
    for v in T.EXTREME_WEIGHTS:
        assert np.count_nonzero(blob == v) > 100, v
    g = run["taps"]["gains_raw"][run["taps"]["silence"] == 0]
    inside = float(np.mean((g > 0.02) & (g < 0.98)))
    print(f"extreme blob: gains_raw {g.min():.3f} .. {g.max():.3f}, {100 * inside:.0f} % inside (0.02, 0.98)")
    assert inside >= 0.9


def test_reference_tells_the_mutants(oracle):
    """The reference with one rule broken must stand out against CORRECT taps by far more than the device's bound: holding the
    GRU states of a silent stream, not advancing the cepstral ring on a silent frame, the doubling of the last band."""
    run = T.restatement("synthetic")
    res, taps = run["result"], run["taps"]
    after = R.first_frames_after_silence(taps["silence"])
    assert len(after) >= 8
    mutant = R.evaluate(run["model_input"], taps, taps["out"], run["blob"], hold_silent=False)
    gaps = [mutant["err"]["gains_raw"][f, s] for f, s in after if f > 3]  # (after the mid-run silence: the states are not zero)
    print(f"GRU states not held through silence: gains_raw off by {min(gaps):.2e} .. {max(gaps):.2e} on the first live frame")
    assert min(gaps) > 10 * R.bound("gains_raw", res)
    mutant = R.evaluate(run["model_input"], taps, taps["out"], run["blob"], advance_on_silence=True)
    gaps = [mutant["err"]["feat"][f, s] for f, s in after if f > 3]
    print(f"cepstral ring advanced on silent frames: features off by {min(gaps):.2e} .. {max(gaps):.2e} on the first live frame")
    assert min(gaps) > 10 * R.bound("feat", res)
    X = taps["X"][5].astype(np.complex128)
    ex, _, _ = R.band_values_f64(X, X)
    assert np.all(np.abs(taps["Ex"][5][:, -1] / ex[:, -1] - 1.0) < 1e-5)  # the last band is doubled (half of it: off by 0.5)


def test_f32_biquad_restatement_is_f32(oracle):
    """The model-input high-pass must be evaluated in f32: in f64 the same recurrence moves bin 0 by ~1e-3 of the frame peak."""
    run = T.restatement("synthetic")
    x = run["model_input"][:1]
    y32 = R.biquad_hp_f32(x, np.zeros((1, 2), dtype=np.float32)).astype(np.float64)
    y64 = np.empty(x.shape[1])
    m0 = m1 = 0.0
    b0, b1, a0, a1 = (float(np.float32(v)) for v in (-2.0, 1.0, -1.99599, 0.99600))
    for i, xi in enumerate(x[0].astype(np.float64)):
        yi = xi + m0
        m0, m1 = m1 + (b0 * xi - a0 * yi), b1 * xi - a1 * yi
        y64[i] = yi
    worst = 0.0
    for f in range(2, T.N_FRAMES):
        a = R.spectrum_f64(y32[:, (f - 1) * 480:(f + 1) * 480])[0]
        b = R.spectrum_f64(y64[None, (f - 1) * 480:(f + 1) * 480])[0]
        worst = max(worst, float(np.max(np.abs(a - b)) / np.max(np.abs(a))))
    print(f"f64 against f32 high-pass recurrence: spectra differ by up to {worst:.2e} of the frame peak")
    assert worst > 20 * CAPS["X"]
