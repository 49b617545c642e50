"""The reference's own assertions on the restatement (tests/ref/output_writer_ref.c): the three retime_audio_block tests
(rust-core/src/audio/processor/tests.rs:829-851, 1030-1085), the six test_output_writer_* tests (:1145-1574) with their
limits and scratch sizes, and test_duration_samples_for_44k1_output (:9-13).  A restatement that fails one of these is
not the reference, whatever the GPU agrees with."""
import numpy as np
import pytest

import output_writer_oracle as O

F = np.float32


def test_duration_samples_for_44k1_output():
    """tests.rs:9-13"""
    assert O.duration_samples(44_100, 30) == 1323
    assert O.duration_samples(44_100, 40) == 1764
    assert O.duration_samples(44_100, 60) == 2646


def test_retime_audio_block_can_expand_and_compress():
    """tests.rs:829-839"""
    x = np.asarray([0.0, 0.25, 0.5, 0.75, 1.0, 0.5], dtype=F)
    assert O.retime(x, 0.5, 32, 32).size > x.size
    assert O.retime(x, 2.0, 32, 32).size < x.size


def test_retime_audio_block_linear_interpolation_does_not_overshoot_neighbors():
    """tests.rs:841-851"""
    y = O.retime(np.asarray([0.0, 0.5, 1.0, 0.5, 0.0], dtype=F), 0.7, 32, 32)
    assert y.size > 5 and ((y >= 0.0) & (y <= 1.0)).all()


# ---- tests.rs:913-1004, restated
def _dbfs(v):
    return float(F(np.log10(max(F(v), F(1e-12)))) * F(20.0))


def _tone_components(sig, rate, hz):
    omega = 2.0 * np.pi * float(F(hz)) / float(F(rate))
    ph = omega * np.arange(sig.size, dtype=np.float64)
    s = sig.astype(np.float64)
    scale = 2.0 / max(sig.size, 1)
    return float(np.sum(s * np.cos(ph)) * scale), float(np.sum(s * np.sin(ph)) * scale)


def _tone_amplitude(sig, rate, hz):
    return float(F(np.hypot(*_tone_components(sig, rate, hz))))


def _max_harmonic_db(sig, rate, hz):
    m = 0.0
    for h in range(2, 6):
        if hz * h >= rate / 2.0:
            break
        m = max(m, _tone_amplitude(sig, rate, hz * h))
    return _dbfs(m)


def _residual(sig, rate, hz):
    c, s = _tone_components(sig, rate, hz)
    ph = 2.0 * np.pi * float(F(hz)) / float(F(rate)) * np.arange(sig.size, dtype=np.float64)
    return sig - (c * np.cos(ph) + s * np.sin(ph)).astype(F)


def _rms_db(sig):
    return -120.0 if sig.size == 0 else _dbfs(np.sqrt(np.mean(sig.astype(np.float64) ** 2)))


def _sinc_reference_retime(x, speed_ratio, taps=128):
    """A windowed-sinc retime in this test's own code, standing where the reference's test uses a 128-tap
    Blackman-Harris-squared sinc resampler: output frame i reads the input at i * speed_ratio, without delay."""
    n_out = int(round(x.size / speed_ratio))
    pos = np.arange(n_out, dtype=np.float64) * float(speed_ratio)
    base = np.floor(pos).astype(np.int64)
    k = np.arange(-taps // 2 + 1, taps // 2 + 1)
    idx = base[:, None] + k[None, :]
    d = pos[:, None] - idx
    fc = 0.9 * min(1.0, 1.0 / float(speed_ratio))  # below Nyquist of the slower side
    u = d / (taps / 2.0)  # -1 .. 1 across the window
    a0, a1, a2, a3 = 0.35875, 0.48829, 0.14128, 0.01168
    win = (a0 + a1 * np.cos(np.pi * u) + a2 * np.cos(2 * np.pi * u) + a3 * np.cos(3 * np.pi * u)) ** 2
    win[np.abs(u) > 1.0] = 0.0
    h = fc * np.sinc(fc * d) * win
    valid = (idx >= 0) & (idx < x.size)
    xs = np.where(valid, x.astype(np.float64)[np.clip(idx, 0, x.size - 1)], 0.0)
    return np.sum(xs * h, axis=1).astype(F)


@pytest.mark.parametrize("speed_ratio,max_error_db,max_fundamental_delta_db",
                         [(0.995, -20.0, 1.5), (1.003, -20.0, 1.5), (1.03, -16.0, 2.0), (1.06, -12.0, 2.5)])
def test_retime_audio_block_quality_stays_within_measured_reference_bounds(speed_ratio, max_error_db, max_fundamental_delta_db):
    """tests.rs:1030-1085"""
    rate = 48_000.0
    i = np.arange(48_000, dtype=F)
    x = (F(0.8) * np.sin(F(2.0) * F(np.pi) * F(10_000.0) * i / F(rate), dtype=F)).astype(F)
    linear = O.retime(x, speed_ratio, 96_000, 96_000)
    reference = _sinc_reference_retime(x, F(speed_ratio))
    n = min(linear.size, reference.size)
    linear, reference = linear[:n], reference[:n]
    hz = float(F(10_000.0) * F(speed_ratio))
    lin_f, ref_f = _dbfs(_tone_amplitude(linear, rate, hz)), _dbfs(_tone_amplitude(reference, rate, hz))
    assert abs(lin_f - ref_f) <= max_fundamental_delta_db, (lin_f, ref_f)
    err = _dbfs(np.sqrt(np.mean((linear.astype(np.float64) - reference.astype(np.float64)) ** 2)))
    assert err <= max_error_db, err
    assert _max_harmonic_db(linear, rate, hz) <= lin_f - 12.0
    assert _rms_db(_residual(linear, rate, hz)) <= _rms_db(_residual(reference, rate, hz)) + 40.0


# ---- the six writer tests: TruePeakLimiter::default() is 48 kHz (true_peak.rs:395-399)
def _writer(capacity, limits, scratch, limiter, ceiling=1.0):
    w = O.Writer(48_000.0, capacity, *limits, scratch_capacity=scratch)
    w.set_limiter(limiter, ceiling)
    return w


def test_output_writer_noop_write_returns_false():
    """tests.rs:1145-1196"""
    w = _writer(32, (8, 16, 4), 64, True)
    assert w.write_chunk(np.zeros(0, dtype=F), 0).size == 0
    assert w.meters()["fill_after"] == 0 and not any(w.counters().values()) and not any(w.branches().values())


def test_output_writer_accounts_for_queue_full_short_write():
    """tests.rs:1198-1260"""
    w = _writer(4, (2, 4, 4), 64, True)
    out = w.write_chunk(np.asarray([0.1, 0.2, 0.3, 0.4], dtype=F), 3)
    c, m = w.counters(), w.meters()
    assert c["short_write_dropped"] == 3 and c["retime_adjustments"] == 0 and c["recovery_events"] == 1
    assert m["fade_remaining"] == 4 and m["fill_after"] == 4 and out.size == 1


def test_output_writer_retime_can_expand_and_compress_output():
    """tests.rs:1262-1382"""
    x = (np.arange(256) / 255.0).astype(F)
    w = _writer(1024, (128, 256, 4), 512, False)
    w.set_state(-10_000.0, 0)
    out = w.write_chunk(x, 0)
    assert out.size > x.size
    assert w.counters()["retime_adjustments"] == 1 and w.counters()["recovery_events"] == 0
    w = _writer(1024, (128, 256, 4), 512, False)
    w.set_state(10_000.0, 0)
    out = w.write_chunk(x, 256)
    c = w.counters()
    assert 256 < 256 + out.size < x.size + 256
    assert c["jitter_dropped"] > 0 and c["retime_adjustments"] == 1 and c["recovery_events"] == 0


def test_output_writer_applies_discontinuity_fade_after_short_write_drop():
    """tests.rs:1384-1445"""
    w = _writer(8, (4, 8, 4), 64, False)
    ones = np.ones(4, dtype=F)
    first = w.write_chunk(ones, 6)
    assert first.size == 2 and w.meters()["fill_after"] == 8 and w.meters()["fade_remaining"] == 4
    faded = w.write_chunk(ones, 0)  # the test drained the queue
    assert faded.size == 4
    assert 0.0 < faded[0] < faded[1] < faded[2] < faded[3] and abs(faded[3] - 1.0) < 1e-6


def test_output_writer_still_applies_limiter_ceiling_clamp():
    """tests.rs:1447-1500"""
    w = _writer(64, (4, 8, 4), 32, True, 0.5)
    a = w.write_chunk(np.asarray([2.0, -2.0, 0.5, 0.0, 0.0, 0.0, 0.0], dtype=F), 0, clean_path=True)
    b = w.write_chunk(np.zeros(24, dtype=F), a.size, clean_path=True)
    limited = np.concatenate([a, b])
    assert limited.size == 31
    assert (np.abs(limited) <= 0.5 + 1e-6).all() and (np.abs(limited) > 0.1).any()


def test_output_writer_limits_true_peak_without_sample_clip():
    """tests.rs:1502-1574"""
    w = _writer(64, (4, 8, 4), 32, True, 1.0)
    a = w.write_chunk(np.asarray([0.0, 1.0, 1.0, 0.0, 0.0], dtype=F), 0, clean_path=True)
    w.write_chunk(np.zeros(32, dtype=F), a.size, clean_path=True)
    c, m = w.counters(), w.meters()
    assert c["clip_events"] == 0 and c["true_peak_events"] == 1
    assert m["true_peak_db"] <= 0.01 and m["true_peak_input_db"] > 0.0 and m["gain_reduction_db"] > 0.0


def test_update_decaying_peak_db_and_clamp_metrics():
    """routing.rs:651-655 and :768-799 (tests.rs:785-805 for the clip metrics)"""
    assert O.update_decaying_peak_db(3.0, 1.0, 0.15) == F(3.0)
    assert O.update_decaying_peak_db(0.0, 1.0, 0.15) == F(1.0) - F(0.15)
    assert O.update_decaying_peak_db(0.0, 0.1, 0.15) == 0.0 and O.update_decaying_peak_db(-1.0, -5.0, 0.15) == 0.0
    buf, events, peak_db, max_clipped = O.sanitize_and_clamp([0.5, 2.0, -4.0, np.nan, np.inf], 1.0)
    assert buf.tolist() == [0.5, 1.0, -1.0, 0.0, 0.0] and events == 2 and max_clipped == 4.0
    assert abs(peak_db - 20.0 * np.log10(4.0)) < 1e-5
