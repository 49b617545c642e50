"""The reference's own unit tests of its input mixdown (input.rs:1141-1430), restated one for one on tests/ref/mixdown_ref.c:
same inputs, same assertions.  This is what holds the restatement to the reference; the GPU tests then hold the kernels to
the restatement bit for bit.  (The #[ignore]d benchmark and the device-listing test are not restated.)"""
import math

import numpy as np

import mixdown_oracle as MO

F = np.float32
HISTORY, LATENCY = MO.HISTORY, MO.LATENCY


def mix_average(interleaved, channels, mono):
    """mix_interleaved_to_mono (input.rs:739-751): writes into `mono`, returns the frames written."""
    w, out, _, _ = MO.mix_with_mode(interleaved, channels, MO.AVERAGE, len(mono))
    mono[:w] = out[:w]
    return w


def test_mix_interleaved_stereo_input_to_mono_average():
    mono = np.zeros(4, dtype=F)
    written = mix_average([1.0, 1.0, 0.25, 0.75], 2, mono)
    assert written == 2
    assert abs(mono[0] - 1.0) < 1e-6
    assert abs(mono[1] - 0.5) < 1e-6


def test_mix_interleaved_stereo_input_preserves_phase_cancellation():
    mono = np.ones(4, dtype=F)
    written = mix_average([1.0, -1.0, 0.5, -0.5], 2, mono)
    assert written == 2
    assert all(abs(s) < 1e-6 for s in mono[:written])


def test_mix_interleaved_multichannel_input_does_not_switch_with_alternating_loudness():
    mono = np.zeros(4, dtype=F)
    written = mix_average([1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 1.0], 2, mono)
    assert written == 4
    assert all(abs(s - 0.5) < 1e-6 for s in mono[:written])


def test_mix_interleaved_multichannel_input_is_stable_and_bounded():
    mono = np.zeros(4, dtype=F)
    written = mix_average([1.0, 0.5, -0.5, -1.0, -0.5, 0.5], 3, mono)
    assert written == 2
    assert abs(mono[0] - F(1.0 / 3.0)) < 1e-6
    assert abs(mono[1] + F(1.0 / 3.0)) < 1e-6
    assert all(abs(s) <= 1.0 for s in mono[:written])


def test_mix_interleaved_left_and_right_modes_select_channels():
    interleaved = [0.75, -0.25, 0.5, -0.5]
    written, mono, _, _ = MO.mix_with_mode(interleaved, 2, MO.LEFT, 2)
    assert written == 2
    assert mono.tolist() == [0.75, 0.5]
    written, mono, _, _ = MO.mix_with_mode(interleaved, 2, MO.RIGHT, 2)
    assert written == 2
    assert mono.tolist() == [-0.25, -0.5]


def test_mix_interleaved_max_rms_selects_one_channel_for_whole_block():
    interleaved = np.array([0.1, 0.9, 0.8, 0.2, 0.1, -0.9, 0.8, -0.2], dtype=F)
    written, mono, _, _ = MO.mix_with_mode(interleaved, 2, MO.MAX_RMS, 4)
    assert written == 4
    assert np.array_equal(mono, np.array([0.9, 0.2, -0.9, -0.2], dtype=F))


def test_mix_interleaved_reports_negative_stereo_correlation():
    written, _, correlation, _ = MO.mix_with_mode([1.0, -1.0, 0.5, -0.5, -0.25, 0.25], 2, MO.AVERAGE, 3)
    assert written == 3
    assert correlation is not None and correlation < MO.WARNING_CORRELATION


def test_phase_safe_mono_recovers_anti_phase_with_polarity_flip():
    written, mono, correlation, (strategy, delay, flipped) = MO.mix_with_mode([0.5, -0.5, 0.25, -0.25, -0.5, 0.5], 2,
                                                                              MO.PHASE_SAFE_MONO, 3)
    assert written == 3
    assert correlation < MO.WARNING_CORRELATION
    assert strategy == MO.POLARITY_FLIP
    assert flipped
    assert abs(delay) < 0.25
    assert abs(mono[0] - 0.5) < 1e-6
    assert abs(mono[1] - 0.25) < 1e-6
    assert abs(mono[2] + 0.5) < 1e-6


def test_phase_safe_mono_aligns_delayed_stereo():
    frames, delay = 256, 3
    sr, freq = F(48_000.0), F(1_000.0)
    t = np.arange(frames, dtype=F) / sr
    left = (np.sin(F(2.0) * F(math.pi) * freq * t).astype(F) * F(0.5)).astype(F)
    interleaved = np.zeros(frames * 2, dtype=F)
    interleaved[0::2] = left
    interleaved[2 * delay + 1::2] = left[: frames - delay]

    written, mono, _, (strategy, estimated, _) = MO.mix_with_mode(interleaved, 2, MO.PHASE_SAFE_MONO, frames)

    average_error = aligned_error = F(0.0)
    output_delay = delay + LATENCY
    for idx in range(output_delay + HISTORY, written - delay):
        reference = left[idx - output_delay]
        average = F(0.5) * (interleaved[idx * 2] + interleaved[idx * 2 + 1])
        average_error += (average - reference) ** 2
        aligned_error += (mono[idx] - reference) ** 2
    average_error, aligned_error = np.sqrt(average_error), np.sqrt(aligned_error)

    assert strategy == MO.FRACTIONAL_DELAY
    assert abs(estimated - delay) < 0.6, f"estimated delay {estimated}"
    assert aligned_error < average_error * 0.6, f"aligned_error={aligned_error} average_error={average_error}"


def test_phase_safe_mono_leaves_normal_stereo_average_unchanged():
    written, mono, correlation, (strategy, _, _) = MO.mix_with_mode([0.5, 0.5, -0.25, -0.25, 0.1, 0.1], 2, MO.PHASE_SAFE_MONO, 3)
    assert written == 3
    assert strategy == MO.NONE
    assert correlation > 0.99
    assert np.array_equal(mono, np.array([0.5, -0.25, 0.1], dtype=F))


def test_lagrange_fractional_delay_reduces_sweep_null_error_vs_linear():
    sample_rate, duration_samples = 48_000.0, 48_000
    delay = F(5.35)
    history = np.zeros(HISTORY, dtype=F)
    lagrange_error = linear_error = 0.0
    measured = 0

    def sweep_sample(position):
        time = position / sample_rate
        sweep_rate = (18_000.0 - 500.0) / (duration_samples / sample_rate)
        phase = 2.0 * math.pi * (500.0 * time + 0.5 * sweep_rate * time * time)
        return F(0.5 * math.sin(phase))

    for index in range(duration_samples):
        history[1:] = history[:-1].copy()
        history[0] = sweep_sample(float(index))
        if index < HISTORY:
            continue
        reference = sweep_sample(float(index) - float(delay))
        lagrange = MO.lagrange_sample(history, delay)
        lower = int(math.floor(delay))
        fraction = delay - F(lower)
        linear = history[lower] * (F(1.0) - fraction) + history[lower + 1] * fraction
        lagrange_error += float((lagrange - reference) ** 2)
        linear_error += float((linear - reference) ** 2)
        measured += 1

    lagrange_rms = math.sqrt(lagrange_error / measured)
    linear_rms = math.sqrt(linear_error / measured)
    assert lagrange_rms < linear_rms * 0.60, f"lagrange_rms={lagrange_rms} linear_rms={linear_rms}"


def test_phase_safe_fractional_delay_state_survives_callback_boundaries():
    sample_rate, frames, delay = 48_000.0, 2048, 3.4

    def source(position):
        time = position / sample_rate
        return F(0.22 * math.sin(2.0 * math.pi * 3100.0 * time) + 0.16 * math.sin(2.0 * math.pi * 9100.0 * time)
                 + 0.09 * math.sin(2.0 * math.pi * 15_000.0 * time))

    interleaved = np.zeros(frames * 2, dtype=F)
    for index in range(frames):
        interleaved[index * 2] = source(float(index))
        interleaved[index * 2 + 1] = source(float(index) - delay)

    state = MO.Mixdown(2, MO.PHASE_SAFE_MONO)
    output = np.zeros(frames, dtype=F)
    callback_frames = 128
    for start in range(0, frames, callback_frames):
        end = min(start + callback_frames, frames)
        w, mono, _, (strategy, _, _) = state.mix(interleaved[start * 2:end * 2], end - start)
        output[start:end] = mono[:w]
        assert strategy == MO.FRACTIONAL_DELAY

    expected_delay = delay + LATENCY
    square_error = square_reference = 0.0
    max_boundary_error = F(0.0)
    for index in range(HISTORY * 2, frames):
        reference = source(float(index) - expected_delay)
        error = output[index] - reference
        square_error += float(error * error)
        square_reference += float(reference * reference)
        if index % callback_frames == 0:
            max_boundary_error = max(max_boundary_error, abs(error))
    relative_null = math.sqrt(square_error / max(square_reference, 1e-12))
    assert relative_null < 0.18, f"relative_null={relative_null}"
    assert max_boundary_error < 0.12, f"max_boundary_error={max_boundary_error}"
