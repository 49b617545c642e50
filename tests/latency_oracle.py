"""The project's own NumPy-only restatement of the reference's python/mic_eq/analysis/latency_calibration.py (no scipy): the
coded probe (:45-115), the normalised correlation scores (:137-168) as direct sums, GCC-PHAT (:171-198), the peak pick
(:201-229) and analyze_latency (:232-515).  Besides the result it returns every intermediate the device exposes through
LatencyCalibration.scores(), and, for tests/test_latency_stimulus.py, the distance of every decision from its threshold.

The one place where it is not the reference's arithmetic: the correlation is np.correlate's direct sum, not scipy's FFT, so a
normalised score differs from the reference's by rounding (1e-13); tests/test_latency_ref.py measures that against the golden
file."""
from __future__ import annotations

import numpy as np

BARKER_13 = np.array([1.0, 1.0, 1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0], dtype=np.float64)
REPETITIONS = 4
FIELDS = ("success", "measured_round_trip_ms", "estimated_one_way_ms", "applied_compensation_ms", "confidence", "peak_sample_offset",
          "message", "repetition_count", "agreement_ms", "ambiguity_score", "sub_sample_offset", "route_latency_ms",
          "directional_latency_ms", "route_kind", "compensation_basis")
FLOAT_FIELDS = ("measured_round_trip_ms", "sub_sample_offset", "confidence", "agreement_ms", "ambiguity_score", "route_latency_ms",
                "applied_compensation_ms")
DISCRETE_FIELDS = ("success", "message", "peak_sample_offset", "repetition_count", "route_kind", "compensation_basis")
NON_FINITE_MESSAGE = "Recording contains non-finite samples."  # this project's addition; the reference would return NaNs


def coded_probe_components(sample_rate, total_samples, repetitions=REPETITIONS):
    """:74-115"""
    repetitions = max(1, int(repetitions))
    chip = max(4, int(round(sample_rate * 0.0005)))
    min_spacing = max(chip, int(round(sample_rate * 0.006)))
    while chip > 4:
        burst_len = BARKER_13.size * chip
        if repetitions * burst_len + (repetitions - 1) * min_spacing <= total_samples:
            break
        chip -= 1
    code = np.repeat(BARKER_13, chip)
    burst = code * np.hanning(code.size)
    burst -= float(np.mean(burst))
    peak = float(np.max(np.abs(burst)))
    if peak > 0.0:
        burst /= peak
    burst_len = burst.size
    if repetitions == 1 or total_samples <= burst_len:
        return burst[:total_samples], [0]
    spacing = max(min_spacing, max(0, total_samples - repetitions * burst_len) // (repetitions - 1))
    offsets, cursor = [], 0
    for _ in range(repetitions):
        if cursor + burst_len > total_samples:
            break
        offsets.append(cursor)
        cursor += burst_len + spacing
    return burst, offsets or [0]


def generate_probe_signal(sample_rate=48_000, duration_ms=80.0, start_freq_hz=1_500.0, end_freq_hz=9_000.0, amplitude=0.8):
    """:45-71"""
    total = max(1, int(sample_rate * (duration_ms / 1000.0)))
    burst, offsets = coded_probe_components(sample_rate, total)
    probe = np.zeros(total, dtype=np.float64)
    for offset in offsets:
        end = min(total, offset + burst.size)
        if end > offset:
            probe[offset:end] += burst[: end - offset]
    peak = np.max(np.abs(probe))
    if peak > 0.0:
        probe = (probe / peak) * float(amplitude)
    return probe.astype(np.float32)


def normalize_audio(signal):
    signal = np.asarray(signal, dtype=np.float64).flatten()
    return signal if signal.size == 0 else signal - float(np.mean(signal))


def correlation_scores(rec, ref, min_lag, max_lag):
    """:137-168 -> (lags, scores, window_energy); the lags are lo..hi, both inside the capture"""
    lo, hi = max(int(min_lag), 0), min(int(max_lag), rec.size - ref.size)
    if hi < lo:
        return np.empty(0, dtype=np.int64), np.empty(0), np.empty(0)
    lags = np.arange(lo, hi + 1, dtype=np.int64)
    corr = np.correlate(rec[lo : hi + ref.size], ref, mode="valid")
    ref_energy = float(np.sum(ref * ref) + 1e-12)
    prefix = np.concatenate(([0.0], np.cumsum(rec * rec)))
    window_energy = prefix[lags + ref.size] - prefix[lags]
    return lags, np.abs(corr) / np.sqrt(np.maximum(window_energy, 1e-12) * ref_energy), window_energy


def pick_peak(lags, scores, bias):
    """:201-229 with :125-134; the median of the off-peak scores is dropped, every caller discards it"""
    if lags.size == 0:
        return dict(peak_lag=0.0, peak_score=0.0, margin=0.0, ambiguity=1.0, empty=True)
    max_index = int(np.argmax(scores))
    max_score = float(scores[max_index])
    threshold = max_score * float(bias)
    strong = np.flatnonzero(scores >= threshold)
    index = int(strong[0]) if strong.size else max_index
    peak = float(scores[index])
    raw = denom = None
    offset = 0.0
    if 0 < index < scores.size - 1:
        left, right = float(scores[index - 1]), float(scores[index + 1])
        denom = left - 2.0 * peak + right
        if abs(denom) >= 1e-12:
            raw = 0.5 * (left - right) / denom
            offset = float(np.clip(raw, -0.5, 0.5))
    radius = max(1, min(128, scores.size // 50))
    mask = np.ones(scores.size, dtype=bool)
    mask[max(0, index - radius) : index + radius + 1] = False
    off = scores[mask]
    second = float(np.max(off)) if off.size else 0.0
    # the distance of every score up to the chosen one from the threshold, relative
    with np.errstate(divide="ignore", invalid="ignore"):
        clear = np.abs(scores[: index + 1] - threshold) / threshold if threshold > 0.0 else np.full(index + 1, np.inf)
    return dict(peak_lag=float(lags[index]) + offset, peak_score=peak, margin=max(0.0, 1.0 - second / (peak + 1e-6)),
                ambiguity=float(np.clip(second / (peak + 1e-6), 0.0, 1.0)), empty=False, index=index, max_score=max_score,
                raw_offset=raw, denom=denom, threshold_clearance=float(np.min(clear)))


def phat_correlation(rec, burst):
    """:182-189"""
    n = 1
    while n < rec.size + burst.size:
        n <<= 1
    cross = np.fft.rfft(rec, n=n) * np.conj(np.fft.rfft(burst, n=n))
    cross /= np.maximum(np.abs(cross), 1e-12)
    return np.fft.irfft(cross, n=n), n


def phat_window(corr, n, min_lag, max_lag):
    """:190-198 -> (lags in the reference's order, |corr| there)"""
    wrapped = np.arange(n)
    wrapped[wrapped > n // 2] -= n
    valid = (wrapped >= min_lag) & (wrapped <= max_lag)
    return wrapped[valid], np.abs(corr[valid])


def _failed(message, route_kind="output_to_input"):
    return dict(success=False, measured_round_trip_ms=0.0, estimated_one_way_ms=0.0, applied_compensation_ms=0.0, confidence=0.0,
                peak_sample_offset=0, message=message, repetition_count=0, agreement_ms=0.0, ambiguity_score=0.0,
                sub_sample_offset=0.0, route_latency_ms=0.0, directional_latency_ms=None, route_kind=route_kind,
                compensation_basis="measured_output_to_input_route")


def analyze_latency(reference_probe, recorded_signal, sample_rate=48_000, min_search_ms=5.0, max_search_ms=500.0,
                    expected_playback_start_ms=None, expected_playback_jitter_ms=None, expected_latency_min_ms=None,
                    expected_latency_max_ms=None, route_kind="output_to_input", trace=None):
    """:232-515 as a dict of FIELDS; `trace`, a dict, receives the intermediates"""
    trace = {} if trace is None else trace
    route_kind = str(route_kind or "output_to_input").strip().lower()
    if route_kind != "output_to_input":
        return _failed("Unsupported latency route; expected output_to_input.", route_kind)
    if reference_probe is None or recorded_signal is None:
        return _failed("Missing probe or recording.")
    if not np.all(np.isfinite(np.asarray(recorded_signal, dtype=np.float64))):
        return _failed(NON_FINITE_MESSAGE)
    ref, rec = normalize_audio(reference_probe), normalize_audio(recorded_signal)
    if ref.size < 16 or rec.size < ref.size:
        return _failed("Recording too short for reliable correlation.")
    min_lag = int((min_search_ms / 1000.0) * sample_rate)
    max_lag = int((max_search_ms / 1000.0) * sample_rate)
    expected = expected_playback_start_ms is not None
    expected_min = expected_latency_min_ms if expected_latency_min_ms is not None else min_search_ms
    expected_max = expected_latency_max_ms if expected_latency_max_ms is not None else max_search_ms
    playback_min_ms = playback_max_ms = 0.0
    if expected:
        jitter = max(0.0, expected_playback_jitter_ms or 0.0)
        playback_min_ms = max(0.0, expected_playback_start_ms - jitter)
        playback_max_ms = max(playback_min_ms, expected_playback_start_ms + jitter)
        min_lag = int(((playback_min_ms + expected_min) / 1000.0) * sample_rate)
        max_lag = int(((playback_max_ms + expected_max) / 1000.0) * sample_rate)
    if max_lag <= min_lag:
        return _failed("Search window is outside valid lag range.")
    burst, offsets = coded_probe_components(sample_rate, ref.size)
    if burst.size < 16 or not offsets:
        burst, offsets = ref, [0]
    full_lags, full_scores, full_energy = correlation_scores(rec, ref, min_lag, max_lag)
    trace.update(full_lags=full_lags, full_scores=full_scores, full_energy=full_energy, bursts=[], offsets=list(offsets), margins=[])
    if full_lags.size == 0:
        return _failed("Search window does not overlap captured audio.")
    full = pick_peak(full_lags, full_scores, 0.985)
    trace["full_pick"] = full
    coarse = full["peak_lag"]
    radius = max(int(round(sample_rate * 0.010)), burst.size)
    estimates, peaks, margins, ambiguities, phat_matches = [], [full["peak_score"]], [full["margin"]], [full["ambiguity"]], []
    corr = None
    for offset in offsets:
        expected_lag = coarse + float(offset)
        lag_min = max(min_lag + int(offset), int(round(expected_lag - radius)))
        lag_max = min(max_lag + int(offset), int(round(expected_lag + radius)))
        lags, scores, energy = correlation_scores(rec, burst, lag_min, lag_max)
        entry = dict(offset=int(offset), lag_min=lag_min, lag_max=lag_max, lags=lags, scores=scores, energy=energy, used=False,
                     rounding=(expected_lag - radius, expected_lag + radius))
        trace["bursts"].append(entry)
        if lags.size == 0:
            continue
        pick = pick_peak(lags, scores, 0.94)
        entry["pick"] = pick
        if pick["peak_score"] < 0.035:
            continue
        entry["used"] = True
        start = pick["peak_lag"] - float(offset)
        estimates.append(start)
        peaks.append(pick["peak_score"])
        margins.append(pick["margin"])
        ambiguities.append(pick["ambiguity"])
        if corr is None:
            corr, n = phat_correlation(rec, burst)
        phat_lags, phat_abs = phat_window(corr, n, lag_min, lag_max)
        entry.update(phat_lags=phat_lags, phat_abs=phat_abs)
        if phat_lags.size:
            hint = int(phat_lags[int(np.argmax(phat_abs))])
            entry["phat_hint"] = hint
            phat_matches.append(max(0.0, 1.0 - abs(float(hint - int(offset)) - start) / max(1.0, sample_rate * 0.006)))
    fallback = not estimates
    if fallback:
        estimates, peaks, margins, ambiguities = [full["peak_lag"]], [full["peak_score"]], [full["margin"]], [full["ambiguity"]]
    trace["fallback"] = fallback
    est = np.asarray(estimates, dtype=np.float64)
    median_start = float(np.median(est))
    deviations = np.abs(est - median_start)
    agreement_ms = (float(np.percentile(deviations, 75)) * 1000.0) / float(sample_rate)
    measured = (median_start * 1000.0) / float(sample_rate)
    if expected:
        measured = max(0.0, measured - expected_playback_start_ms)
    peak_value, margin_ratio = float(np.median(peaks)), float(np.median(margins))
    ambiguity_score = float(np.median(ambiguities))
    phat_score = float(np.median(phat_matches)) if phat_matches else 0.5
    strength = float(np.clip((peak_value - 0.06) / 0.24, 0.0, 1.0))
    agreement_score = float(np.clip(1.0 - agreement_ms / 4.0, 0.0, 1.0))
    repetition = float(np.clip(len(estimates) / min(3, max(1, len(offsets))), 0.0, 1.0))
    margin_score = float(np.clip(margin_ratio / 0.28, 0.0, 1.0))
    ambiguity_confidence = float(np.clip(1.0 - ambiguity_score, 0.0, 1.0))
    alignment = 0.0
    if expected:
        centre_ms = 0.5 * (playback_min_ms + playback_max_ms + expected_min + expected_max)
        centre = int((centre_ms / 1000.0) * sample_rate)
        alignment = max(0.0, 1.0 - (abs(median_start - centre) / float(max(1, (max_lag - min_lag) // 2))))
    confidence = (0.24 * strength + 0.24 * agreement_score + 0.18 * repetition + 0.14 * margin_score + 0.12 * ambiguity_confidence
                  + 0.08 * phat_score)
    if expected:
        confidence = 0.88 * confidence + 0.12 * alignment
    success = (confidence >= 0.32 and measured > 0.0 and peak_value >= 0.07 and ambiguity_score < 0.90
               and len(estimates) >= min(2, len(offsets)) and agreement_ms <= 6.0)
    if success:
        message = "ok"
    elif agreement_ms > 6.0 and len(estimates) > 1:
        message = "Repeated probes disagree; echoes or bleed make latency ambiguous."
    elif ambiguity_score > 0.82:
        message = "Echo ambiguity: competing correlation peaks are too close."
    else:
        message = "Low confidence or ambiguous coded-probe correlation."
    trace["rules"] = dict(confidence=(confidence, 0.32), peak_value=(peak_value, 0.07), ambiguity_090=(ambiguity_score, 0.90),
                          ambiguity_082=(ambiguity_score, 0.82), agreement_ms=(agreement_ms, 6.0))
    return dict(success=bool(success), measured_round_trip_ms=measured, estimated_one_way_ms=0.0, applied_compensation_ms=measured,
                confidence=confidence, peak_sample_offset=int(round(median_start)), message=message,
                repetition_count=len(estimates), agreement_ms=agreement_ms, ambiguity_score=ambiguity_score,
                sub_sample_offset=median_start, route_latency_ms=measured, directional_latency_ms=None, route_kind=route_kind,
                compensation_basis="measured_output_to_input_route")
