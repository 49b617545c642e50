"""Latency calibration: python/mic_eq/analysis/latency_calibration.py of the reference, batched over recordings.

A repeated Barker-13 coded probe is played on the selected output and recorded on the selected input; ``analyze_latency``
estimates the route delay, with a confidence and a reason, from the normalised cross-correlation of the whole probe, a local
search per burst and a GCC-PHAT cross-check.  Here one ``LatencyCalibration`` holds one probe at one sample rate and analyses
many recordings per call on the device (csrc/af_latency.hip); the rules of analyze_latency:424-515 run on the host from the
small record each stream leaves (csrc/af_latency_math.h).  The probe itself is a table computed on the host, bit for bit the
reference's.

One addition over the reference: a recording with a sample that is not finite is not analysed and comes back as a failed
result with ``NON_FINITE_MESSAGE``; the reference has no such check and would return NaNs.  Recordings are float32.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from datetime import datetime, timezone

import numpy as np

from . import _lib

BARKER_13 = np.array([1.0, 1.0, 1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0], dtype=np.float64)  # :17-20
DEFAULT_REPETITIONS = 4
NON_FINITE_MESSAGE = "Recording contains non-finite samples."
MAX_TRANSFORM = 1 << 18  # AF_LATENCY_MAX_TRANSFORM
PASSES = ("condition", "probe", "bursts", "phat")  # AF_LATENCY_PASS_*


@dataclass
class LatencyCalibrationResult:
    """Result of latency calibration analysis (:24-42)."""

    success: bool
    measured_round_trip_ms: float
    estimated_one_way_ms: float
    applied_compensation_ms: float
    confidence: float
    peak_sample_offset: int
    message: str = ""
    repetition_count: int = 0
    agreement_ms: float = 0.0
    ambiguity_score: float = 0.0
    sub_sample_offset: float = 0.0
    route_latency_ms: float = 0.0
    directional_latency_ms: float | None = None
    route_kind: str = "output_to_input"
    compensation_basis: str = "measured_output_to_input_route"


def _coded_probe_components(sample_rate, total_samples, repetitions=DEFAULT_REPETITIONS):
    """:74-115: a single coded burst and its start offsets inside the full probe."""
    repetitions = max(1, int(repetitions))
    chip_samples = max(4, int(round(sample_rate * 0.0005)))
    min_spacing = max(chip_samples, int(round(sample_rate * 0.006)))
    while chip_samples > 4:
        burst_len = BARKER_13.size * chip_samples
        if repetitions * burst_len + (repetitions - 1) * min_spacing <= total_samples:
            break
        chip_samples -= 1
    code = np.repeat(BARKER_13, chip_samples)
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


def generate_probe_signal(sample_rate: int = 48_000, duration_ms: float = 80.0, start_freq_hz: float = 1_500.0,
                          end_freq_hz: float = 9_000.0, amplitude: float = 0.8) -> np.ndarray:
    """:45-71.  ``start_freq_hz`` and ``end_freq_hz`` are kept for the reference's signature; the probe is coded bursts."""
    del start_freq_hz, end_freq_hz
    total_samples = max(1, int(sample_rate * (duration_ms / 1000.0)))
    burst, offsets = _coded_probe_components(sample_rate, total_samples)
    probe = np.zeros(total_samples, dtype=np.float64)
    for offset in offsets:
        end = min(total_samples, offset + burst.size)
        if end > offset:
            probe[offset:end] += burst[: end - offset]
    peak = np.max(np.abs(probe))
    if peak > 0.0:
        probe = (probe / peak) * float(amplitude)
    return probe.astype(np.float32)


class _Search(C.Structure):  # af_latency_search
    _fields_ = ([(name, C.c_double) for name in ("min_search_ms", "max_search_ms", "expected_playback_start_ms",
                                                 "expected_playback_jitter_ms", "expected_latency_min_ms", "expected_latency_max_ms")]
                + [(name, C.c_int32) for name in ("has_playback_start", "has_playback_jitter", "has_latency_min", "has_latency_max",
                                                  "route_supported", "reserved")])


class _Result(C.Structure):  # af_latency_result
    _fields_ = ([(name, C.c_int32) for name in ("success", "exit_code", "message", "repetition_count")]
                + [("peak_sample_offset", C.c_int64)]
                + [(name, C.c_double) for name in ("measured_round_trip_ms", "applied_compensation_ms", "confidence", "agreement_ms",
                                                   "ambiguity_score", "sub_sample_offset", "route_latency_ms")])


_EXIT_ROUTE = 1  # AF_LATENCY_EXIT_ROUTE


def _failed(message: str, route_kind: str = "output_to_input") -> LatencyCalibrationResult:
    return LatencyCalibrationResult(success=False, measured_round_trip_ms=0.0, estimated_one_way_ms=0.0, applied_compensation_ms=0.0,
                                    confidence=0.0, peak_sample_offset=0, route_kind=route_kind, message=message)


def _per_stream(value, n_streams: int, name: str) -> list:
    """A scalar (None and text included) for every stream, or one value per stream."""
    if value is None or isinstance(value, (str, bytes)) or np.isscalar(value):
        return [value] * n_streams
    values = list(value)
    if len(values) != n_streams:
        raise ValueError(f"{name}: expected a scalar or one value per stream ({n_streams}), got {len(values)}")
    return values


class LatencyCalibration:
    """analyze_latency for up to ``max_streams`` recordings of up to ``max_record_samples`` samples of one probe (af_latency_*)."""

    def __init__(self, sample_rate, reference_probe, max_streams: int, max_record_samples: int, device: int = 0):
        self._lib = _lib.load()
        probe = np.ascontiguousarray(np.asarray(reference_probe, dtype=np.float64).flatten())
        handle = C.c_void_p()
        _lib.check(self._lib.af_latency_create(float(sample_rate), probe.ctypes.data_as(C.POINTER(C.c_double)), int(probe.size),
                                               int(max_streams), int(max_record_samples), int(device), C.byref(handle)))
        self._h = handle
        self.sample_rate = sample_rate
        self.max_streams, self.max_record_samples = int(max_streams), int(max_record_samples)
        count, offsets, burst, radius = C.c_int32(0), (C.c_int32 * 4)(), C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.af_latency_layout(self._h, C.byref(count), offsets, C.byref(burst), C.byref(radius)))
        self.offsets, self.burst_samples, self.local_radius = [int(o) for o in offsets[: count.value]], burst.value, radius.value
        self.n_streams = 0
        self._route_kinds: list[str] = []

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_latency_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _searches(self, n_streams, min_search_ms, max_search_ms, expected_playback_start_ms, expected_playback_jitter_ms,
                  expected_latency_min_ms, expected_latency_max_ms, route_kind):
        columns = [_per_stream(v, n_streams, name) for name, v in (
            ("min_search_ms", min_search_ms), ("max_search_ms", max_search_ms), ("expected_playback_start_ms", expected_playback_start_ms),
            ("expected_playback_jitter_ms", expected_playback_jitter_ms), ("expected_latency_min_ms", expected_latency_min_ms),
            ("expected_latency_max_ms", expected_latency_max_ms))]
        kinds = [str(kind or "output_to_input").strip().lower() for kind in _per_stream(route_kind, n_streams, "route_kind")]  # :253
        searches = (_Search * n_streams)()
        for s in range(n_streams):
            lo, hi, start, jitter, lat_min, lat_max = (column[s] for column in columns)
            if lo is None or hi is None:
                raise ValueError("min_search_ms and max_search_ms must be numbers")
            q = searches[s]
            q.min_search_ms, q.max_search_ms = float(lo), float(hi)
            for name, flag, value in (("expected_playback_start_ms", "has_playback_start", start),
                                      ("expected_playback_jitter_ms", "has_playback_jitter", jitter),
                                      ("expected_latency_min_ms", "has_latency_min", lat_min),
                                      ("expected_latency_max_ms", "has_latency_max", lat_max)):
                setattr(q, flag, int(value is not None))
                setattr(q, name, float(value) if value is not None else 0.0)
            q.route_supported = int(kinds[s] == "output_to_input")
        return searches, kinds

    @staticmethod
    def _lengths(lengths, n_streams):
        if lengths is None:
            return None, None
        values = np.ascontiguousarray(lengths, dtype=np.int64).reshape(-1)
        if values.size != n_streams:
            raise ValueError(f"lengths: expected one per stream ({n_streams}), got {values.size}")
        return values, values.ctypes.data_as(C.POINTER(C.c_int64))

    def analyze(self, recorded, lengths=None, min_search_ms=5.0, max_search_ms=500.0, expected_playback_start_ms=None,
                expected_playback_jitter_ms=None, expected_latency_min_ms=None, expected_latency_max_ms=None,
                route_kind="output_to_input") -> list[LatencyCalibrationResult]:
        """``recorded`` [streams, n] float32 on the host, stream s holding ``lengths[s]`` samples (default n)."""
        recorded = np.ascontiguousarray(recorded, dtype=np.float32)
        if recorded.ndim != 2:
            raise TypeError("recorded must be [n_streams, n_samples]")
        n_streams, n = recorded.shape
        searches, kinds = self._searches(n_streams, min_search_ms, max_search_ms, expected_playback_start_ms,
                                         expected_playback_jitter_ms, expected_latency_min_ms, expected_latency_max_ms, route_kind)
        keep, pointer = self._lengths(lengths, n_streams)
        _lib.check(self._lib.af_latency_analyze_host(self._h, recorded.ctypes.data_as(C.POINTER(C.c_float)), int(n), int(n), int(n_streams),
                                                     pointer, searches))
        del keep
        return self._results(n_streams, kinds)

    def analyze_device(self, device_pointer: int, stride: int, n_streams: int, lengths, n_samples=None, min_search_ms=5.0,
                       max_search_ms=500.0, expected_playback_start_ms=None, expected_playback_jitter_ms=None,
                       expected_latency_min_ms=None, expected_latency_max_ms=None, route_kind="output_to_input"):
        """As ``analyze`` for [n_streams][stride] float32 already on the device; ``n_samples`` defaults to the longest length."""
        n_streams = int(n_streams)
        keep, pointer = self._lengths(lengths, n_streams)
        if n_samples is None:
            n_samples = int(keep.max()) if keep is not None and keep.size else int(stride)
        searches, kinds = self._searches(n_streams, min_search_ms, max_search_ms, expected_playback_start_ms,
                                         expected_playback_jitter_ms, expected_latency_min_ms, expected_latency_max_ms, route_kind)
        _lib.check(self._lib.af_latency_analyze_device(self._h, C.c_void_p(device_pointer), int(n_samples), int(stride), n_streams, pointer,
                                                       searches))
        del keep
        return self._results(n_streams, kinds)

    def _results(self, n_streams, kinds):
        rows = (_Result * n_streams)()
        _lib.check(self._lib.af_latency_read_results(self._h, rows, n_streams))
        self.n_streams = n_streams
        out = []
        for row, kind in zip(rows, kinds):
            text = self._lib.af_latency_message_text(row.exit_code, row.message).decode()
            if row.exit_code:
                out.append(_failed(text, kind if row.exit_code == _EXIT_ROUTE else "output_to_input"))
                continue
            out.append(LatencyCalibrationResult(
                success=bool(row.success), measured_round_trip_ms=row.measured_round_trip_ms, estimated_one_way_ms=0.0,
                applied_compensation_ms=row.applied_compensation_ms, confidence=row.confidence,
                peak_sample_offset=int(row.peak_sample_offset), message=text, repetition_count=int(row.repetition_count),
                agreement_ms=row.agreement_ms, ambiguity_score=row.ambiguity_score, sub_sample_offset=row.sub_sample_offset,
                route_latency_ms=row.route_latency_ms, directional_latency_ms=None, route_kind=kind,
                compensation_basis="measured_output_to_input_route"))
        return out

    def scores(self, stream: int) -> dict:
        """Diagnostics of one stream of the last analysis: ``full`` and ``bursts[k]`` hold ``lags``, ``scores`` and
        ``window_energy``; a burst also ``phat_lags`` and ``phat`` (the PHAT correlation inside its window, in lag order)."""
        capacity = max(self.max_record_samples, 2 * self.local_radius + 2)
        values, energy, phat = (np.empty(capacity, dtype=np.float64) for _ in range(3))
        as_dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        parts = []
        for which in range(1 + len(self.offsets)):
            lo, count, phat_lo, phat_count = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int32(0)
            _lib.check(self._lib.af_latency_read_scores(self._h, int(stream), which, C.byref(lo), C.byref(count), as_dp(values), as_dp(energy),
                                                        C.byref(phat_lo), C.byref(phat_count), as_dp(phat), capacity))
            part = {"lags": np.arange(lo.value, lo.value + count.value, dtype=np.int64), "scores": values[: count.value].copy(),
                    "window_energy": energy[: count.value].copy()}
            if which:
                part["offset"] = self.offsets[which - 1]
                part["phat_lags"] = np.arange(phat_lo.value, phat_lo.value + phat_count.value, dtype=np.int64)
                part["phat"] = phat[: phat_count.value].copy()
            parts.append(part)
        return {"full": parts[0], "bursts": parts[1:]}

    def last_kernel_ms(self, passes: bool = False):
        """The device time of the last analysis; with ``passes`` a dict of its parts as well."""
        ms, parts = C.c_double(0.0), (C.c_double * len(PASSES))()
        _lib.check(self._lib.af_latency_last_kernel_ms(self._h, C.byref(ms), parts))
        return (ms.value, dict(zip(PASSES, parts))) if passes else ms.value

    def debug_rfft(self, x) -> np.ndarray:
        """Test hook: the PHAT pass's forward real transform of float32 ``x`` (a power of two long) alone."""
        x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
        out = np.empty((x.size // 2 + 1, 2), dtype=np.float64)
        _lib.check(self._lib.af_latency_debug_rfft(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), int(x.size),
                                                   out.ctypes.data_as(C.POINTER(C.c_double))))
        return out[:, 0] + 1j * out[:, 1]


def analyze_latency_batch(reference_probe, recorded, sample_rate, lengths=None, min_search_ms=5.0, max_search_ms=500.0,
                          expected_playback_start_ms=None, expected_playback_jitter_ms=None, expected_latency_min_ms=None,
                          expected_latency_max_ms=None, route_kind="output_to_input", device: int = 0) -> list[LatencyCalibrationResult]:
    """analyze_latency (:232-515) for ``recorded`` [streams, n] float32 against one probe: one result per stream.  The search
    keywords and ``route_kind`` take a scalar or one value per stream; an early exit of the reference comes back as that stream's
    failed result and does not stop the batch."""
    recorded = np.ascontiguousarray(recorded, dtype=np.float32)
    if recorded.ndim != 2:
        raise TypeError("recorded must be [n_streams, n_samples]")
    calibration = LatencyCalibration(sample_rate, reference_probe, recorded.shape[0], max(1, recorded.shape[1]), device)
    try:
        return calibration.analyze(recorded, lengths, min_search_ms, max_search_ms, expected_playback_start_ms, expected_playback_jitter_ms,
                                   expected_latency_min_ms, expected_latency_max_ms, route_kind)
    finally:
        calibration.close()


def analyze_latency(reference_probe, recorded_signal, sample_rate: int = 48_000, min_search_ms: float = 5.0, max_search_ms: float = 500.0,
                    expected_playback_start_ms: float | None = None, expected_playback_jitter_ms: float | None = None,
                    expected_latency_min_ms: float | None = None, expected_latency_max_ms: float | None = None,
                    route_kind: str = "output_to_input") -> LatencyCalibrationResult:
    """The reference's analyze_latency: a batch of one."""
    kind = str(route_kind or "output_to_input").strip().lower()
    if kind != "output_to_input":
        return _failed("Unsupported latency route; expected output_to_input.", kind)
    if reference_probe is None or recorded_signal is None:
        return _failed("Missing probe or recording.")
    probe = np.asarray(reference_probe, dtype=np.float64).flatten()
    recorded = np.asarray(recorded_signal, dtype=np.float32).flatten()
    if probe.size < 16 or recorded.size < probe.size:
        return _failed("Recording too short for reliable correlation.")
    return analyze_latency_batch(probe, recorded[None, :], sample_rate, None, min_search_ms, max_search_ms, expected_playback_start_ms,
                                 expected_playback_jitter_ms, expected_latency_min_ms, expected_latency_max_ms, kind)[0]


def result_to_profile(result: LatencyCalibrationResult, sample_rate: int = 48_000, *, engine_latency_ms: float = 0.0,
                      engine_config_signature: str = "") -> dict:
    """:518-555: the persisted profile dictionary."""
    route_latency_ms = float(result.route_latency_ms)
    if route_latency_ms <= 0.0:
        route_latency_ms = max(0.0, float(result.measured_round_trip_ms), float(result.applied_compensation_ms))
    engine_latency_ms = max(0.0, float(engine_latency_ms))
    return {
        "measured_round_trip_ms": float(result.measured_round_trip_ms),
        "estimated_one_way_ms": float(result.estimated_one_way_ms),
        "applied_compensation_ms": float(result.applied_compensation_ms),
        "route_latency_ms": route_latency_ms,
        "directional_latency_ms": float(result.directional_latency_ms) if result.directional_latency_ms is not None else None,
        "route_kind": str(result.route_kind),
        "compensation_basis": str(result.compensation_basis),
        "confidence": float(result.confidence),
        "agreement_ms": float(result.agreement_ms),
        "ambiguity_score": float(result.ambiguity_score),
        "repetition_count": int(result.repetition_count),
        "sample_rate": int(sample_rate),
        "engine_latency_ms": engine_latency_ms,
        "total_latency_ms": route_latency_ms + engine_latency_ms,
        "engine_config_signature": str(engine_config_signature),
        "timestamp_utc": datetime.now(timezone.utc).isoformat(),
    }
