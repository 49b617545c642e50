"""EQ headroom validation: the gain-scale sweep of python/mic_eq/analysis/auto_eq_parts/headroom.py, batched over captures.

The reference's apply_headroom_validation (headroom.py:292-354) renders a capture through the chain with the candidate EQ and,
while the render is not headroom-safe, again with the band gains scaled by 0.85 ... 0.0.  Here every (capture, scale) pair is a
LANE: ``LaneEq`` (csrc/af_lane_eq.hip) runs the ten-band EQ with per-lane coefficients over one front-end run per capture (the
de-esser as given; EQ, compressor and limiter off), and ``cs_sweep_kernel`` / ``cs_fold_kernel`` (compressor_search.py) take the
lanes' EQ output on the device through compressor -> limiter -> true-peak limiter into the reference's result dict.  The
selection runs on the host.  Settings the sweep cannot express go through simulate_auto_eq_chain_batch, one call per scale.
"""
from __future__ import annotations

import ctypes as C
import time
from copy import deepcopy
from typing import Any, Mapping

import numpy as np

from . import _lib
from . import mic_eq_core as core
from .compressor_search import _DEESSER_DEFAULTS, MAX_BLOCKS, CompressorSearch, _per_stream, simulation_dict
from .setup_verification import _COMPRESSOR_KEYS, _render

HEADROOM_TARGET_DB = 1.0                      # headroom.py:14
LIMITER_GAIN_REDUCTION_WARN_DB = 1.0          # :15
TRUE_PEAK_GAIN_REDUCTION_WARN_DB = 0.5        # :16
HEADROOM_SCALES = (1.0, 0.85, 0.70, 0.55, 0.40, 0.25, 0.0)  # :17
_LIMITER_KEYS = (("enabled", True), ("ceiling_db", -0.5), ("release_ms", 50.0), ("careful_output_enabled", True))  # :77-83
_LOOKAHEAD_MS = 2.0                           # the flat settings carry none: simulate_auto_eq_chain's default (python_api.rs:472-487)
DEFAULT_LANE_EQ_BYTES = 4 << 30               # a chunk's lane-EQ output: about 300 captures of 10 s at seven scales


class LaneEq:
    """The ten-band EQ with per-lane bands over shared captures (af_lane_eq_*).  A lane is one (capture, band set) pair."""

    def __init__(self, sample_rate: float = 48_000.0, device: int = 0):
        self._lib = _lib.load()
        handle = C.c_void_p()
        _lib.check(self._lib.af_lane_eq_create(float(sample_rate), int(device), C.byref(handle)))
        self._h = handle
        self.sample_rate = float(sample_rate)
        self.n_lanes = self.n_samples = 0

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_lane_eq_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _lanes(lane_capture, bands):
        lanes = np.ascontiguousarray(lane_capture, dtype=np.int32).reshape(-1)
        values = np.ascontiguousarray(bands, dtype=np.float64)
        if values.shape != (lanes.size, core.NUM_BANDS, 3):
            raise ValueError(f"expected bands [{lanes.size}, {core.NUM_BANDS}, 3] (frequency_hz, gain_db, q), got {values.shape}")
        return lanes, values

    def run(self, audio: np.ndarray, lane_capture, bands) -> None:
        """``audio`` [captures, n] float32 on the host; ``lane_capture`` [lanes]; ``bands`` [lanes, 10, 3]."""
        audio = np.ascontiguousarray(audio, dtype=np.float32)
        if audio.ndim != 2:
            raise TypeError("audio must be [n_captures, n_samples]")
        lanes, values = self._lanes(lane_capture, bands)
        _lib.check(self._lib.af_lane_eq_run_host(self._h, audio.ctypes.data_as(C.POINTER(C.c_float)), int(audio.shape[1]), int(audio.shape[0]),
                                                 int(audio.shape[1]), lanes.ctypes.data_as(C.POINTER(C.c_int32)), int(lanes.size),
                                                 values.ctypes.data_as(C.POINTER(C.c_double))))
        self.n_lanes, self.n_samples = int(lanes.size), int(audio.shape[1])

    def run_device(self, pointer: int, n_samples: int, n_captures: int, stride: int, lane_capture, bands) -> None:
        """As ``run`` for [n_captures][stride] float32 already on the device."""
        lanes, values = self._lanes(lane_capture, bands)
        _lib.check(self._lib.af_lane_eq_run_device(self._h, C.c_void_p(pointer), int(n_samples), int(n_captures), int(stride),
                                                   lanes.ctypes.data_as(C.POINTER(C.c_int32)), int(lanes.size),
                                                   values.ctypes.data_as(C.POINTER(C.c_double))))
        self.n_lanes, self.n_samples = int(lanes.size), int(n_samples)

    def device_output(self) -> tuple[int, int]:
        """(device pointer, stride in samples) of the last run's [lanes][stride] float32 output; valid until the next run."""
        pointer, stride = C.c_void_p(), C.c_int64(0)
        _lib.check(self._lib.af_lane_eq_output(self._h, C.byref(pointer), C.byref(stride)))
        return int(pointer.value), int(stride.value)

    def output(self) -> np.ndarray:
        """[lanes, n] float32 output of the last run."""
        out = np.empty((self.n_lanes, self.n_samples), dtype=np.float32)
        _lib.check(self._lib.af_lane_eq_read_output(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), int(self.n_samples)))
        return out

    def last_kernel_ms(self) -> float:
        ms = C.c_double(0.0)
        _lib.check(self._lib.af_lane_eq_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value


# ------------------------------------------------------------------------------------------- the reference's settings
def _as_float(value: Any, default: float) -> float:
    """headroom.py:28-33."""
    try:
        parsed = float(value)
    except (TypeError, ValueError):
        return default
    return parsed if np.isfinite(parsed) else default


def _as_bool(value: Any, default: bool) -> bool:
    """headroom.py:36-39."""
    return value if isinstance(value, bool) else default


def _flatten_chain_settings(chain_settings: Mapping[str, Any] | None) -> dict[str, Any]:
    """headroom.py:42-84: the nested ``deesser`` / ``compressor`` / ``limiter`` dicts as simulate_auto_eq_chain's flat keys."""
    chain_settings = chain_settings or {}
    flat: dict[str, Any] = {"return_output_audio": _as_bool(chain_settings.get("return_output_audio"), False)}
    for prefix, keys in (("deesser", _DEESSER_DEFAULTS), ("compressor", _COMPRESSOR_KEYS), ("limiter", _LIMITER_KEYS)):
        source = chain_settings.get(prefix) or {}
        for key, default in keys:
            convert = _as_bool if isinstance(default, bool) else _as_float
            flat[f"{prefix}_{key}"] = convert(source.get(key), default)
    return flat


def _bands_from_settings(eq_settings: Mapping[str, Any]) -> list:
    """headroom.py:87-96."""
    freqs, gains, qs = (list(eq_settings.get(key) or []) for key in ("band_freqs", "band_gains", "band_qs"))
    if not (len(freqs) == len(gains) == len(qs) == core.NUM_BANDS):
        raise ValueError("Auto-EQ settings must contain 10 frequencies, gains, and Q values")
    return [(_as_float(f, 1000.0), _as_float(g, 0.0), _as_float(q, 1.41)) for f, g, q in zip(freqs, gains, qs)]


def _scaled_bands(bands: list, scale: float) -> list:
    """The bands of headroom.py:312-315's candidate: ``(original_gains * scale)`` in f64, read back through _as_float."""
    return [(f, _as_float(np.float64(g) * np.float64(scale), 0.0), q) for f, g, q in bands]


def _is_headroom_safe(simulation: Mapping[str, Any]) -> bool:
    """headroom.py:278-289, in f64 on the record's values."""
    headroom = _as_float(simulation.get("pre_limiter_true_peak_headroom_db"), simulation.get("true_peak_headroom_db", 120.0))
    limiter_gr = _as_float(simulation.get("limiter_gain_reduction_db"), 0.0)
    true_peak_gr = _as_float(simulation.get("true_peak_limiter_gain_reduction_db"), 0.0)
    return bool(headroom >= HEADROOM_TARGET_DB and limiter_gr <= LIMITER_GAIN_REDUCTION_WARN_DB
                and true_peak_gr <= TRUE_PEAK_GAIN_REDUCTION_WARN_DB)


def _sweep_expresses(flat: Mapping[str, Any], n_samples: int, sample_rate: float) -> bool:
    """The sweep kernels run compressor and limiter with auto-makeup off, and the fold holds MAX_BLOCKS control blocks."""
    block = int(min(max(round(sample_rate * 0.020), 1), 8192))
    return bool(flat["compressor_enabled"] and flat["limiter_enabled"] and not flat["compressor_auto_makeup_enabled"]
                and 0 < n_samples and -(-n_samples // block) <= MAX_BLOCKS)


def _engine_settings(flat: Mapping[str, Any]) -> dict:
    return {key: value for key, value in flat.items() if key != "return_output_audio"}


# ------------------------------------------------------------------------------------------- the two routes
def _front_end(audio: np.ndarray, sample_rate: float, flats: list, device: int) -> tuple[np.ndarray, np.ndarray]:
    """What every stream's EQ sees and the rows of that run: compressor_input_batch's engine call with the EQ off as well, one
    call per distinct de-esser configuration.  Returns ([streams, n] float32, [blocks, streams] rows)."""
    n_streams, n = audio.shape
    groups: dict = {}
    for s, flat in enumerate(flats):
        front = {key: flat[key] for key in flat if key.startswith("deesser_")}
        if not front["deesser_enabled"]:
            front = {"deesser_enabled": False}
        front.update(compressor_enabled=False, limiter_enabled=False)
        groups.setdefault(repr(sorted(front.items())), (front, []))[1].append(s)
    block = int(min(max(round(sample_rate * 0.020), 1), 8192))
    out = np.empty_like(audio)
    rows = np.zeros((-(-n // block), n_streams), dtype=core.STATS_DTYPE)
    flat_bands = [(1000.0, 0.0, 1.41)] * core.NUM_BANDS
    for front, members in groups.values():
        engine = core.Engine(sample_rate, len(members), device)
        try:
            core.configure_auto_eq_chain(engine, float(sample_rate), flat_bands, front)
            engine.set_eq_enabled(0)
            out[members] = engine.process(np.ascontiguousarray(audio[members]))
            rows[:, members] = engine.block_stats()
        finally:
            engine.close()
    return out, rows


def _sweep_route(audio: np.ndarray, sample_rate: float, bands: list, flats: list, scales: tuple, device: int, max_bytes: int,
                 want_rows: bool, timing: dict) -> tuple[list, np.ndarray | None]:
    """Every (stream, scale) as a lane.  Returns (records [streams][scales], rows [blocks, streams, scales] or None)."""
    n_streams, n = audio.shape
    n_scales = len(scales)
    block = int(min(max(round(sample_rate * 0.020), 1), 8192))
    records: list = [None] * n_streams
    rows_out = np.zeros((-(-n // block), n_streams, n_scales), dtype=core.STATS_DTYPE) if want_rows else None
    limiters: dict = {}
    for s, flat in enumerate(flats):
        key = (flat["limiter_ceiling_db"], flat["limiter_release_ms"], _LOOKAHEAD_MS, flat["limiter_careful_output_enabled"])
        limiters.setdefault(key, []).append(s)
    per_capture = n_scales * (-(-n // 64) * 64) * 4
    chunk = max(1, int(max_bytes) // per_capture)
    lane_eq, search = LaneEq(sample_rate, device), CompressorSearch(sample_rate, device)
    try:
        for limiter, group in limiters.items():
            search.set_limiter(*limiter)
            for start in range(0, len(group), chunk):
                members = group[start:start + chunk]
                t0 = time.perf_counter()
                front, front_rows = _front_end(np.ascontiguousarray(audio[members]), sample_rate, [flats[s] for s in members], device)
                timing["front_end_wall_ms"] = timing.get("front_end_wall_ms", 0.0) + (time.perf_counter() - t0) * 1000.0
                lane_capture = np.repeat(np.arange(len(members), dtype=np.int32), n_scales)
                lane_bands = np.asarray([_scaled_bands(bands[s], scale) for s in members for scale in scales], dtype=np.float64)
                lane_eq.run(front, lane_capture, lane_bands)
                pointer, stride = lane_eq.device_output()
                search.load_device(pointer, n, lane_capture.size, stride, front_rows[:, lane_capture])
                candidates, bases = [], []
                for lane, c in enumerate(lane_capture):
                    flat = flats[members[c]]
                    candidates.append((lane, flat["compressor_threshold_db"], flat["compressor_ratio"], flat["compressor_attack_ms"],
                                       flat["compressor_release_ms"]))
                    bases.append((flat["compressor_makeup_gain_db"], flat["compressor_base_release_ms"], flat["compressor_adaptive_release"],
                                  flat["compressor_sidechain_highpass_enabled"]))
                lanes = search.sweep(candidates, bases)
                if want_rows:
                    rows_out[:, members, :] = search.rows().reshape(-1, len(members), n_scales)
                kernel = search.last_kernel_ms()
                for key, ms in (("lane_eq_kernel_ms", lane_eq.last_kernel_ms()), ("sweep_kernel_ms", kernel["sweep"]),
                                ("fold_kernel_ms", kernel["fold"])):
                    timing[key] = timing.get(key, 0.0) + ms
                for c, s in enumerate(members):
                    records[s] = [lanes[c * n_scales + k] for k in range(n_scales)]
    finally:
        search.close()  # before the lane EQ: it reads the lane EQ's output buffer
        lane_eq.close()
    return records, rows_out


def simulate_candidate_chain_batch(audio, fs: float, eq_settings, chain_settings=None, scales=(1.0,), route: str = "auto", device: int = 0,
                                   max_lane_eq_bytes: int = DEFAULT_LANE_EQ_BYTES, return_rows: bool = False, timing: dict | None = None):
    """simulate_candidate_chain (headroom.py:251-275) for every row of ``audio`` [streams, n] float32 and every gain scale.

    ``eq_settings`` (band_freqs / band_gains / band_qs) and ``chain_settings`` (the nested ``deesser`` / ``compressor`` /
    ``limiter`` dicts, or None) are the reference's, one for every stream or a list with one per stream.  Returns, per stream, one
    dict per scale with the keys of simulate_auto_eq_chain plus simulation_backend "rust" and safety_authority "authoritative".

    ``route``: "sweep" runs every (stream, scale) as a lane of the per-lane EQ and the compressor sweep, in chunks whose lane-EQ
    output stays under ``max_lane_eq_bytes``; "engine" calls simulate_auto_eq_chain_batch once per scale; "auto" takes the sweep
    for the streams whose settings it expresses (compressor and limiter enabled, auto-makeup off, at most 2048 control blocks)
    and the engine for the rest.  ``return_rows`` (route "sweep" only) returns {"results", "rows" [blocks, streams, scales]}.
    ``timing``: a dict that receives the summed kernel times of the sweep route."""
    started = time.perf_counter()
    if route not in ("auto", "sweep", "engine"):
        raise ValueError(f"route must be 'auto', 'sweep' or 'engine', got {route!r}")
    if not np.isfinite(fs) or fs <= 0.0:
        raise ValueError("sample_rate must be positive and finite")
    audio = np.ascontiguousarray(audio, dtype=np.float32)
    if audio.ndim != 2:
        raise TypeError("audio must be [n_streams, n_samples]")
    n_streams, n = audio.shape
    scales = tuple(float(v) for v in scales)
    if not scales:
        raise ValueError("scales must not be empty")
    bands = [_bands_from_settings(e) for e in _per_stream(eq_settings, n_streams, "eq_settings")]
    flats = [_flatten_chain_settings(c) for c in _per_stream(chain_settings, n_streams, "chain_settings")]
    expressible = [_sweep_expresses(flat, n, float(fs)) for flat in flats]
    if route == "sweep" and not all(expressible):
        raise ValueError("route 'sweep' simulates compressor and limiter with auto-makeup off over at most 2048 control blocks; "
                         f"stream {expressible.index(False)} asks for something else (use route 'auto' or 'engine')")
    if return_rows and route != "sweep":
        raise ValueError("return_rows needs route 'sweep'")
    on_sweep = [s for s in range(n_streams) if expressible[s] and route != "engine"]
    on_engine = [s for s in range(n_streams) if s not in set(on_sweep)]
    timing = {} if timing is None else timing
    results: list = [[None] * len(scales) for _ in range(n_streams)]
    rows = None
    if on_sweep:
        records, rows = _sweep_route(np.ascontiguousarray(audio[on_sweep]), float(fs), [bands[s] for s in on_sweep],
                                     [flats[s] for s in on_sweep], scales, device, max_lane_eq_bytes, return_rows, timing)
        for s, lanes in zip(on_sweep, records):
            results[s] = [simulation_dict(record) for record in lanes]
    if on_engine:
        sub = np.ascontiguousarray(audio[on_engine])
        settings = [_engine_settings(flats[s]) for s in on_engine]
        for k, scale in enumerate(scales):
            _, dicts = _render(sub, float(fs), [_scaled_bands(bands[s], scale) for s in on_engine], settings, device)
            for s, d in zip(on_engine, dicts):
                results[s][k] = d
    runtime_ms = (time.perf_counter() - started) * 1000.0
    for per_scale in results:
        for d in per_scale:
            d["candidate_runtime_ms"] = runtime_ms
            d["simulation_backend"] = "rust"
            d["safety_authority"] = "authoritative"
    if return_rows:
        return {"results": results, "rows": rows}
    return results


def apply_headroom_validation_batch(audio, fs: float, eq_settings, chain_settings=None, route: str = "auto", device: int = 0,
                                    max_lane_eq_bytes: int = DEFAULT_LANE_EQ_BYTES, timing: dict | None = None) -> list:
    """apply_headroom_validation (headroom.py:292-354) for every row of ``audio`` [streams, n] float32: per stream the input
    ``eq_settings`` deep-copied with band_gains scaled by the first headroom-safe scale of HEADROOM_SCALES (0.0 when none is),
    validation_gain_scale, the capped validation_confidence / analysis_confidence, headroom_validation, headroom_safe,
    headroom_advisory and headroom_gain_scale.  All seven scales are simulated; the reference stops at the first safe one, which is
    the one selected here.  A ``band_gains`` that is not ten values returns the copy untouched (:303-304)."""
    audio = np.ascontiguousarray(audio, dtype=np.float32)
    if audio.ndim != 2:
        raise TypeError("audio must be [n_streams, n_samples]")
    n_streams = audio.shape[0]
    results = [deepcopy(e) for e in _per_stream(eq_settings, n_streams, "eq_settings")]
    chains = _per_stream(chain_settings, n_streams, "chain_settings")
    gains = [np.asarray(r.get("band_gains", []), dtype=float) for r in results]
    members = [s for s in range(n_streams) if gains[s].size == core.NUM_BANDS]
    if not members:
        return results
    simulations = simulate_candidate_chain_batch(np.ascontiguousarray(audio[members]), fs, [results[s] for s in members],
                                                 [chains[s] for s in members], HEADROOM_SCALES, route, device, max_lane_eq_bytes,
                                                 timing=timing)
    for s, per_scale in zip(members, simulations):
        result, before = results[s], per_scale[0]
        index = next((k for k, d in enumerate(per_scale) if _is_headroom_safe(d)), len(HEADROOM_SCALES) - 1)
        selected, scale = per_scale[index], HEADROOM_SCALES[index]
        result["band_gains"] = (gains[s] if index == 0 else gains[s] * scale).tolist()  # :309, :313-318
        result["validation_gain_scale"] = float(_as_float(result.get("validation_gain_scale"), 1.0) * scale)
        meets = _is_headroom_safe(selected)
        authoritative = selected.get("simulation_backend") == "rust"
        safe = bool(meets and authoritative)
        if not safe:
            result["validation_confidence"] = float(min(_as_float(result.get("validation_confidence"), 1.0), 0.42))
            result["analysis_confidence"] = float(min(_as_float(result.get("analysis_confidence"), 1.0), 0.58))
        elif scale < 1.0:
            result["validation_confidence"] = float(min(_as_float(result.get("validation_confidence"), 1.0), 0.72))
        result["headroom_validation"] = {"safe": safe, "authoritative": authoritative, "advisory": not authoritative,
                                         "meets_advisory_thresholds": meets, "gain_scale": scale, "before": before, "after": selected,
                                         "status": "safe" if safe else "risk" if authoritative else "advisory"}
        result["headroom_safe"] = safe
        result["headroom_advisory"] = not authoritative
        result["headroom_gain_scale"] = scale
    return results


def simulate_candidate_chain(audio_data, sample_rate: int, eq_settings, chain_settings=None) -> dict:
    """headroom.py:251-275 with the reference's signature: one capture, scale 1.0."""
    audio = np.ascontiguousarray(audio_data, dtype=np.float32).reshape(1, -1)
    return simulate_candidate_chain_batch(audio, sample_rate, eq_settings, chain_settings)[0][0]


def apply_headroom_validation(audio_data, sample_rate: int, eq_settings, chain_settings=None) -> dict:
    """headroom.py:292-354 with the reference's signature: one capture."""
    audio = np.ascontiguousarray(audio_data, dtype=np.float32).reshape(1, -1)
    return apply_headroom_validation_batch(audio, sample_rate, eq_settings, chain_settings)[0]
