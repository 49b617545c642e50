"""Compressor candidate sweep: many (capture, candidate) chain simulations over one de-esser and EQ pass per capture.

The reference's compressor calibration (python/mic_eq/analysis/voice_setup.py:699-1079) calls simulate_auto_eq_chain once per
candidate (threshold, ratio, attack, release) of a capture.  Here the capture's compressor input -- an engine run with the
compressor and the limiter disabled -- is made once, and every candidate is a lane of ``cs_sweep_kernel``
(csrc/af_compressor_search.hip), which runs compressor -> limiter -> true-peak limiter with per-lane parameters; the lanes'
rows are folded into the reference's result dict on the device (``cs_fold_kernel``).
"""
from __future__ import annotations

import ctypes as C
import time
from typing import Any, Mapping

import numpy as np

from . import _lib
from . import mic_eq_core as core
from ._lib import BlockStats, ChainSimulation, CompressorBase, CompressorCandidate

MAX_BLOCKS = 2048  # control blocks per capture the fold holds (csrc/af_compressor_search_host.hpp)
SIMULATION_DTYPE = np.dtype([(name, {C.c_float: "<f4", C.c_uint64: "<u8", C.c_int32: "<i4"}[ctype]) for name, ctype in ChainSimulation._fields_])
assert SIMULATION_DTYPE.itemsize == C.sizeof(ChainSimulation)
_RAW_FIELDS = ("output_sample_peak", "pre_limiter_true_peak", "output_true_peak", "output_rms")
_FRONT_END_KEYS = ("eq_bands_v2", "eq_before_deesser", "deesser_enabled", "deesser_auto_enabled", "deesser_auto_amount", "deesser_low_cut_hz",
                   "deesser_high_cut_hz", "deesser_threshold_db", "deesser_ratio", "deesser_attack_ms", "deesser_release_ms",
                   "deesser_max_reduction_db")
_LIMITER_DEFAULTS = (("limiter_ceiling_db", -0.5), ("limiter_release_ms", 50.0), ("limiter_lookahead_ms", 2.0),
                     ("limiter_careful_output_enabled", True))


class CompressorSearch:
    """A batch of captures on the device and sweeps of compressor candidates over them (af_compressor_search_*)."""

    def __init__(self, sample_rate: float = 48_000.0, device: int = 0):
        self._lib = _lib.load()
        handle = C.c_void_p()
        _lib.check(self._lib.af_compressor_search_create(float(sample_rate), int(device), C.byref(handle)))
        self._h = handle
        self.sample_rate = float(sample_rate)
        self.n_captures = self.n_samples = self.n_lanes = 0

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_compressor_search_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_limiter(self, ceiling_db: float = -1.5, release_ms: float = 80.0, lookahead_ms: float = 2.0, careful_output: bool = True) -> None:
        _lib.check(self._lib.af_compressor_search_set_limiter(self._h, float(ceiling_db), float(release_ms), float(lookahead_ms),
                                                              int(bool(careful_output))))

    def load(self, compressor_input: np.ndarray, input_rows: np.ndarray) -> None:
        """``compressor_input`` [captures, n] float32 and the [blocks, captures] rows of the engine run that made it."""
        audio = np.ascontiguousarray(compressor_input, dtype=np.float32)
        rows = np.ascontiguousarray(input_rows, dtype=core.STATS_DTYPE)
        if audio.ndim != 2 or rows.ndim != 2 or rows.shape[1] != audio.shape[0]:
            raise ValueError("expected audio [captures, n] and rows [blocks, captures]")
        block = int(min(max(round(self.sample_rate * 0.020), 1), 8192))
        if rows.shape[0] != -(-audio.shape[1] // block):
            raise ValueError(f"expected {-(-audio.shape[1] // block)} rows per capture, got {rows.shape[0]}")
        _lib.check(self._lib.af_compressor_search_load_host(self._h, audio.ctypes.data_as(C.POINTER(C.c_float)), int(audio.shape[1]),
                                                            int(audio.shape[0]), int(audio.shape[1]), rows.ctypes.data_as(C.POINTER(BlockStats))))
        self.n_captures, self.n_samples = audio.shape
        self.n_lanes = 0

    def load_device(self, pointer: int, n_samples: int, n_captures: int, stride: int, input_rows: np.ndarray) -> None:
        """As ``load`` for [n_captures][stride] float32 already on the device; the memory must stay alive while it is loaded."""
        rows = np.ascontiguousarray(input_rows, dtype=core.STATS_DTYPE)
        _lib.check(self._lib.af_compressor_search_load_device(self._h, C.c_void_p(pointer), int(n_samples), int(n_captures), int(stride),
                                                              rows.ctypes.data_as(C.POINTER(BlockStats))))
        self.n_captures, self.n_samples, self.n_lanes = int(n_captures), int(n_samples), 0

    def sweep(self, candidates, bases, keep_audio: bool = False) -> np.ndarray:
        """``candidates``: rows of (capture, threshold_db, ratio, attack_ms, release_ms); ``bases``: per capture
        (makeup_gain_db, base_release_ms, adaptive_release, sidechain_highpass_enabled).  Returns one SIMULATION_DTYPE
        record per candidate."""
        lanes = (CompressorCandidate * len(candidates))()
        for i, (capture, threshold_db, ratio, attack_ms, release_ms) in enumerate(candidates):
            lanes[i] = CompressorCandidate(int(capture), 0, float(threshold_db), float(ratio), float(attack_ms), float(release_ms))
        if len(bases) != self.n_captures:
            raise ValueError(f"expected one base per capture ({self.n_captures}), got {len(bases)}")
        base = (CompressorBase * len(bases))()
        for i, (makeup, base_release, adaptive, sidechain) in enumerate(bases):
            base[i] = CompressorBase(float(makeup), float(base_release), int(bool(adaptive)), int(bool(sidechain)))
        out = np.zeros(len(candidates), dtype=SIMULATION_DTYPE)
        _lib.check(self._lib.af_compressor_search_sweep(self._h, lanes, len(candidates), base, int(bool(keep_audio)),
                                                        out.ctypes.data_as(C.POINTER(ChainSimulation))))
        self.n_lanes = len(candidates)
        return out

    def masks(self) -> dict:
        """What the host derived per capture at load: in_db, active and audible [captures, blocks], active_threshold_db."""
        blocks = int(self._lib.af_compressor_search_blocks(self._h))
        in_db = np.zeros((self.n_captures, blocks), dtype=np.float32)
        mask = np.zeros((self.n_captures, blocks), dtype=np.uint8)
        threshold = np.zeros(self.n_captures, dtype=np.float32)
        _lib.check(self._lib.af_compressor_search_read_masks(self._h, in_db.ctypes.data_as(C.POINTER(C.c_float)),
                                                             mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                             threshold.ctypes.data_as(C.POINTER(C.c_float))))
        return {"in_db": in_db, "active": (mask & 1) != 0, "audible": (mask & 2) != 0, "active_threshold_db": threshold}

    def rows(self) -> np.ndarray:
        """[blocks, lanes] block rows of the last sweep, in the engine's row format."""
        blocks = int(self._lib.af_compressor_search_blocks(self._h))
        rows = np.zeros((blocks, self.n_lanes), dtype=core.STATS_DTYPE)
        _lib.check(self._lib.af_compressor_search_read_rows(self._h, rows.ctypes.data_as(C.POINTER(BlockStats)), rows.size))
        return rows

    def audio(self) -> np.ndarray:
        """[lanes, n] output audio of the last sweep (``keep_audio=True``)."""
        out = np.empty((self.n_lanes, self.n_samples), dtype=np.float32)
        _lib.check(self._lib.af_compressor_search_read_audio(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), int(self.n_samples)))
        return out

    def last_kernel_ms(self) -> dict:
        sweep, fold = C.c_double(0.0), C.c_double(0.0)
        _lib.check(self._lib.af_compressor_search_last_kernel_ms(self._h, C.byref(sweep), C.byref(fold)))
        return {"sweep": sweep.value, "fold": fold.value}

    def last_run_ms(self) -> dict:
        """Kernel ms of the last run's three sweeps."""
        ms = (C.c_double * 6)()
        _lib.check(self._lib.af_compressor_search_last_run_ms(self._h, ms))
        return {"phase1_sweep": ms[0], "phase1_fold": ms[1], "phase2_sweep": ms[2], "phase2_fold": ms[3], "verification_sweep": ms[4],
                "verification_fold": ms[5]}

    def run(self, settings) -> list:
        """The reference's calibration search for every loaded capture (af_compressor_search_run).  ``settings``: one
        mapping per capture with the fields of af_compressor_search_settings.  Returns the result structures."""
        if len(settings) != self.n_captures:
            raise ValueError(f"expected one settings entry per capture ({self.n_captures}), got {len(settings)}")
        arr = (_lib.CompressorSearchSettings * len(settings))()
        for i, st in enumerate(settings):
            arr[i] = _lib.CompressorSearchSettings(**{name: (int(st[name]) if kind is C.c_int32 else float(st[name]))
                                                      for name, kind in _lib.CompressorSearchSettings._fields_ if name != "reserved"})
        out = (_lib.CompressorSearchResult * len(settings))()
        _lib.check(self._lib.af_compressor_search_run(self._h, arr, out))
        self.n_lanes = 0
        return list(out)


def _front_end_settings(settings: Mapping[str, object] | None) -> dict:
    """The chain settings of the run that makes the compressor input: de-esser and EQ as given, compressor and limiter off."""
    out = {key: settings[key] for key in _FRONT_END_KEYS if settings is not None and settings.get(key) is not None}
    out["compressor_enabled"] = False
    out["limiter_enabled"] = False
    return out


def compressor_input_batch(audio: np.ndarray, sample_rate: float, bands, settings, device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """What the compressor of every stream's chain sees, and the rows of that run: one engine call per distinct de-esser and EQ
    configuration (streams that share one run together; a stream count needs no padding, since the whole engine has one preset).

    ``bands`` / ``settings``: one preset for every stream or one entry per stream, as simulate_auto_eq_chain_batch takes them.
    Returns ([n_streams, n] float32, [blocks, n_streams] rows)."""
    audio = np.ascontiguousarray(audio, dtype=np.float32)
    n_streams, n = audio.shape
    per_stream = core._is_preset_list(bands, settings)
    per_bands = list(bands) if (per_stream and len(bands) and isinstance(bands[0][0], (list, tuple))) else [bands] * n_streams
    per_settings = list(settings) if isinstance(settings, (list, tuple)) else [settings] * n_streams
    if len(per_bands) != n_streams or len(per_settings) != n_streams:
        raise ValueError(f"expected one preset per stream ({n_streams}), got {len(per_bands)} band lists and {len(per_settings)} settings")
    groups: dict = {}
    for s, (b, st) in enumerate(zip(per_bands, per_settings)):
        if len(b) != core.NUM_BANDS:
            raise ValueError(f"expected {core.NUM_BANDS} EQ bands, got {len(b)}")
        front = _front_end_settings(st)
        key = (repr([tuple(x) for x in b]), repr(sorted(front.items(), key=lambda kv: kv[0])))
        groups.setdefault(key, (b, front, []))[2].append(s)
    block = int(min(max(round(sample_rate * 0.020), 1), 8192))
    out = np.empty_like(audio)
    rows = np.zeros((-(-n // block), n_streams), dtype=core.STATS_DTYPE)
    for b, front, members in groups.values():
        engine = core.Engine(sample_rate, len(members), device)
        try:
            core.configure_auto_eq_chain(engine, float(sample_rate), b, front)
            out[members] = engine.process(audio[members])
            rows[:, members] = engine.block_stats()
        finally:
            engine.close()
    return out, rows


def _uniform_limiter(per_settings) -> tuple:
    values = {tuple(core._get(st, key, default) for key, default in _LIMITER_DEFAULTS) for st in per_settings}
    if len(values) != 1:
        raise ValueError("the limiter settings must be the same for every stream of a sweep")
    for st in per_settings:
        if not core._get(st, "limiter_enabled", True) or not core._get(st, "compressor_enabled", True):
            raise NotImplementedError("a compressor sweep simulates compressor and limiter; a setting disables one of them")
        if core._get(st, "compressor_auto_makeup_enabled", False):
            raise NotImplementedError("a compressor sweep runs the compressor with auto-makeup off (voice_setup.py:742-747); "
                                      "turn compressor_auto_makeup_enabled off in the settings")
    return values.pop()


def simulation_dict(record) -> dict[str, Any]:
    """One SIMULATION_DTYPE record as the reference's result dict (python_api.rs:649-712)."""
    d: dict[str, Any] = {}
    for name in SIMULATION_DTYPE.names:
        if name in _RAW_FIELDS:
            continue
        value = record[name]
        if name in ("true_peak_limited_events", "active_analysis_block_count", "processed_samples"):
            d[name] = int(value)
        elif name == "non_finite_output":
            d[name] = bool(value)
        else:
            d[name] = float(value)
    return d


def simulate_compressor_candidates_batch(audio: np.ndarray, sample_rate: float, bands, settings, candidates, device: int = 0,
                                         return_rows: bool = False, return_output_audio: bool = False):
    """simulate_auto_eq_chain for many compressor candidates per stream, with one de-esser and EQ pass per stream.

    ``audio`` [n_streams, n] float32; ``bands`` / ``settings`` as simulate_auto_eq_chain_batch takes them (one preset, or one
    per stream); ``candidates``: rows of (stream, threshold_db, ratio, attack_ms, release_ms) that replace the settings'
    compressor_threshold_db / _ratio / _attack_ms / _release_ms.  The limiter settings must be the same for every stream.

    Returns one reference-shaped dict per candidate; with ``return_rows`` / ``return_output_audio`` a dict
    {"results", "records" (the SIMULATION_DTYPE array behind them), "rows" [blocks, candidates] or None,
    "output_audio" [candidates, n] or None} instead."""
    started = time.perf_counter()
    if not np.isfinite(sample_rate) or sample_rate <= 0.0:
        raise ValueError("sample_rate must be positive and finite")
    audio = np.ascontiguousarray(audio, dtype=np.float32)
    if audio.ndim != 2:
        raise TypeError("audio must be [n_streams, n_samples]")
    n_streams = audio.shape[0]
    per_settings = list(settings) if isinstance(settings, (list, tuple)) else [settings] * n_streams
    ceiling_db, release_ms, lookahead_ms, careful = _uniform_limiter(per_settings)
    comp_in, input_rows = compressor_input_batch(audio, sample_rate, bands, settings, device)
    bases = [(core._get(st, "compressor_makeup_gain_db", 0.0), core._get(st, "compressor_base_release_ms", 50.0),
              core._get(st, "compressor_adaptive_release", False), core._get(st, "compressor_sidechain_highpass_enabled", True))
             for st in per_settings]
    search = CompressorSearch(sample_rate, device)
    try:
        search.set_limiter(ceiling_db, release_ms, lookahead_ms, careful)
        search.load(comp_in, input_rows)
        records = search.sweep(candidates, bases, keep_audio=return_output_audio)
        rows = search.rows() if return_rows else None
        output = search.audio() if return_output_audio else None
    finally:
        search.close()
    runtime_ms = (time.perf_counter() - started) * 1000.0
    results = []
    for record in records:
        d = simulation_dict(record)
        d["candidate_runtime_ms"] = runtime_ms
        results.append(d)
    if return_rows or return_output_audio:
        return {"results": results, "records": records, "rows": rows, "output_audio": output}
    return results


# ------------------------------------------------------------------------------------------- the calibration search
SEARCH_BUDGET = 68  # _COMPRESSOR_SEARCH_BUDGET, voice_setup.py:699
SEARCH_CONTROLS = ("threshold_db", "ratio", "attack_ms", "release_ms")
OBJECTIVE_NORMALIZERS = {"loudness_error_db": 2.0, "median_gr_error_db": 1.0, "p95_gr_error_db": 1.0, "headroom_shortfall_db": 1.0,
                         "pumping_score_db": 1.0, "silence_gain_excess_db": 1.0, "activity_ratio_deficit": 0.20}  # :706-714
OBJECTIVE_WEIGHTS = {"loudness": 1.00, "median_gr": 0.35, "p95_gr": 0.90, "headroom": 0.45, "pumping": 0.30, "silence_gain": 1.50,
                     "activity": 0.25, "prior": 0.08}  # :715-724
_DEESSER_DEFAULTS = (("enabled", False), ("auto_enabled", True), ("auto_amount", 0.5), ("low_cut_hz", 4000.0), ("high_cut_hz", 11000.0),
                     ("threshold_db", -28.0), ("ratio", 4.0), ("attack_ms", 2.0), ("release_ms", 80.0), ("max_reduction_db", 6.0))


def _per_stream(value, n_streams: int, what: str) -> list:
    if isinstance(value, (list, tuple)):
        if len(value) != n_streams:
            raise ValueError(f"expected one {what} per stream ({n_streams}), got {len(value)}")
        return list(value)
    return [value] * n_streams


def _bands_from_settings(eq_settings: Mapping[str, Any]) -> list:
    """auto_eq_parts/headroom.py:87-96."""
    freqs, gains, qs = (list(eq_settings.get(key) or []) for key in ("band_freqs", "band_gains", "band_qs"))
    if not (len(freqs) == len(gains) == len(qs) == core.NUM_BANDS):
        raise ValueError("Auto-EQ settings must contain 10 frequencies, gains, and Q values")
    return [(float(f), float(g), float(q)) for f, g, q in zip(freqs, gains, qs)]


def _search_settings(compressor: Mapping[str, Any], target_p95_db: float, target_median_db: float, peak_cap_db: float) -> dict:
    """One capture's af_compressor_search_settings; the defaults are those of auto_eq_parts/headroom.py:63-76."""
    get = lambda key, default: compressor[key] if compressor.get(key) is not None else default  # noqa: E731
    return {"threshold_db": float(compressor["threshold_db"]), "ratio": float(compressor["ratio"]), "attack_ms": float(compressor["attack_ms"]),
            "release_ms": float(compressor["release_ms"]), "makeup_gain_db": float(get("makeup_gain_db", 0.0)),
            "base_release_ms": float(get("base_release_ms", 50.0)), "adaptive_release": bool(get("adaptive_release", False)),
            "sidechain_highpass_enabled": bool(get("sidechain_highpass_enabled", True)),
            "auto_makeup_enabled": bool(get("auto_makeup_enabled", False)), "target_lufs": float(get("target_lufs", -18.0)),
            "measured_short_term_lufs": float(get("measured_short_term_lufs", -18.0)), "target_p95_db": float(target_p95_db),
            "target_median_db": float(target_median_db), "peak_cap_db": float(peak_cap_db)}


def _calibration_dicts(compressor: Mapping[str, Any], st: Mapping[str, Any], r, runtime_ms: float) -> tuple[dict, dict]:
    """(calibrated, diagnostics) with the keys of voice_setup.py:754-768 and :1037-1078."""
    calibrated = dict(compressor)
    diagnostics: dict[str, Any] = {
        "backend": "unavailable", "objective": "bounded_multi_objective_compressor_search_v1",
        "target_p95_gain_reduction_db": st["target_p95_db"], "target_median_gain_reduction_db": st["target_median_db"],
        "peak_gain_reduction_cap_db": st["peak_cap_db"], "measured_p95_gain_reduction_db": 0.0, "measured_median_gain_reduction_db": 0.0,
        "measured_peak_gain_reduction_db": 0.0, "iterations": int(r.iterations), "candidate_budget": SEARCH_BUDGET,
        "objective_normalizers": dict(OBJECTIVE_NORMALIZERS), "objective_weights": dict(OBJECTIVE_WEIGHTS)}
    if not r.backend_available:
        diagnostics["search_runtime_ms"] = runtime_ms
        return calibrated, diagnostics
    calibrated.update({key: float(getattr(r, key)) for key in SEARCH_CONTROLS})
    diagnostics.update({
        "backend": "rust", "measured_median_gain_reduction_db": r.measured_median_gain_reduction_db,
        "measured_p95_gain_reduction_db": r.measured_p95_gain_reduction_db, "measured_peak_gain_reduction_db": r.measured_peak_gain_reduction_db,
        "active_reduction_ratio": r.active_reduction_ratio, "peak_cap_passed": bool(r.peak_cap_passed), "total_objective": r.total_objective,
        "incumbent_objective": r.incumbent_objective, "threshold_only_objective": r.threshold_only_objective,
        "expanded_candidate_objective": r.expanded_candidate_objective, "expanded_search_selected": bool(r.expanded_search_selected),
        "active_output_gain_db": r.active_output_gain_db, "silence_output_gain_db": r.silence_output_gain_db,
        "compressor_pumping_score_db": r.compressor_pumping_score_db, "output_true_peak_db": r.output_true_peak_db,
        "pre_limiter_true_peak_headroom_db": r.pre_limiter_true_peak_headroom_db, "search_runtime_ms": runtime_ms,
        "candidate_count": int(r.candidate_count), "iterations": int(r.iterations),
        "target_gain_reduction_db": st["target_p95_db"], "measured_gain_reduction_db": r.measured_p95_gain_reduction_db,
        "threshold_db": calibrated["threshold_db"], "ratio": calibrated["ratio"], "attack_ms": calibrated["attack_ms"],
        "release_ms": calibrated["release_ms"]})
    return calibrated, diagnostics


def calibrate_compressor_batch(speech, fs: float, eq_settings, deesser_settings, compressor_settings, target_p95_db, target_median_db,
                               peak_cap_db, device: int = 0, return_search: bool = False) -> list:
    """_calibrate_compressor_threshold (voice_setup.py:742-1079) for every row of ``speech`` [n_streams, n] float32.

    ``eq_settings`` (band_freqs / band_gains / band_qs), ``deesser_settings`` and ``compressor_settings`` are the reference's
    dicts, one for every stream or a list with one per stream; the three targets are numbers or one per stream.  Returns a
    list of (calibrated, diagnostics) with the reference's keys (``search_runtime_ms`` is the whole batch's); with
    ``return_search`` a third element holds the evaluated candidates, their scores and the winner's index.

    The de-esser and the EQ run once per stream; the up to 67 simulations of a stream are lanes of three sweeps."""
    started = time.perf_counter()
    audio = np.ascontiguousarray(speech, dtype=np.float32)
    if audio.ndim != 2:
        raise TypeError("speech must be [n_streams, n_samples]")
    n_streams = audio.shape[0]
    eq = _per_stream(eq_settings, n_streams, "eq_settings")
    deesser = _per_stream(deesser_settings, n_streams, "deesser_settings")
    compressor = _per_stream(compressor_settings, n_streams, "compressor_settings")
    targets = [_per_stream(v, n_streams, "target") for v in (target_p95_db, target_median_db, peak_cap_db)]
    bands = [_bands_from_settings(e) for e in eq]
    front = [{f"deesser_{key}": (d[key] if (d or {}).get(key) is not None else default) for key, default in _DEESSER_DEFAULTS} for d in deesser]
    comp_in, input_rows = compressor_input_batch(audio, float(fs), bands, front, device)
    settings = [_search_settings(c, targets[0][s], targets[1][s], targets[2][s]) for s, c in enumerate(compressor)]
    search = CompressorSearch(float(fs), device)  # the limiter is the search's fixed one
    try:
        search.load(comp_in, input_rows)
        results = search.run(settings)
    finally:
        search.close()
    runtime_ms = (time.perf_counter() - started) * 1000.0
    out = []
    for c, st, r in zip(compressor, settings, results):
        pair = _calibration_dicts(c, st, r, runtime_ms)
        if return_search:
            n = int(r.evaluated_count)
            pair += ({"evaluated": np.array([list(r.evaluated[i]) for i in range(n)], dtype=np.float64).reshape(n, 4),
                      "scores": np.array(list(r.scores)[:n], dtype=np.float64), "winner": int(r.winner),
                      "verification_equals_evaluation": bool(r.verification_equals_evaluation)},)
        out.append(pair)
    return out


def calibrate_compressor(*, speech_audio, sample_rate: int, eq_settings, deesser_settings, compressor_settings, target_p95_db: float,
                         target_median_db: float, peak_cap_db: float) -> tuple[dict, dict]:
    """_calibrate_compressor_threshold with the reference's signature: one capture."""
    audio = np.ascontiguousarray(speech_audio, dtype=np.float32).reshape(1, -1)
    return calibrate_compressor_batch(audio, sample_rate, eq_settings, deesser_settings, compressor_settings, target_p95_db,
                                      target_median_db, peak_cap_db)[0]
