"""The streaming lane chain: one processor per stream, each under its own settings, state carried from call to call.

The reference configures one processor per caller (python/mic_eq/config_parts/settings.py:543-593).  An ``Engine`` preset is a
64-stream group; a ``LaneChain`` stream is one lane of a wave with its own EQ bands, compressor, limiter and stage switches,
and one slot can be configured again for a new caller while its neighbours keep running.  Each stream runs what
``simulate_auto_eq_chain`` configures (python_api.rs:400-487) without the de-esser: input scrub -> ten-band EQ -> compressor ->
limiter -> true-peak limiter -> block statistics.  The kernels are csrc/af_lane_chain.hip's; there is no CPU audio path.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Mapping, Sequence

import numpy as np

from . import _lib
from ._lib import BlockStats, LaneChainSettings
from .mic_eq_core import CAREFUL_OUTPUT_CEILING_DB, NUM_BANDS, STATS_DTYPE, _get

DEFAULT_LOOKAHEAD_MS = 2.0  # python_api.rs:472-476


def refuse_unsupported(settings: Mapping[str, object] | None, lookahead_ms: float) -> None:
    """NotImplementedError, naming the setting, for what a lane does not run (it stays with ``Engine``)."""
    if settings is None:
        return
    if _get(settings, "deesser_enabled", False):
        raise NotImplementedError("deesser_enabled: the lane chain has no de-esser; use an Engine preset")
    if _get(settings, "compressor_auto_makeup_enabled", False):
        raise NotImplementedError("compressor_auto_makeup_enabled: the lane chain runs the compressor with auto-makeup off; use an Engine preset")
    if settings.get("eq_bands_v2") is not None:
        raise NotImplementedError("eq_bands_v2: the lane chain runs the ten legacy (frequency, gain, Q) bands; use an Engine preset")
    if _get(settings, "eq_before_deesser", False):
        raise NotImplementedError("eq_before_deesser: the lane chain has no de-esser to order the EQ against; use an Engine preset")
    lookahead = _get(settings, "limiter_lookahead_ms", float(lookahead_ms))
    if lookahead != float(lookahead_ms):
        raise NotImplementedError(f"limiter_lookahead_ms: {lookahead} differs from the object's {float(lookahead_ms)} "
                                  "(the lookahead is fixed when the LaneChain is created)")


def effective_ceiling_db(settings: Mapping[str, object] | None) -> float:
    """effective_limiter_ceiling_db, audio/processor/control.rs:904-910, then ``as f32``."""
    ceiling_db = _get(settings, "limiter_ceiling_db", -0.5)
    careful = _get(settings, "limiter_careful_output_enabled", True)
    return float(np.float32(min(ceiling_db, CAREFUL_OUTPUT_CEILING_DB) if careful else ceiling_db))


def settings_record(bands, settings: Mapping[str, object] | None, lookahead_ms: float = DEFAULT_LOOKAHEAD_MS) -> LaneChainSettings:
    """One stream's ``af_lane_chain_settings`` from the arguments of ``simulate_auto_eq_chain`` (its defaults included);
    ``eq_enabled`` (default on) is the processor's own switch, which the simulation has no key for."""
    refuse_unsupported(settings, lookahead_ms)
    if len(bands) != NUM_BANDS:
        raise ValueError(f"expected {NUM_BANDS} EQ bands, got {len(bands)}")
    r = LaneChainSettings()
    for i, (frequency, gain_db, q) in enumerate(bands):
        r.bands[i][0], r.bands[i][1], r.bands[i][2] = float(frequency), float(gain_db), float(q)
    r.eq_enabled = int(_get(settings, "eq_enabled", True))
    r.compressor_enabled = int(_get(settings, "compressor_enabled", True))
    r.compressor_threshold_db = _get(settings, "compressor_threshold_db", -20.0)
    r.compressor_ratio = _get(settings, "compressor_ratio", 4.0)
    r.compressor_attack_ms = _get(settings, "compressor_attack_ms", 10.0)
    r.compressor_release_ms = _get(settings, "compressor_release_ms", 200.0)
    r.compressor_makeup_gain_db = _get(settings, "compressor_makeup_gain_db", 0.0)
    r.compressor_adaptive_release = int(_get(settings, "compressor_adaptive_release", False))
    r.compressor_base_release_ms = _get(settings, "compressor_base_release_ms", 50.0)
    r.compressor_sidechain_highpass_enabled = int(_get(settings, "compressor_sidechain_highpass_enabled", True))
    r.limiter_enabled = int(_get(settings, "limiter_enabled", True))
    r.limiter_ceiling_db = _get(settings, "limiter_ceiling_db", -0.5)
    r.limiter_careful_output_enabled = int(_get(settings, "limiter_careful_output_enabled", True))
    r.limiter_release_ms = _get(settings, "limiter_release_ms", 50.0)
    return r


def _per_stream(bands, settings, n: int) -> tuple[list, list]:
    """``bands`` / ``settings`` as one value for all n streams or one per stream -> two lists of n."""
    per_stream_bands = len(bands) > 0 and isinstance(bands[0], (list, tuple)) and len(bands[0]) > 0 and isinstance(bands[0][0], (list, tuple))
    per_bands = list(bands) if per_stream_bands else [bands] * n
    per_settings = list(settings) if isinstance(settings, (list, tuple)) else [settings] * n
    if len(per_bands) != n or len(per_settings) != n:
        raise ValueError(f"expected one preset per stream ({n}), got {len(per_bands)} band lists and {len(per_settings)} settings")
    return per_bands, per_settings


class LaneChain:
    """``n_streams`` independent dynamics chains resident on one GPU, one lane each.

    ``configure(streams, bands, settings)`` makes the listed streams fresh processors under new settings (at any time between
    calls; every other stream continues bit for bit), ``process`` runs one call over ``[n_streams, n]`` audio, ``block_stats``
    returns the call's rows in ``Engine.block_stats()``'s dtype.  A stream that was never configured runs the processor's
    defaults (flat EQ, compressor off, limiter at -0.5 dB)."""

    def __init__(self, sample_rate: float = 48_000.0, n_streams: int = 1, device: int = 0,
                 limiter_lookahead_ms: float = DEFAULT_LOOKAHEAD_MS):
        self._lib = _lib.load()
        handle = C.c_void_p()
        _lib.check(self._lib.af_lane_chain_create(float(sample_rate), int(n_streams), float(limiter_lookahead_ms), int(device),
                                                  C.byref(handle)))
        self._h = handle
        self.sample_rate = float(sample_rate)
        self.n_streams = int(n_streams)
        self.device = int(device)
        self.limiter_lookahead_ms = float(limiter_lookahead_ms)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_lane_chain_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def configure(self, streams: Sequence[int], bands, settings=None) -> None:
        """Host work only: the streams' columns reach the device with the next ``process`` call."""
        streams = [int(s) for s in streams]
        per_bands, per_settings = _per_stream(bands, settings, len(streams))
        records = (LaneChainSettings * max(len(streams), 1))()
        for i, (b, st) in enumerate(zip(per_bands, per_settings)):
            records[i] = settings_record(b, st, self.limiter_lookahead_ms)
        index = (C.c_int32 * max(len(streams), 1))(*streams)
        _lib.check(self._lib.af_lane_chain_configure(self._h, index, len(streams), records))

    def process(self, audio: np.ndarray) -> np.ndarray:
        audio = np.ascontiguousarray(audio, dtype=np.float32)
        if audio.ndim != 2 or audio.shape[0] != self.n_streams:
            raise ValueError(f"audio must be [n_streams = {self.n_streams}, n_samples]")
        out = np.empty_like(audio)
        n = audio.shape[1]
        fp = C.POINTER(C.c_float)
        _lib.check(self._lib.af_lane_chain_process_host(self._h, audio.ctypes.data_as(fp), out.ctypes.data_as(fp), n, max(n, 1)))
        return out

    def process_device(self, in_ptr: int, out_ptr: int, n_samples: int, stride: int, hip_stream: int = 0) -> None:
        """Device pointers (e.g. ``tensor.data_ptr()``) to [n_streams][stride] float32; asynchronous on ``hip_stream``."""
        _lib.check(self._lib.af_lane_chain_process_device(self._h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), int(n_samples), int(stride),
                                                          C.c_void_p(hip_stream)))

    def block_stats(self) -> np.ndarray:
        """Structured array [blocks, n_streams] of the last process call."""
        blocks = int(self._lib.af_lane_chain_blocks(self._h))
        rows = np.zeros((blocks, self.n_streams), dtype=STATS_DTYPE)
        if blocks:
            _lib.check(self._lib.af_lane_chain_read_rows(self._h, rows.ctypes.data_as(C.POINTER(BlockStats)), rows.size))
        return rows

    def reset(self) -> None:
        _lib.check(self._lib.af_lane_chain_reset(self._h))

    def samples_processed(self, stream: int) -> int:
        n = C.c_int64(0)
        _lib.check(self._lib.af_lane_chain_samples_processed(self._h, int(stream), C.byref(n)))
        return int(n.value)

    def last_kernel_ms(self) -> float:
        ms = C.c_double(0.0)
        _lib.check(self._lib.af_lane_chain_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value


def simulate_lanes(audio: np.ndarray, sample_rate: float, bands, settings, device: int) -> tuple[np.ndarray, np.ndarray, list[float]]:
    """``simulate_auto_eq_chain_batch``'s ``route="lanes"``: (output, rows [blocks, n_streams], effective ceiling per stream).
    Everything that can be refused is refused before any device work."""
    n_streams, n = audio.shape
    per_bands, per_settings = _per_stream(bands, settings, n_streams)
    lookaheads = {_get(st, "limiter_lookahead_ms", DEFAULT_LOOKAHEAD_MS) for st in per_settings}
    if len(lookaheads) > 1:
        raise NotImplementedError(f"limiter_lookahead_ms: the streams of one LaneChain share one lookahead, got {sorted(lookaheads)}")
    lookahead = lookaheads.pop()
    chain = LaneChain(sample_rate, n_streams, device, lookahead)  # (host work only, like configure)
    try:
        chain.configure(range(n_streams), per_bands, per_settings)  # the refusals
        output = chain.process(audio) if n else audio.copy()
        rows = chain.block_stats()
    finally:
        chain.close()
    return output, rows, [effective_ceiling_db(st) for st in per_settings]


__all__ = ["LaneChain", "LaneChainSettings", "settings_record", "simulate_lanes"]
