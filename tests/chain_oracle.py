"""The oracle's block processor (`af_oracle_py.Chain`) configured as `simulate_auto_eq_chain` configures it, driven over
the same calls as an engine: every call starts a new control block, so a call whose length is not a multiple of the
control block ends in a short block -- as on the GPU.  `simulate_auto_eq_chain` runs one call; this runs any call
pattern and also returns the per-block rows, the de-esser's reduction among them.  The de-esser is set up as the simulation sets
it up, in either stage order; with the EQ, compressor and limiter switched off it runs alone.  Used by the tests only (CPU side
of a comparison)."""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import af_oracle_py as O

ROW_FIELDS = ("input_sample_peak", "output_sample_peak", "true_peak_limiter_input_peak", "output_true_peak",
              "limiter_peak_gain_reduction_db", "true_peak_limiter_gain_reduction_db", "true_peak_limited_events",
              "compressor_gain_reduction_db")
# the rows also carry the de-esser's per-block reduction (0 with the de-esser off); ROW_FIELDS stays what the chain tests walk over
ALL_ROW_FIELDS = ROW_FIELDS + ("deesser_gain_reduction_db",)
ROW_DTYPE = np.dtype([(name, "<u8" if name == "true_peak_limited_events" else "<f4") for name in ALL_ROW_FIELDS])


def _lib() -> C.CDLL:
    L = O.lib()
    if L.afo_sanitize_and_clamp.restype is not C.c_uint64:
        L.afo_sanitize_and_clamp.argtypes = [C.POINTER(C.c_float), C.c_size_t]
        L.afo_sanitize_and_clamp.restype = C.c_uint64
    return L


def control_block(sample_rate: float) -> int:
    return int(min(max(round(sample_rate * 0.020), 1), 8192))  # python_api.rs:512-514


def make_chain(sample_rate: float, bands, settings: dict | None, eq_enabled: bool = True) -> O.Chain:
    """afo_simulate_auto_eq_chain's set-up (af_oracle.c), step for step, on a fresh chain.  `eq_enabled=False` switches the EQ
    off afterwards (the simulation itself has no such setting; the compressor and the limiter have theirs), so that with
    `compressor_enabled` and `limiter_enabled` false a stage such as the de-esser runs alone."""
    s = O.settings_from_dict(settings)
    chain = O.Chain(float(sample_rate))
    L = chain.L
    chain.set("eq_enabled", 1)
    if s.has_eq_bands_v2:
        for i in range(10):
            L.afo_eq_set_band_config(chain.eq, i, C.byref(s.eq_bands_v2[i]))
        L.afo_eq_reset(chain.eq)
    else:
        for i, (frequency, gain, q) in enumerate(bands):
            L.afo_eq_set_band_frequency(chain.eq, i, float(frequency))
            L.afo_eq_set_band_gain(chain.eq, i, float(gain))
            L.afo_eq_set_band_q(chain.eq, i, float(q))
    chain.set("eq_before_deesser", s.eq_before_deesser)
    chain.set("deesser_enabled", s.deesser_enabled)
    if s.deesser_enabled:
        O.deesser_apply(chain.deesser, s)
    chain.set("compressor_enabled", s.compressor_enabled)
    if s.compressor_enabled:
        c = chain.compressor
        L.afo_compressor_set_threshold(c, s.compressor_threshold_db)
        L.afo_compressor_set_ratio(c, s.compressor_ratio)
        L.afo_compressor_set_attack_time(c, s.compressor_attack_ms)
        L.afo_compressor_set_release_time(c, s.compressor_release_ms)
        L.afo_compressor_set_makeup_gain(c, s.compressor_makeup_gain_db)
        L.afo_compressor_set_adaptive_release(c, s.compressor_adaptive_release)
        L.afo_compressor_set_base_release_time(c, s.compressor_base_release_ms)
        L.afo_compressor_set_auto_makeup_enabled(c, s.compressor_auto_makeup_enabled)
        L.afo_compressor_set_target_lufs(c, s.compressor_target_lufs)
        L.afo_compressor_set_sidechain_highpass_enabled(c, s.compressor_sidechain_highpass_enabled)
    chain.set("limiter_enabled", s.limiter_enabled)
    effective = float(np.float32(min(s.limiter_ceiling_db, -1.5) if s.limiter_careful_output_enabled else s.limiter_ceiling_db))
    if s.limiter_enabled:
        L.afo_limiter_set_lookahead_ms(chain.limiter, s.limiter_lookahead_ms)
        L.afo_limiter_set_ceiling(chain.limiter, effective)
        L.afo_limiter_set_release_time(chain.limiter, s.limiter_release_ms)
        L.afo_tp_limiter_set_release_ms(chain.tp_limiter, float(np.float32(s.limiter_release_ms)))
    if not eq_enabled:
        chain.set("eq_enabled", 0)
    return chain


def sanitize(x: np.ndarray, clamp: bool) -> np.ndarray:
    """What the engine does to its input first: non-finite samples to 0 (always), and with the input clamp on
    `afo_sanitize_and_clamp` (routing.rs:802-823)."""
    y = np.array(x, dtype=np.float32, copy=True)
    if clamp:
        _lib().afo_sanitize_and_clamp(y.ctypes.data_as(C.POINTER(C.c_float)), y.size)
    else:
        y[~np.isfinite(y)] = 0.0
    return y


def run_calls(x: np.ndarray, sample_rate: float, bands, settings: dict | None, calls, clamp: bool = False,
              eq_enabled: bool = True):
    """One stream through the chain in calls of the given lengths: (output float32, rows [blocks] of ROW_DTYPE)."""
    chain = make_chain(sample_rate, bands, settings, eq_enabled)
    y = sanitize(x, clamp)
    cb = control_block(sample_rate)
    rows = []
    at = 0
    for length in calls:
        for b0 in range(at, at + length, cb):
            block = y[b0 : min(b0 + cb, at + length)]
            st = chain.process_block(block)
            rows.append(tuple(getattr(st, name) for name in ALL_ROW_FIELDS))
        at += length
    return y[:at], np.array(rows, dtype=ROW_DTYPE)


def run_batch(audio: np.ndarray, sample_rate: float, bands, settings: dict | None, calls, clamp: bool = False,
              workers: int = 16, eq_enabled: bool = True):
    """run_calls over every stream of [n_streams, n] on up to `workers` threads (the oracle keeps no global state:
    every chain is its own allocation, and ctypes releases the GIL inside each call).
    Returns (output [n_streams, sum(calls)], rows [blocks, n_streams])."""
    _lib()  # (loaded, and its signatures set, before the threads start)
    n_streams = audio.shape[0]
    out = np.empty((n_streams, int(sum(calls))), dtype=np.float32)
    rows = [None] * n_streams

    def one(s):
        out[s], rows[s] = run_calls(audio[s], sample_rate, bands, settings, calls, clamp, eq_enabled)

    with ThreadPoolExecutor(max_workers=max(1, min(workers, n_streams))) as pool:
        list(pool.map(one, range(n_streams)))
    return out, np.stack(rows, axis=1)
