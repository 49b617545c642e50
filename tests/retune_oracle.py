"""The oracle's block processor retuned while it runs: `chain_oracle`'s chain driven over a list of calls, with a schedule of
setter calls applied to the LIVE chain between them -- what the reference's realtime control plane does at the top of a
wake-up (audio/processor/control.rs:844-919).  The `afo_*` setters act on the running objects and keep their state, so this
is the CPU side of the live-control comparisons (tests/test_gpu_live_control.py).  Used by the tests only.

A schedule is `{call index: [(setter, args), ...]}`; the setters of call k are applied, in order, before the first sample
of call k.  Setter names are the engine's method names (`eq_set_band_gain`, `compressor_set_threshold`, ...), so one
schedule drives both sides (`apply_to_engine`).  `eq_set_band_config` takes `(band, (type name, Hz, dB, Q, slope, enabled))`.
"""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import af_oracle_py as O
import chain_oracle as CO

ROW_FIELDS = CO.ROW_FIELDS + ("deesser_gain_reduction_db",)
ROW_DTYPE = np.dtype([(name, "<u8" if name == "true_peak_limited_events" else "<f4") for name in ROW_FIELDS])

_INT_SETTERS = {"compressor_set_adaptive_release", "compressor_set_auto_makeup_enabled",
                "compressor_set_sidechain_highpass_enabled", "deesser_set_auto_enabled"}


def apply_to_chain(chain: O.Chain, name: str, args) -> None:
    """One engine-named setter on the live oracle chain."""
    L = chain.L
    if name == "eq_set_band_config":
        band, (kind, freq, gain, q, slope, enabled) = args
        cfg = O.EqBandConfig(O.EQ_TYPE_IDS[kind], float(freq), float(gain), float(q), int(slope), int(bool(enabled)))
        L.afo_eq_set_band_config(chain.eq, int(band), C.byref(cfg))
    elif name.startswith("eq_set_band_"):
        band, value = args
        getattr(L, "afo_" + name)(chain.eq, int(band), float(value))
    elif name == "true_peak_limiter_set_release_ms":
        L.afo_tp_limiter_set_release_ms(chain.tp_limiter, float(np.float32(args[0])))
    elif name.split("_set_")[0] in ("compressor", "limiter", "deesser"):
        target = getattr(chain, name.split("_set_")[0])
        value = int(args[0]) if name in _INT_SETTERS else float(args[0])
        getattr(L, "afo_" + name)(target, value)
    else:
        raise KeyError(name)


def apply_to_engine(engine, name: str, args) -> None:
    """The same setter on a `mic_eq_mi` Engine."""
    if name == "eq_set_band_config":
        engine.eq_set_band_config_tuple(int(args[0]), tuple(args[1]))
    elif name in _INT_SETTERS:
        getattr(engine, name)(int(args[0]))
    else:
        getattr(engine, name)(*args)


def make_chain(sample_rate: float, bands, settings: dict | None, deesser: dict | None = None) -> O.Chain:
    """`chain_oracle.make_chain`, plus the de-esser configured as tests/test_gpu_deesser.py configures it:
    `deesser = {"eq_first": bool, "setters": [(engine setter name, args), ...]}`."""
    chain = CO.make_chain(sample_rate, bands, settings)
    if deesser is not None:
        chain.set("deesser_enabled", 1)
        chain.set("eq_before_deesser", int(bool(deesser.get("eq_first", False))))
        for name, args in deesser.get("setters", ()):
            apply_to_chain(chain, name, args)
    return chain


def run_calls(x: np.ndarray, sample_rate: float, bands, settings: dict | None, calls, schedule: dict | None = None,
              clamp: bool = False, deesser: dict | None = None):
    """One stream through the chain in calls of the given lengths, retuned by `schedule`: (output float32, rows [blocks])."""
    chain = make_chain(sample_rate, bands, settings, deesser)
    y = CO.sanitize(x, clamp)
    cb = CO.control_block(sample_rate)
    rows = []
    at = 0
    pending = []
    for index, length in enumerate(calls):
        pending += list((schedule or {}).get(index, ()))
        if length > 0:  # (a call that processes nothing leaves its setters pending for the next one that does)
            for name, args in pending:
                apply_to_chain(chain, name, args)
            pending = []
        for b0 in range(at, at + length, cb):
            block = y[b0 : min(b0 + cb, at + length)]
            st = chain.process_block(block)
            rows.append(tuple(getattr(st, name) for name in ROW_FIELDS))
        at += length
    return y[:at], np.array(rows, dtype=ROW_DTYPE)


def run_batch(audio: np.ndarray, sample_rate: float, bands, settings: dict | None, calls, schedule: dict | None = None,
              clamp: bool = False, deesser: dict | None = None, workers: int = 16):
    """run_calls over every stream of [n_streams, n] on up to `workers` threads.
    Returns (output [n_streams, sum(calls)], rows [blocks, n_streams])."""
    CO._lib()  # (loaded, and its signatures set, before the threads start)
    n_streams = audio.shape[0]
    out = np.empty((n_streams, int(sum(calls))), dtype=np.float32)
    rows = [None] * n_streams

    def one(s):
        out[s], rows[s] = run_calls(audio[s], sample_rate, bands, settings, calls, schedule, clamp, deesser)

    with ThreadPoolExecutor(max_workers=max(1, min(workers, n_streams))) as pool:
        list(pool.map(one, range(n_streams)))
    return out, np.stack(rows, axis=1)
