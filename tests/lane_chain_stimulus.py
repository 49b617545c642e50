"""Stimulus of the lane chain tests: seeded noise-plus-tone-burst streams whose levels are spread so that the compressor, the
limiter and the true-peak limiter all engage on some streams and on none of others, and one settings dict and band list per
stream from a fixed seed.  Together the settings cover: side chain on and off, adaptive release on and off, non-zero makeup
gains, the EQ off on some streams, the compressor off on some, the limiter stage off on some, ceilings above and below -1.5 dB
with careful output on and off, and different limiter releases."""
from __future__ import annotations

import numpy as np

FS = 48_000
N_STREAMS = 70  # one full wave and a wave of six lanes
N = 7_300
# a one-sample call, a call that ends inside the 72-sample crossfade, calls that end inside a van-Herk block of 97, short and
# long final blocks (the control block is 960)
CALLS = (1, 63, 8, 900, 960, 1921, 1000, N - (1 + 63 + 8 + 900 + 960 + 1921 + 1000))

MAKEUPS = (0.0, 2.5, -1.5, 4.0)
CEILINGS = (-0.3, -1.0, -1.5, -3.0, -6.0)
LIMITER_RELEASES = (20.0, 50.0, 80.0, 150.0)


def eq_on(i: int) -> bool:
    return i % 9 != 4


def compressor_on(i: int) -> bool:
    return i % 7 != 2


def limiter_on(i: int) -> bool:
    return i % 5 != 3


def audio(n_streams: int = N_STREAMS, n: int = N, fs: int = FS, seed: int = 2024) -> np.ndarray:
    """[n_streams, n] float32: white noise under a slow envelope plus Hann-windowed tone bursts, peak from 0.02 to 2.5; a
    stream whose limiter stage is off stays below 0.5, so that its output keeps the resolution the oracle bounds assume."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    out = np.empty((n_streams, n), dtype=np.float32)
    for i in range(n_streams):
        level = 0.02 * (2.5 / 0.02) ** (((i * 37) % n_streams) / max(n_streams - 1, 1))
        if not limiter_on(i):
            level = min(level, 0.5)
        x = 0.25 * rng.standard_normal(n) * (0.6 + 0.4 * np.sin(2 * np.pi * (1.0 + 0.1 * i) * t + i))
        period = int(fs * (0.021 + 0.002 * (i % 5)))
        length = int(fs * 0.008)
        burst = np.hanning(length) * np.sin(2 * np.pi * (300.0 + 170.0 * (i % 11)) * np.arange(length) / fs)
        for start in range((i * 131) % period, n - length, period):
            x[start : start + length] += 0.75 * burst
        out[i] = (level * x / np.max(np.abs(x))).astype(np.float32)
    return out


def bands(i: int, seed: int = 7) -> list:
    rng = np.random.default_rng(seed * 1000 + i)
    return [(float(80.0 * 1.75**k * rng.uniform(0.9, 1.1)), float(rng.uniform(-6.0, 6.0)), float(rng.uniform(0.6, 2.0))) for k in range(10)]


def settings(i: int, seed: int = 7, lookahead_ms: float = 2.0) -> dict:
    """Stream i's settings dict, in simulate_auto_eq_chain's keys plus ``eq_enabled`` (the processor's own switch)."""
    rng = np.random.default_rng(seed * 1000 + 500 + i)
    return {
        "eq_enabled": eq_on(i),
        "compressor_enabled": compressor_on(i),
        "compressor_threshold_db": float(rng.uniform(-40.0, -10.0)),
        "compressor_ratio": float(rng.uniform(1.5, 8.0)),
        "compressor_attack_ms": float(rng.uniform(1.0, 30.0)),
        "compressor_release_ms": float(rng.uniform(40.0, 400.0)),
        "compressor_makeup_gain_db": MAKEUPS[i % 4],
        "compressor_adaptive_release": bool(i % 3 == 1),
        "compressor_base_release_ms": float(rng.uniform(30.0, 120.0)),
        "compressor_auto_makeup_enabled": False,
        "compressor_sidechain_highpass_enabled": bool(i % 2 == 0),
        "limiter_enabled": limiter_on(i),
        "limiter_ceiling_db": CEILINGS[i % 5 if limiter_on(i) else (i // 5) % 5],
        "limiter_careful_output_enabled": bool((i // 2) % 2 == 0),
        "limiter_release_ms": LIMITER_RELEASES[(i // 3) % 4],
        "limiter_lookahead_ms": float(lookahead_ms),
    }


def engine_settings(st: dict) -> dict:
    """What configure_auto_eq_chain and the oracle take: the dict without the processor's own EQ switch."""
    return {k: v for k, v in st.items() if k != "eq_enabled"}
