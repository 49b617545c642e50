"""The committed stimulus of the VAD-fused gate tests: audio, per-stream evidence and the configurations both
tests/test_gate_vad_stimulus.py (restatement alone) and tests/test_gpu_gate_vad.py (device against restatement) run."""
from __future__ import annotations

import numpy as np

import vad_gate_oracle as V

FS = 48_000.0
N_STREAMS = 70
BLOCK = 500                      # control block: not a multiple of 32, nor of the 480-sample frame
CALLS = (70_250, 61_000)         # unequal, the first one ends inside a control block's worth of a tile
EDGE_DB = 1e-4                   # a stream within this of a bin edge / the level threshold may leave the discrete comparison
EDGE_CAP = 0.02

CONFIGS = {
    # name: (mode, controller settings)
    "assisted_auto_hold200": (V.VAD_ASSISTED, dict(V.DEFAULT_CONTROLLER)),
    "only_manual_hold0": (V.VAD_ONLY, dict(V.DEFAULT_CONTROLLER, hold_ms=0.0, auto_threshold=False, vad_threshold=0.5)),
    "assisted_auto_hold0": (V.VAD_ASSISTED, dict(V.DEFAULT_CONTROLLER, hold_ms=0.0, margin_db=6.0)),
    "only_auto_hold200": (V.VAD_ONLY, dict(V.DEFAULT_CONTROLLER, vad_threshold=0.4)),
}


def gate_params(mode, release_ms=100.0):
    return dict(threshold_db=-40.0, attack_ms=10.0, release_ms=release_ms, mode=mode)


def audio(n_streams=N_STREAMS, n=sum(CALLS), seed=11) -> np.ndarray:
    """Per stream (shifted and scaled differently): 0.4 s of talk, a quiet tail at about -44 dB (below the level threshold),
    a pause on a noise bed whose level steps up and later down (the noise floor follows both ways), 0.6 s of flutter."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    out = np.empty((n_streams, n), dtype=np.float32)
    for s in range(n_streams):
        f = 140.0 + 11.0 * (s % 19)
        tone = np.sin(2 * np.pi * f * t + 0.3 * s) + 0.3 * np.sin(2 * np.pi * 2.7 * f * t)
        ts = (t + 0.041 * s) % 1.3
        env = np.where(ts < 0.4, 0.22, np.where(ts < 0.55, 0.009, 0.0))
        flutter = np.where(((ts - 0.7) % 0.1) < 0.05, 0.06, 0.0)
        env = np.where(ts >= 0.7, flutter, env) * (0.7 + 0.05 * (s % 9))
        bed = np.where(t < 0.9, 6e-4, np.where(t < 1.9, 4e-3, 3e-4)) * (0.8 + 0.04 * (s % 7))
        out[s] = (env * tone + bed * rng.standard_normal(n)).astype(np.float32)
    return out


def evidence(calls=CALLS, block=BLOCK, n_streams=N_STREAMS, seed=5):
    """Per call (probabilities [blocks, n_streams] float32, available [blocks, n_streams] bool): the posterior follows each
    stream's talk spurts, lingers in the uncertain band over the quiet tail, toggles block by block during the flutter, and
    the worker drops out (not available) for a stretch of every stream."""
    rng = np.random.default_rng(seed)
    res, at = [], 0
    for c in calls:
        nb = (c + block - 1) // block
        tb = (at + (np.arange(nb) + 0.5) * block) / FS
        p = np.empty((nb, n_streams), dtype=np.float32)
        a = np.ones((nb, n_streams), dtype=bool)
        for s in range(n_streams):
            ts = (tb + 0.041 * s) % 1.3
            base = np.where(ts < 0.4, 0.92, np.where(ts < 0.55, 0.40, 0.04))
            tog = np.where((np.arange(nb) + s) % 2 == 0, 0.95, 0.0)
            q = np.where(ts >= 0.7, tog, base) + 0.03 * rng.standard_normal(nb)
            if s % 10 == 3:
                q = q * 0.25  # a stream the worker never hears speech in: every block feeds the noise-floor history
            p[:, s] = np.clip(q, -0.05, 1.05)  # (out-of-range values: the gate clamps them)
            lo = 0.35 + 0.02 * (s % 11)
            a[:, s] = ~((tb > lo) & (tb < lo + 0.25))
        res.append((p, a))
        at += c
    return res


def excluded(state) -> np.ndarray:
    """Streams the restatement reports within EDGE_DB of a bin edge or of the level threshold in some block."""
    return np.asarray(state["min_edge_distance_db"]) <= EDGE_DB
