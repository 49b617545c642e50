"""Stimulus of the compressor candidate sweep tests: three 1 s captures with a 333-sample tail (the last control block is
partial), their chain settings, and 50 + 16 candidates per capture shaped like the two phases of the reference's calibration
search (python/mic_eq/analysis/voice_setup.py:699-1079): the incumbent, a threshold grid and scattered four-control points,
then local steps around one of them."""
from __future__ import annotations

import numpy as np

import signals as S

FS = 48_000
N = 48_333
PHASE_1, PHASE_2 = 50, 16
BANDS = [(80.0, -2.0, 1.0), (140.0, 1.5, 1.0), (245.0, 0.0, 1.0), (428.75, -1.0, 1.2), (750.3125, 0.5, 1.0), (1313.046875, 0.0, 1.0),
         (2297.83203125, 2.0, 0.9), (4021.2060546875, 3.0, 1.0), (7037.110595703125, 1.0, 1.0), (12314.943542480469, -1.5, 1.0)]
# per capture: level, the incumbent (threshold, ratio, attack, release) and what the candidates leave alone
INCUMBENTS = [(-24.0, 4.5, 5.0, 100.0), (-24.0, 2.0, 20.0, 300.0), (-18.0, 5.5, 4.0, 120.0)]
LEVELS = (1.0, 0.3, 2.2)
SETTINGS = [
    {"compressor_sidechain_highpass_enabled": True, "compressor_adaptive_release": False, "compressor_makeup_gain_db": 0.0},
    {"compressor_sidechain_highpass_enabled": False, "compressor_adaptive_release": True, "compressor_base_release_ms": 80.0,
     "compressor_makeup_gain_db": 2.5, "deesser_enabled": True, "deesser_auto_amount": 0.7},
    {"compressor_sidechain_highpass_enabled": True, "compressor_adaptive_release": True, "compressor_makeup_gain_db": -1.0},
]
LIMITER = {"limiter_enabled": True, "limiter_ceiling_db": -1.5, "limiter_release_ms": 80.0, "limiter_careful_output_enabled": True,
           "limiter_lookahead_ms": 2.0}


def captures() -> np.ndarray:
    out = np.empty((len(LEVELS), N), dtype=np.float32)
    for i, level in enumerate(LEVELS):
        state, f0, phrase = S.stream_params(3 * i)
        x = level * S.kat_signal(-(-N // 480), state, f0, phrase)[:N].astype(np.float64)
        if i > 0:  # pauses: capture 0 has no block 6 dB over its 20 % level (the fold's all-blocks fallback), the others do
            t = np.arange(N) / FS
            x[((t >= 0.15) & (t < 0.35)) | ((t >= 0.70) & (t < 0.82))] *= 0.02
        if i == 2:  # ... and digital silence: blocks that are not audible
            x[int(0.72 * FS) : int(0.80 * FS)] = 0.0
        out[i] = x.astype(np.float32)
    return out


def chain_settings(capture: int, candidate=None) -> dict:
    """The settings dict simulate_auto_eq_chain takes for one capture (with one candidate's four controls)."""
    d = dict(LIMITER)
    d.update(SETTINGS[capture])
    d["compressor_enabled"] = True
    d["compressor_auto_makeup_enabled"] = False
    threshold, ratio, attack, release = candidate if candidate is not None else INCUMBENTS[capture]
    d.update(compressor_threshold_db=float(threshold), compressor_ratio=float(ratio), compressor_attack_ms=float(attack),
             compressor_release_ms=float(release))
    return d


def candidates(capture: int) -> list:
    """PHASE_1 + PHASE_2 (threshold, ratio, attack, release) tuples of one capture."""
    rng = np.random.default_rng(100 + capture)
    threshold, ratio, attack, release = INCUMBENTS[capture]
    out = [INCUMBENTS[capture]]
    out += [(float(t), ratio, attack, release) for t in np.linspace(-55.0, -6.0, 33)]
    while len(out) < PHASE_1:
        out.append((float(rng.uniform(-55.0, -6.0)), float(rng.uniform(1.5, 8.0)), float(rng.uniform(1.0, 30.0)), float(rng.uniform(40.0, 400.0))))
    seed = out[PHASE_1 - 3]
    for k in range(PHASE_2):
        step = [0.0, 0.0, 0.0, 0.0]
        step[k % 4] = (1.0, 0.25, 1.5, 20.0)[k % 4] * (1 if (k // 4) % 2 == 0 else -1) * (1 + k // 8)
        out.append(tuple(float(max(lo, v + s)) for v, s, lo in zip(seed, step, (-55.0, 1.0, 0.1, 5.0))))
    return out


def lanes() -> list:
    """(capture, threshold, ratio, attack, release) for every capture: phase 1 of all captures, then phase 2 of all."""
    per_capture = [candidates(c) for c in range(len(LEVELS))]
    out = [(c, *cand) for c in range(len(LEVELS)) for cand in per_capture[c][:PHASE_1]]
    out += [(c, *cand) for c in range(len(LEVELS)) for cand in per_capture[c][PHASE_1:]]
    return out
