"""Stimulus of the EQ headroom validation tests: ten captures of 19 533 samples at 48 kHz (20 control blocks of 960 and a
333-sample tail), each with the Auto-EQ settings and the nested chain settings that
python/mic_eq/analysis/auto_eq_parts/headroom.py:292-354 takes.  With the seven gain scales that is 70 lanes: one wave and six.

What each capture is there for (tests/test_headroom_stimulus.py asserts it on the reference's own results):
  0 quiet, mild EQ: safe at scale 1.0            5 all-zero gains (a setter that changes no gain)
  1, 2 boosted EQ: two different interior scales 6 its own limiter ceiling: a second sweep group
  3 hot input: still unsafe at scale 0.0         7 compressor disabled: the engine route
  4 de-esser on                                  8, 9 adaptive release with makeup; side chain off, cuts instead of boosts
"""
from __future__ import annotations

import numpy as np

import signals as S

FS = 48_000
N = 19_533
SCALES = (1.0, 0.85, 0.70, 0.55, 0.40, 0.25, 0.0)  # HEADROOM_SCALES, headroom.py:17
FREQS = [80.0, 160.0, 320.0, 640.0, 1280.0, 2500.0, 5000.0, 8000.0, 12000.0, 16000.0]
LEVELS = (0.25, 1.05, 1.3, 4.0, 0.9, 0.5, 0.8, 1.1, 1.0, 1.6)
GAINS = [
    [1.0, -1.0, 0.5, 0.0, -0.5, 1.0, 1.5, 0.5, 0.0, -1.0],
    [4.0, 3.0, 2.0, 1.0, 0.0, 3.0, 5.0, 4.0, 2.0, 1.0],
    [6.0, 5.0, 4.0, 3.0, 2.0, 4.0, 6.0, 5.0, 3.0, 2.0],
    [2.0, 1.0, 0.0, 0.0, 0.0, 1.0, 2.0, 1.0, 0.0, 0.0],
    [0.0, 1.0, 0.0, -1.0, 0.0, 2.0, 6.0, 6.0, 4.0, 2.0],
    [0.0] * 10,
    [3.0, 3.0, 3.0, 2.0, 2.0, 3.0, 4.0, 3.0, 2.0, 1.0],
    [5.0, 4.0, 3.0, 2.0, 1.0, 3.0, 5.0, 4.0, 2.0, 1.0],
    [3.0, 2.5, 2.0, 1.5, 1.0, 2.0, 3.5, 3.0, 1.5, 0.5],
    [-3.0, -2.0, -1.0, 0.0, 2.0, 3.0, 4.0, -2.0, -4.0, -6.0],
]
QS = [[1.41] * 10, [1.0] * 10, [0.8] * 10, [1.41] * 10, [1.2] * 10, [1.41] * 10, [1.0] * 10, [1.1] * 10, [0.9] * 10,
      [0.7, 1.0, 1.41, 2.0, 1.0, 0.9, 1.41, 3.0, 1.0, 0.8]]
# what an Auto-EQ result carries beside its bands (the validation multiplies / caps these)
EXTRAS = [{"validation_confidence": 0.9, "analysis_confidence": 0.8}, {"validation_confidence": 0.95, "analysis_confidence": 0.9},
          {"validation_gain_scale": 0.9, "validation_confidence": 0.6}, {"validation_confidence": 0.3, "analysis_confidence": 0.7},
          {}, {"analysis_confidence": 0.5}, {"validation_confidence": 0.8}, {}, {"validation_confidence": 0.7, "analysis_confidence": 0.55},
          {"apply_recommended": True}]
CHAINS = [
    None,
    {"compressor": {"threshold_db": -24.0, "ratio": 3.0, "makeup_gain_db": 3.0}},
    {"compressor": {"threshold_db": -22.0, "ratio": 2.5, "attack_ms": 8.0, "release_ms": 150.0, "makeup_gain_db": 2.0}},
    {"compressor": {"threshold_db": -12.0, "ratio": 2.0, "makeup_gain_db": 6.0}},
    {"deesser": {"enabled": True, "auto_amount": 0.7, "threshold_db": -34.0, "max_reduction_db": 8.0},
     "compressor": {"threshold_db": -24.0, "ratio": 3.0, "makeup_gain_db": 4.0}},
    {"compressor": {"threshold_db": -26.0, "ratio": 4.0, "makeup_gain_db": 9.0}},
    {"compressor": {"threshold_db": -24.0, "ratio": 3.0, "makeup_gain_db": 3.0},
     "limiter": {"ceiling_db": -3.0, "release_ms": 80.0}},
    {"compressor": {"enabled": False}},
    {"compressor": {"threshold_db": -26.0, "ratio": 3.5, "adaptive_release": True, "base_release_ms": 80.0, "makeup_gain_db": 4.0}},
    {"compressor": {"threshold_db": -20.0, "ratio": 2.0, "sidechain_highpass_enabled": False, "makeup_gain_db": 1.0},
     "limiter": {"careful_output_enabled": False, "ceiling_db": -1.0}},
]
N_CAPTURES = len(LEVELS)
assert len(GAINS) == len(QS) == len(EXTRAS) == len(CHAINS) == N_CAPTURES == 10


def captures() -> np.ndarray:
    out = np.empty((N_CAPTURES, N), dtype=np.float32)
    t = np.arange(N) / FS
    for i, level in enumerate(LEVELS):
        state, f0, phrase = S.stream_params(5 * i + 2)
        x = level * S.kat_signal(-(-N // 480), state, f0, phrase)[:N].astype(np.float64)
        x[(t >= 0.12) & (t < 0.20)] *= 0.03  # a pause: blocks under the active threshold
        out[i] = x.astype(np.float32)
    return out


def eq_settings(capture: int) -> dict:
    d = {"band_freqs": list(FREQS), "band_gains": list(GAINS[capture]), "band_qs": list(QS[capture])}
    d.update(EXTRAS[capture])
    return d


def all_eq_settings() -> list:
    return [eq_settings(c) for c in range(N_CAPTURES)]


def chain_settings(capture: int):
    return CHAINS[capture]


def all_chain_settings() -> list:
    return list(CHAINS)
