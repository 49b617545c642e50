"""High-precision references for tests/test_gpu_device_math.py: mpmath at 45 significant digits, error in units in the last
place of the correctly rounded f64 result.  Module-level functions so that a spawned worker process can import them."""
from __future__ import annotations

import mpmath
import numpy as np

DPS = 45


def _ulps(dev: float, exact) -> float:
    """|dev - exact| in ulps of the f64 nearest `exact` (an mpf)."""
    if exact == 0:
        return 0.0 if dev == 0.0 else float("inf")
    nearest = float(exact)
    ulp = np.spacing(np.float64(abs(nearest)))
    return float(abs(mpmath.mpf(dev) - exact) / mpmath.mpf(float(ulp)))


def log10_ulps(chunk):
    """chunk = (x, device fast_log10_pos(x)) arrays -> ulp errors."""
    mpmath.mp.dps = DPS
    x, dev = chunk
    return np.array([_ulps(float(d), mpmath.log10(mpmath.mpf(float(v)))) for v, d in zip(x, dev)])


def exp10_ulps(chunk):
    """chunk = (y, device exp10(y)) arrays -> ulp errors."""
    mpmath.mp.dps = DPS
    y, dev = chunk
    return np.array([_ulps(float(d), mpmath.power(10, mpmath.mpf(float(v)))) for v, d in zip(y, dev)])


def f1_reference(chunk):
    """chunk = (g, thr) -> the gated pre-pass's F1 gain by the same f64 steps with correctly rounded log10 and 10^x:
    level = 20 * log10(max(sqrt(g), 1e-10)); d = clamp((thr - level) * 0.75, 0, 36); 10^(-d / 20).  Returns (level, gain) as
    f64 plus the exact 10^(-d / 20) as strings (for the ulp comparison in the parent)."""
    mpmath.mp.dps = DPS
    g, thrs = chunk
    thr = float(thrs[0]) if len(thrs) else 0.0
    levels, gains = np.empty(len(g)), np.empty(len(g))
    for i, v in enumerate(g):
        s = max(abs(float(np.sqrt(np.float64(v)))), 1e-10)
        level = 20.0 * float(mpmath.log10(mpmath.mpf(s)))
        d = min(max((thr - level) * (1.0 - 1.0 / 4.0), 0.0), 36.0)
        levels[i] = level
        gains[i] = float(mpmath.power(10, mpmath.mpf(-d / 20.0)))
    return levels, gains
