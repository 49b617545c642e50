"""The seeded stereo batch the mixdown is tested on: 67 streams (one 64-lane group and a tail of 3), each with material of its
own so that neighbouring lanes of the decision pass decide differently, pushed as the callback sequence CALLBACKS.

The sequence is 1, 2, 3, 5, 16, 17, 128, 480, 1000 frames, then one call of 8192 + 5 frames (the callback wrapper cuts it
into a full chunk and a 5-frame chunk in which only |lag| <= 2 has the 3 overlapping frames a correlation needs), then
four short callbacks of 2, 3, 1 and 4 frames.  The tail is there for one hysteresis edge: a chunk with a correlation
below -0.75 in which nothing is detected.  delayed_correlation(0, -1) is the exact negation of the stereo correlation, so
with 3 frames or more a correlation below -0.75 is always detected (as a polarity flip at the least); a stored candidate
can only be *reused* in a chunk shorter than 3 frames that follows a detection, and the head of the sequence has its two
such chunks before any candidate exists.

Families (FAMILIES[s] names the family of stream s; the order is shuffled so that neighbours differ):
  coherent        right = g * left (+ a little noise): no rescue, plain average
  antiphase       right = -g * left: polarity flip; max-RMS fallback in the 1- and 2-frame callbacks
  delay+N/delay-N right (or left) delayed by N = 1..8 frames: fractional-delay rescue, best_delay = +-8 at N = 8
  frac            right delayed by 3.4 / 5.35 frames, a sum of sines
  anti_delay      right = -left delayed: polarity -1 with a delay
  noise           independent channels
  hyst_reuse      antiphase all the way: the tail alternates undetectable / detectable below -0.75
  hyst_clear      a rescue that the material then stops needing: the stored candidate is cleared
  silence         zeros
  tiny            amplitudes of 1e-20 (denormal products) and around the EPSILON bound of the denominators
  negzero         frames of -0.0 (Average and the phase-safe average differ in the sign of zero there)
  tie             period-4 square waves: several lags reach a correlation of exactly 1.0, the first one must win
"""
from __future__ import annotations

import numpy as np

SEED = 20240611
N_STREAMS = 67
HEAD = (1, 2, 3, 5, 16, 17, 128, 480, 1000, 8192 + 5)
TAIL = (2, 3, 1, 4)
CALLBACKS = HEAD + TAIL
N_FRAMES = sum(CALLBACKS)
TAIL_START = sum(HEAD)
F = np.float32


def _noise(rng, n, amp=0.3):
    return (rng.standard_normal(n) * amp).astype(F)


def _shift(x, d):
    """x delayed by d >= 0 frames, zeros in front"""
    y = np.zeros_like(x)
    if d == 0:
        y[:] = x
    else:
        y[d:] = x[:-d]
    return y


def _sines(n, delay, rng):
    freqs = np.array([3100.0, 9100.0, 15000.0]) * (1.0 + 0.1 * rng.random(3))
    amps = np.array([0.22, 0.16, 0.09])
    t = (np.arange(n, dtype=np.float64) - delay) / 48_000.0
    return (amps[:, None] * np.sin(2.0 * np.pi * freqs[:, None] * t[None, :])).sum(0).astype(F)


def _family_list():
    fam = []
    fam += [("coherent", k) for k in range(5)]
    fam += [("antiphase", k) for k in range(5)]
    fam += [(f"delay+{d}", d) for d in range(1, 9)]
    fam += [(f"delay-{d}", -d) for d in range(1, 9)]
    fam += [("frac", 3.4), ("frac", 5.35), ("frac", -3.4), ("frac", -5.35), ("frac", 0.6), ("frac", 7.5)]
    fam += [("anti_delay", d) for d in (1, 2, 5, 8, -3, -8)]
    fam += [("noise", k) for k in range(7)]
    fam += [("hyst_reuse", k) for k in range(4)]
    fam += [("hyst_clear", k) for k in range(4)]
    fam += [("silence", 0), ("silence", 1)]
    fam += [("tiny", k) for k in range(5)]
    fam += [("negzero", k) for k in range(4)]
    fam += [("tie", k) for k in range(3)]
    assert len(fam) == N_STREAMS, len(fam)
    order = np.random.default_rng(SEED).permutation(N_STREAMS)
    return [fam[i] for i in order]


_FAMILY = _family_list()
FAMILIES = [f for f, _ in _FAMILY]


def _stream(s):
    name, p = _FAMILY[s]
    rng = np.random.default_rng(SEED + 1000 + s)
    n = N_FRAMES
    left = _noise(rng, n, 0.1 + 0.4 * rng.random())
    if name == "coherent":
        right = (left * F(0.5 + 0.25 * p)).astype(F) + _noise(rng, n, 0.002 * p)
    elif name == "antiphase":
        right = (-left * F(0.5 + 0.25 * p)).astype(F)
    elif name.startswith("delay"):
        d = abs(p)
        if p > 0:
            right = _shift(left, d)
        else:
            right = left.copy()
            left = _shift(right, d)
        right = right + _noise(rng, n, 0.01)
    elif name == "frac":
        left = _sines(n, max(0.0, -p), rng)
        rng = np.random.default_rng(SEED + 1000 + s)  # the same frequencies for the other side
        right = _sines(n, max(0.0, p), rng)
    elif name == "anti_delay":
        d = abs(p)
        if p > 0:
            right = (-_shift(left, d)).astype(F)
        else:
            right = (-left).astype(F)
            left = _shift(left, d)
    elif name == "noise":
        right = _noise(rng, n, 0.3)
    elif name == "hyst_reuse":
        right = (-left * F(1.0 - 0.1 * p)).astype(F)
    elif name == "hyst_clear":
        # a rescue first, then material that needs none: at a callback boundary inside the head (p = 0..2) or in the
        # 2-frame callback of the tail (p = 3), where a candidate is stored and the correlation is +1
        cut = (sum(HEAD[:7]), sum(HEAD[:8]), sum(HEAD[:9]), TAIL_START)[p]
        right = (-left).astype(F) if p % 2 else _shift(left, 4)
        right[cut:] = left[cut:]
    elif name == "silence":
        left = np.zeros(n, dtype=F)
        right = np.zeros(n, dtype=F)
        if p == 1:  # silence with one callback of signal in the middle
            a, b = sum(HEAD[:6]), sum(HEAD[:7])
            left[a:b] = _noise(rng, b - a, 0.2)
            right[a:b] = -left[a:b]
    elif name == "tiny":
        scale = (1e-20, 1e-20, 2.0e-4, 3.0e-4, 1.5e-4)[p]
        left = (rng.standard_normal(n) * scale).astype(F)
        right = {0: left.copy(), 1: (-left).astype(F), 2: _shift(left, 2), 3: (-left).astype(F), 4: left.copy()}[p]
    elif name == "negzero":
        if p == 0:  # nothing but -0.0
            left = np.full(n, -0.0, dtype=F)
            right = np.full(n, -0.0, dtype=F)
        else:  # coherent (p = 1), antiphase (2) or delayed (3) material with runs of -0.0 frames in both channels
            right = {1: left.copy(), 2: (-left).astype(F), 3: _shift(left, 3)}[p]
            holes = rng.random(n) < 0.3
            holes[:6] = True
            left[holes] = -0.0
            right[holes] = -0.0
    elif name == "tie":
        sq = np.where((np.arange(n) // 2) % 2 == 0, 0.5, -0.5).astype(F)  # + + - - : period 4
        left = sq
        # 0: right = left (lags -8, -4, 0, 4, 8 tie at +1, and -6, -2, 2, 6 with polarity -1): nothing to rescue
        # 1: right = left two frames late = -left: lags -6, -2, 2, 6 tie at exactly 1.0; -6 is first
        # 2: the same at another amplitude, one frame late: lags -7, -3, 1, 5
        right = {0: sq.copy(), 1: np.roll(sq, 2), 2: (np.roll(sq, 1) * F(0.25)).astype(F)}[p]
    else:  # pragma: no cover
        raise AssertionError(name)
    return np.stack([left.astype(F), right.astype(F)], axis=1)


_BATCH = None


def batch() -> np.ndarray:
    """[N_STREAMS, N_FRAMES, 2] float32; built once, shared and read-only."""
    global _BATCH
    if _BATCH is None:
        b = np.stack([_stream(s) for s in range(N_STREAMS)])
        b.setflags(write=False)
        _BATCH = b
    return _BATCH


def callbacks(x: np.ndarray | None = None):
    """The batch cut into its callbacks: a list of [streams, frames, channels] views."""
    x = batch() if x is None else x
    out, at = [], 0
    for n in CALLBACKS:
        out.append(x[:, at:at + n])
        at += n
    return out


def multichannel(channels: int) -> np.ndarray:
    """[N_STREAMS, N_FRAMES, channels]: the stereo material spread over `channels` with per-channel gains and a little
    noise of its own, so that the strongest channel differs between streams and between callbacks."""
    x = batch()
    rng = np.random.default_rng(SEED + 77 + channels)
    out = np.empty((N_STREAMS, N_FRAMES, channels), dtype=F)
    for c in range(channels):
        gain = (0.25 + rng.random((N_STREAMS, 1))).astype(F)
        src = x[:, :, c % 2]
        out[:, :, c] = src * gain + (rng.standard_normal(src.shape) * 0.01).astype(F) * (c >= 2)
    # the loudest channel changes over time: swap two channels' halves in every other stream
    if channels >= 2:
        half = N_FRAMES // 2
        out[::2, half:, [0, channels - 1]] = out[::2, half:, [channels - 1, 0]]
    out.setflags(write=False)
    return out


_REFERENCE = {}


def reference(channels: int, mode: int):
    """The restatement on the batch, callback by callback: (list of mono [streams, frames] per callback, list of the
    diagnostics dict after each callback, per-stream branch counters).  Computed once per (channels, mode)."""
    key = (channels, mode)
    if key not in _REFERENCE:
        import mixdown_oracle as MO

        x = batch() if channels == 2 else (batch()[:, :, :1] if channels == 1 else multichannel(channels))
        b = MO.Batch(channels, mode, N_STREAMS)
        outs, diags = [], []
        for cb in callbacks(x):
            outs.append(b.push(cb))
            diags.append(b.diagnostics())
        _REFERENCE[key] = (outs, diags, b.counters())
    return _REFERENCE[key]


def material(channels: int) -> np.ndarray:
    return batch() if channels == 2 else (batch()[:, :, :1] if channels == 1 else multichannel(channels))
