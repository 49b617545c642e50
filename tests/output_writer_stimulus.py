"""The push sequences the output-writer tests share: block lengths around every tile edge, per-stream queue fills that put
expand / pass-through / compress / emergency / short-write / zero-free streams into the same launch, a fade that straddles
several pushes, input that reaches every safety branch, and the live toggles.  Deterministic; no GPU, no library."""
from __future__ import annotations

import numpy as np

N_STREAMS = 67  # one wave plus three
LENGTHS = (480, 1, 2, 5, 63, 64, 65, 256, 480, 1024, 8191, 8192, 480, 33, 480, 7, 480, 19, 300, 480)

# name -> (rate, capacity, centre, hard backlog, fade); None: derived from the rate (dsp_loop.rs:781-795)
CONFIGS = {
    "derived_48k": (48_000, None, None, None, None),
    "limits_4_8_4": (48_000, 8, 4, 8, 4),          # tests.rs:1429, the queue of :1386
    "limits_128_256_4": (48_000, 1024, 128, 256, 4),  # tests.rs:1308, the queue of :1266
    "one_frame_queue": (48_000, 1, 1, 2, 2),       # every retimed block comes out one frame long (resampling.rs:106-107)
}


def limits(name: str) -> dict:
    rate, cap, center, hard, fade = CONFIGS[name]
    if cap is None:
        low, high = (rate * 30 + 500) // 1000, (rate * 40 + 500) // 1000
        cap, center, hard, fade = 2 * rate, (low + high + 1) // 2, (rate * 60 + 500) // 1000, max((rate * 6 + 500) // 1000, 1)
    return dict(rate=rate, capacity=cap, center=center, hard=hard, fade=fade)


def _fills(k: int, lim: dict, rng: np.random.Generator) -> np.ndarray:
    cap, center, hard = lim["capacity"], lim["center"], lim["hard"]
    f = np.zeros(N_STREAMS, dtype=np.int64)
    for s in range(N_STREAMS):
        role = s % 8
        if role == 0:
            v = center                                   # no error: ratio 1, pass-through
        elif role == 1:
            v = 0                                        # starved: expands
        elif role == 2:
            v = max(hard - 1, 0)                         # backlog below the hard limit: compresses
        elif role == 3:
            v = min(hard + s, cap)                       # emergency ratio
        elif role == 4:
            v = max(cap - 1 - (s // 8), 0) if k % 2 == 0 else center   # short write, then a fade across the next pushes
        elif role == 5:
            v = cap if k % 3 == 0 else min(center + 1, cap)            # no free space at all
        elif role == 6:
            v = (center + (k * 37 + s * 11) % (2 * max(hard, 1))) % (cap + 1)   # drifts up and down
        else:
            v = int(rng.integers(0, cap + 1))
        f[s] = min(max(v, 0), cap)
    return f


def _audio(k: int, n: int, rng: np.random.Generator) -> np.ndarray:
    t = np.arange(n, dtype=np.float64) + 1000.0 * k
    x = np.empty((N_STREAMS, n), dtype=np.float32)
    for s in range(N_STREAMS):
        tone = (0.45 + 0.005 * s) * np.sin(2 * np.pi * (400.0 + 37.0 * s) / 48_000.0 * t)
        x[s] = tone.astype(np.float32)
        kind = (s + k) % 6
        if kind == 1 and n >= 4:      # steps over any ceiling: limited events with the limiter on, clips with it off
            a = n // 3
            x[s, a:a + max(n // 8, 2)] = np.float32(1.5 if s % 2 else -1.75)
        elif kind == 2 and n >= 3:    # non-finite frames
            x[s, n // 2] = np.nan
            x[s, 0] = np.inf
            x[s, n - 1] = -np.inf
        elif kind == 3:               # a fade through the denormals
            x[s] = (x[s].astype(np.float64) * 1e-36 * np.exp(-np.arange(n) * (12.0 / max(n, 1)))).astype(np.float32)
        elif kind == 4:
            x[s] += rng.standard_normal(n).astype(np.float32) * np.float32(0.4)
    return x


def sequence(name: str, lengths=LENGTHS, seed: int = 2024):
    """Yields one dict per push: `pre` (actions on the writer before the push: ("limiter", enabled, ceiling) / ("reset",)),
    `x` [N_STREAMS, n], `fill` [N_STREAMS], `clean_path`."""
    lim = limits(name)
    rng = np.random.default_rng(seed)
    pushes = []
    for k, n in enumerate(lengths):
        pre = []
        if k == 5:
            pre.append(("limiter", False, 1.0))   # reset of the limiter; detector and limiter-output histories diverge
        if k == 8:
            pre.append(("limiter", True, 0.7))
        if k == 13:
            pre.append(("limiter", True, 0.25))   # a ceiling change
        if k == 15:
            pre.append(("reset",))
        if k == 16:
            pre.append(("limiter", False, 0.5))
        if k == 18:
            pre.append(("limiter", True, 1.0))
        fill = _fills(k, lim, rng)
        if k == 14:  # the ragged maximum at the last stream of a wave, one frame reaching the queue at its first
            fill[0] = max(lim["capacity"] - 1, 0)
            fill[63] = 0
        pushes.append(dict(pre=pre, x=_audio(k, n, rng), fill=fill, clean_path=k in (11, 12, 17)))
    return pushes


def apply_pre(writer, pre) -> None:
    """The same actions on a restatement Batch or on the library's OutputWriter."""
    for action in pre:
        if action[0] == "limiter":
            writer.set_limiter(action[1], action[2])
        else:
            writer.reset()
