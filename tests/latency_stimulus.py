"""Seeded recordings for the latency calibration (tests/test_latency_*.py, tests/test_gpu_latency_*.py): a Barker-coded probe
delayed into a noise floor of about -60 dBFS, with the faults a real route adds.  CASES holds one recording per property;
batch() repeats them with other seeds and ragged lengths, 70 streams in a shuffled order.  tools/gen_golden_latency.py runs the
reference on exactly these and writes tests/golden/latency_calibration.npz."""
from __future__ import annotations

import pathlib

import numpy as np

import latency_oracle as LO

LONG, SHORT = 33_600, 4_200  # 0.7 s at 48 kHz: a 65536-point PHAT transform (four-step form); 4200: 8192 points (LDS form)
NOISE = 1e-3                 # about -60 dBFS
RATES = (48_000, 16_000, 44_100, 96_000)
PROBE_MS = {48_000: 80.0, 16_000: 40.0, 44_100: 80.0, 96_000: 80.0}  # 40 ms at 16 kHz: the chip length has to shrink (:84-89)
BATCH = 70
GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "latency_calibration.npz"


def probe(rate=48_000):
    return LO.generate_probe_signal(rate, PROBE_MS[rate])


def record(rate, n, seed, delay=None, gain=0.5, taps=(), dc=0.0, noise=NOISE, nan_at=None, fade_after=None):
    """`gain` x probe at `delay`, further (delay offset, gain) `taps`, all cut at the end of the recording; `fade_after`: the probe
    drops by 180 dB from that sample of it on"""
    rng = np.random.default_rng(seed)
    x = noise * rng.standard_normal(n) + dc
    p = probe(rate).astype(np.float64)
    if fade_after is not None:
        p[fade_after:] *= 1e-9
    if delay is not None:
        for d, g in ((0, gain),) + tuple(taps):
            at = delay + d
            m = max(0, min(p.size, n - at))
            x[at : at + m] += g * p[:m]
    x = x.astype(np.float32)
    if nan_at is not None:
        x[nan_at] = np.nan
    return x


# name -> (rate, recording keywords, analysis keywords)
CASES = {
    "clean_long": (48_000, dict(n=LONG, seed=1, delay=2400), {}),
    "clean_short": (48_000, dict(n=SHORT, seed=2, delay=300), {}),
    "fractional": (48_000, dict(n=LONG, seed=3, delay=3001, gain=0.3, taps=((1, 0.2),)), {}),
    "dc_offset": (48_000, dict(n=LONG, seed=4, delay=1777, dc=0.1), {}),
    "weak_echo": (48_000, dict(n=LONG, seed=5, delay=2000, taps=((100, 0.15),)), {}),
    "strong_echo": (48_000, dict(n=LONG, seed=6, delay=2000, taps=((200, 0.49),)), {}),
    # a floor of -180 dBFS and a probe that fades out after its second burst: the windows of the last two are under the 1e-12 clamp
    "weak_probe": (48_000, dict(n=LONG, seed=7, delay=2500, noise=1e-9, fade_after=2000), {}),
    "cut_probe": (48_000, dict(n=LONG, seed=8, delay=LONG - 3000), {"max_search_ms": 700.0}),
    "noise_only": (48_000, dict(n=LONG, seed=9), {}),
    "silence": (48_000, dict(n=LONG, seed=10, noise=0.0), {}),
    "equal_size": (48_000, dict(n=3840, seed=11, delay=0), {}),
    "too_short": (48_000, dict(n=2000, seed=12, delay=0), {}),
    "expected_window": (48_000, dict(n=LONG, seed=13, delay=2400),
                        dict(expected_playback_start_ms=20.0, expected_playback_jitter_ms=5.0, expected_latency_min_ms=5.0,
                             expected_latency_max_ms=100.0)),
    "bad_window": (48_000, dict(n=SHORT, seed=14, delay=300), dict(max_search_ms=4.0)),
    "bad_route": (48_000, dict(n=SHORT, seed=15, delay=300), dict(route_kind="input_to_output")),
    "non_finite": (48_000, dict(n=SHORT, seed=16, delay=300, nan_at=1234), {}),
    "rate_16k": (16_000, dict(n=3000, seed=17, delay=400), {}),
    "rate_44k": (44_100, dict(n=8000, seed=18, delay=1000), {}),
    "rate_96k": (96_000, dict(n=66_000, seed=19, delay=5000), {}),
}
SCORE_CASES = ("clean_long", "clean_short")  # the golden file holds the reference's score arrays of these
EXACT = ("silence",)                         # every sum is exactly 0 in both arithmetics


def recording(name):
    rate, kw, _ = CASES[name]
    return record(rate, **kw)


def batch():
    """-> (recorded [70][LONG] float32, lengths [70], per-stream analysis keywords as a dict of lists).  48 kHz."""
    rng = np.random.default_rng(2024)
    names = [n for n, (rate, _, kw) in CASES.items() if rate == 48_000 and set(kw) <= {"max_search_ms"}]
    rows, lengths, max_ms = [], [], []
    for i in range(BATCH):
        name = names[i % len(names)]
        _, kw, akw = CASES[name]
        kw = dict(kw, seed=2000 + i)
        if kw["n"] == LONG and name != "cut_probe":
            kw["n"] = LONG - int(rng.integers(0, 4000))
        rows.append(record(48_000, **kw))
        lengths.append(kw["n"])
        max_ms.append(akw.get("max_search_ms", 500.0))
    order = rng.permutation(BATCH)
    out = np.zeros((BATCH, LONG), dtype=np.float32)
    for to, src in enumerate(order):
        out[to, : lengths[src]] = rows[src]
    return out, np.asarray(lengths, dtype=np.int64)[order], {"max_search_ms": [max_ms[s] for s in order]}
