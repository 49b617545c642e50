"""Stimuli of the speech-feature tests at device rates: the recipe of tests/speech_features_stimulus.py (a noise floor, voiced
tone bursts below 4 kHz, broadband bursts between 5.5 and 8.5 kHz -- 5.2 to 7 kHz at 16 kHz, below its Nyquist -- at the end of
every voiced burst on two streams out of three, a room-noise capture and a track of speech posteriors) made at a given rate,
with the burst edges on that rate's 20 ms hop grid and a posterior per ceil(fs 512 / 16000) samples.

The main batch, at 16, 32, 44.1 and 96 kHz, has 67 streams (one past the 64-stream tile) of 170 hops + 123 samples: one
short-term window, a partial tail chunk, and a resampled length that is no multiple of 64 or 960.  The small batches, at
44.1 kHz, take the other paths: exactly one frame and twelve hops with a burst (no momentary window: the masked-energy
fallback, over no sample and over a resampled mask with both edges), one momentary window, no
posteriors, no noise capture, a noise capture below one frame, an all-zero stream and a stream with a NaN.  The tap batches, at
22.05, 24 and 88.2 kHz, are 3 streams of 1.1 s for the resampling stage alone.

Burst places are drawn per stream until no 0.4 s loudness window has exactly 11 of its 20 hops active, as at 48 kHz: the
resampled mask's edges lie within a sample of the hop edges, so a window there would sit on the 0.55 cut.
tools/gen_golden_speech_features_rates.py ran the reference over exactly these arrays and asserts the conditions with the
reference's own resampled mask.

Everything is a function of (batch, stream index): no state, no files."""
from __future__ import annotations

import functools
import pathlib

import numpy as np

from speech_features_stimulus import DC, FLOOR_DB, MARGIN, VOICED_DB, _amp, _layout, rms_db, sibilance_db  # noqa: F401
from voice_spectrum_stimulus import fingerprint  # noqa: F401

RATES = (16_000, 22_050, 24_000, 32_000, 44_100, 48_000, 88_200, 96_000)
MAIN_RATES = (16_000, 32_000, 44_100, 96_000)
TAP_RATES = (22_050, 24_000, 88_200)
SMALL_RATE = 44_100
MAIN_STREAMS, MAIN_HOPS, MAIN_EXTRA = 67, 170, 123


def hop(fs: int) -> int:
    return int(fs * 20 / 1000.0)


def frame(fs: int) -> int:
    return int(fs * 40 / 1000.0)


def vad_window(fs: int) -> int:
    return -(-fs * 512 // 16_000)


def frames(fs: int, n: int) -> int:
    return 0 if n < frame(fs) else (n - frame(fs)) // hop(fs) + 1


# name -> (rate, streams, speech samples, noise samples or 0, posteriors, kind of every stream or None for "voice")
BATCHES = {f"main_{fs}": (fs, MAIN_STREAMS, MAIN_HOPS * hop(fs) + MAIN_EXTRA, fs, True, None) for fs in MAIN_RATES}
BATCHES.update({
    "one_frame": (SMALL_RATE, 2, frame(SMALL_RATE), SMALL_RATE, False, None),
    "short": (SMALL_RATE, 3, 12 * hop(SMALL_RATE) + 57, SMALL_RATE, True, None),
    "one_window": (SMALL_RATE, 3, 20 * hop(SMALL_RATE), SMALL_RATE, True, None),
    "no_vad": (SMALL_RATE, 3, 100 * hop(SMALL_RATE), SMALL_RATE, False, None),
    "no_noise": (SMALL_RATE, 3, 100 * hop(SMALL_RATE), 0, True, None),
    "short_noise": (SMALL_RATE, 3, 100 * hop(SMALL_RATE), 1000, True, None),
    "special": (SMALL_RATE, 5, 50 * hop(SMALL_RATE), SMALL_RATE, False, ("voice", "all_zero", "steady", "nan", "voice")),
})
BATCHES.update({f"tap_{fs}": (fs, 3, 55 * hop(fs), 0, True, None) for fs in TAP_RATES})
ANALYZED = tuple(name for name in BATCHES if not name.startswith("tap_"))


def _band_noise(rng, fs: int, n: int, low: float, high: float) -> np.ndarray:
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / fs)
    X[(f < low) | (f > high)] = 0.0
    x = np.fft.irfft(X, n)
    return x / np.sqrt(np.mean(x * x))


def _components(seed: int, stream: int, fs: int, n: int):
    """What a stream is mixed from: the floor, a unit-RMS harmonic series and unit-RMS sibilant noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / fs
    f0 = 105.0 + 9.0 * (stream % 13)
    voiced = np.zeros(n)
    for h in range(1, 1 + min(16, int(3800.0 // f0))):
        voiced += np.sin(2.0 * np.pi * f0 * h * t + rng.uniform(0.0, 2.0 * np.pi)) / h ** (0.8 + 0.05 * (stream % 5))
    voiced /= np.sqrt(np.mean(voiced * voiced))
    low, high = (5500.0, 8500.0) if fs >= 22_050 else (5200.0, 7000.0)
    return rng.standard_normal(n) * _amp(FLOOR_DB), voiced, _band_noise(rng, fs, n, low, high)


def _voice(parts, seed: int, stream: int, fs: int, with_vad: bool):
    floor, voiced, hiss = parts
    n, H, W = floor.size, hop(fs), vad_window(fs)
    rng = np.random.default_rng(seed)
    C = -(-n // H)
    bursts = _layout(rng, n // H)
    env_v, env_s = np.zeros(C), np.zeros(C)
    for k0, k1, sib in bursts:
        env_v[k0:k1 - sib] = 1.0
        env_s[k1 - sib:k1] = 1.0
    env_v, env_s = np.repeat(env_v, H)[:n], np.repeat(env_s, H)[:n]
    level = sibilance_db(stream)
    x = floor + voiced * _amp(VOICED_DB) * env_v
    if level is None:
        x += voiced * _amp(VOICED_DB - 6.0) * env_s  # the burst goes on, quieter
    else:
        x += hiss * _amp(level) * env_s + voiced * _amp(VOICED_DB - 20.0) * env_s
    vad = None
    if with_vad:
        n_vad = -(-n // W)
        centres = (np.arange(n_vad) + 0.5) * W / H  # in hops
        vad = 0.04 + 0.1 * rng.random(n_vad)
        for k0, k1, sib in bursts:
            vad[(centres >= k0 - 1) & (centres < k1 - sib + 0.5)] = 0.8 + 0.15 * rng.random()
            vad[(centres >= k1 - sib + 0.5) & (centres < k1 + 1)] = 0.25 + 0.5 * rng.random()  # sibilants: often below 0.4
    return x + DC, vad


def _masked_window_counts(x: np.ndarray, fs: int, noise_rms_db: float, vad):
    """The number of active hops in every 0.4 s window, by the rules of :178-212 (only to place the bursts)."""
    H, N, F = hop(fs), frame(fs), frames(fs, x.size)
    sq = np.concatenate([[0.0], np.cumsum(x.astype(np.float64) ** 2)])
    starts = np.arange(F) * H
    db = 10.0 * np.log10((sq[starts + N] - sq[starts]) / N + 1e-12)
    floor = max(noise_rms_db + 6.0, float(np.percentile(db, 30.0)) + 2.0)
    active = db >= floor
    if vad is not None:
        p = np.interp(starts + N * 0.5, (np.arange(vad.size) + 0.5) * vad_window(fs), np.clip(vad, 0.0, 1.0))
        posterior = ((p >= 0.4) & (db >= max(noise_rms_db + 2.0, floor - 4.0))) | (p >= 0.65)
        if np.count_nonzero(posterior) >= 6:
            active = posterior
    if F >= 3:
        active = np.convolve(active.astype(int), np.ones(3, dtype=int), mode="same") > 0
    mask = np.zeros(-(-x.size // H) + 1, dtype=int)
    for f in np.flatnonzero(active):
        mask[f:f + 2] = 1
    return [int(mask[c:c + 20].sum()) for c in range(0, x.size // H - 19, 5)]


@functools.lru_cache(maxsize=None)
def batch(name: str) -> dict:
    """dict(name, fs, kinds, speech [B, n] f32, noise [B, m] f32 | None, noise_rms_db [B], vad [B, n_vad] | None)."""
    fs, B, n, m, with_vad, kinds = BATCHES[name]
    kinds = kinds or ("voice",) * B
    base = 101 + list(BATCHES).index(name)
    speech, noise, vads, levels = [], [], [], []
    for s in range(B):
        rng = np.random.default_rng(90_001 * base + 131 * s)
        z = (rng.standard_normal(max(m, fs)) * _amp(FLOOR_DB - 1.0 + 0.1 * (s % 9)) + DC).astype(np.float32)
        level = rms_db(z)  # the level the caller measured on its room tone, whatever part of it the call is handed
        parts = _components(1_000_003 * base + 7919 * s, s, fs, n)
        for attempt in range(200):
            x, vad = _voice(parts, 1_000_003 * base + 7919 * s + 104_729 * (attempt + 1), s, fs, with_vad)
            if kinds[s] == "all_zero":
                x = np.zeros(n)
            elif kinds[s] == "steady":
                x = rng.standard_normal(n) * _amp(-40.0) + DC
            x = x.astype(np.float32)
            if 11 not in _masked_window_counts(x, fs, level, vad):
                break
        else:
            raise AssertionError((name, s, "no layout keeps the loudness windows off the 0.55 cut"))
        if kinds[s] == "nan":
            x[n // 3] = np.nan
        speech.append(x)
        noise.append(z[:m])
        vads.append(vad)
        levels.append(level)
    return dict(name=name, fs=fs, kinds=kinds, speech=np.stack(speech), noise=np.stack(noise) if m else None,
                noise_rms_db=np.array(levels), vad=np.stack(vads) if with_vad else None)


def resample_input(fs: int) -> np.ndarray:
    """One short float32 stream per rate for the resampler alone: more than two phase cycles of its filter, both edges."""
    rng = np.random.default_rng(424_243 + fs)
    return (0.5 * rng.standard_normal(331 + fs // 400)).astype(np.float32)


# ---- whole capture pairs at 44.1 kHz for the end-to-end operator: three voice captures of 4 s with 2 s of room tone each
CHAIN_RATE, CHAIN_PAIRS, CHAIN_SPEECH_HOPS, CHAIN_NOISE_HOPS = 44_100, 3, 200, 100


@functools.lru_cache(maxsize=None)
def chain_batch() -> dict:
    """dict(fs, speech [3, n] f32, vad [3, n_vad], noise [3, m] f32, noise_vad [3, k])."""
    fs, H = CHAIN_RATE, hop(CHAIN_RATE)
    n, m = CHAIN_SPEECH_HOPS * H, CHAIN_NOISE_HOPS * H
    speech, vads, noise, noise_vad = [], [], [], []
    for s in range(CHAIN_PAIRS):
        rng = np.random.default_rng(77_003 + 17 * s)
        z = (rng.standard_normal(m) * _amp(FLOOR_DB + 0.1 * (s % 5)) + DC).astype(np.float32)
        parts = _components(5_000_011 + 7919 * s, s + 1, fs, n)
        for attempt in range(200):
            x, vad = _voice(parts, 5_000_011 + 7919 * s + 104_729 * (attempt + 1), s + 1, fs, True)
            x = x.astype(np.float32)
            if 11 not in _masked_window_counts(x, fs, rms_db(z), vad):
                break
        else:
            raise AssertionError((s, "no layout keeps the loudness windows off the 0.55 cut"))
        speech.append(x)
        vads.append(vad)
        noise.append(z)
        noise_vad.append(0.03 + 0.05 * rng.random(-(-m // vad_window(fs))))
    return dict(fs=fs, speech=np.stack(speech), vad=np.stack(vads), noise=np.stack(noise), noise_vad=np.stack(noise_vad))


_FIXTURE = None


def fixture():
    """tests/golden/speech_features_rates.npz, loaded once and shared."""
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(pathlib.Path(__file__).resolve().parent / "golden" / "speech_features_rates.npz", allow_pickle=False) as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE
