"""Stimuli of the speech-feature tests (python/mic_eq/analysis/voice_setup.py:161-458 at 48 kHz): seeded voice captures made of a
noise floor, voiced tone bursts (sixteen harmonics at the most, below 4 kHz) and, on two streams out of three, broadband bursts between 5.5
and 8.5 kHz at the end of every voiced burst, each with a room-noise capture and a track of speech posteriors.  The main batch
has 67 streams (one past the 64-lane tile) of 201,600 samples (209 frames, two short-term windows); the small batches take
the other paths: one frame, a partial tail chunk, exactly one momentary window, momentary windows without a short-term one, no
posteriors, fewer than six posterior-active frames, no noise capture, a noise capture below one frame, an all-zero stream, a
steady stream in which no frame passes the adaptive floor, and a stream with a NaN.

Burst edges lie on the 960-sample hop grid.  Their places are drawn per stream until no 0.4 s loudness window has exactly 11 of
its 20 hops active: 11 / 20 is the 0.55 cut of :154 itself, and a window there would be decided by rounding.
tools/gen_golden_speech_features.py ran the reference over exactly these arrays and asserts that condition with the reference's
own mask; tests/golden/speech_features.npz holds their fingerprints (tests/test_speech_features_stimulus.py).

Everything is a function of (batch, stream index): no state, no files."""
from __future__ import annotations

import functools
import pathlib

import numpy as np

from voice_spectrum_stimulus import fingerprint  # noqa: F401  (shared with the other fixtures)

FS, FRAME, HOP, VAD_WINDOW = 48_000, 1920, 960, 1536
FLOOR_DB, VOICED_DB = -62.0, -20.0
DC = 0.0002  # a small offset: the frames' detrend has something to remove
MARGIN = 1e-6
# name -> (streams, speech samples, noise samples or 0, posteriors, kind of every stream or None for "voice")
BATCHES = {
    "main": (67, 201_600, 48_000, True, None),
    "one_frame": (2, 1920, 48_000, False, None),
    "tail": (2, 1920 + 959, 48_000, True, None),
    "one_window": (3, 19_200, 48_000, True, None),
    "no_short_term": (3, 120_000, 48_000, True, None),
    "no_vad": (3, 96_000, 48_000, False, None),
    "few_posterior": (3, 96_000, 48_000, True, ("few_posterior",) * 3),
    "no_noise": (3, 96_000, 0, True, None),
    "short_noise": (3, 96_000, 1000, True, None),
    "special": (5, 48_000, 48_000, False, ("voice", "all_zero", "steady", "nan", "voice")),
}
CLASSES = tuple(BATCHES) + ("all_zero", "steady", "nan")


def _amp(db: float) -> float:
    return 10.0 ** (db / 20.0)


def frames(n: int) -> int:
    return 0 if n < FRAME else (n - FRAME) // HOP + 1


def chunks(n: int) -> int:
    return -(-n // HOP)


def sibilance_db(stream: int) -> float | None:
    """The level of the broadband bursts of a stream: none on every third, otherwise -44 .. -20 dB."""
    return None if stream % 3 == 0 else -44.0 + 4.0 * (stream % 7)


def _layout(rng, n_chunks: int):
    """Voiced bursts [k0, k1) in hops with the hops of each that are sibilant instead, at least 24 hops apart."""
    bursts, k = [], int(rng.integers(4, 12))
    while True:
        length = int(rng.integers(22, 40))
        if k + length + 3 > n_chunks:
            break
        bursts.append((k, k + length, int(rng.integers(4, 9))))
        k += length + int(rng.integers(24, 36))
    if not bursts and n_chunks >= 8:  # a short capture: one burst in its middle
        k0 = int(rng.integers(2, max(3, n_chunks // 3)))
        bursts.append((k0, int(rng.integers(k0 + 3, n_chunks - 1)), 2))
    return bursts


def _band_noise(rng, n: int, low: float, high: float) -> np.ndarray:
    X = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / FS)
    X[(f < low) | (f > high)] = 0.0
    x = np.fft.irfft(X, n)
    return x / np.sqrt(np.mean(x * x))


def _components(seed: int, stream: int, n: int):
    """What a stream is mixed from, whatever its layout: the floor, a unit-RMS harmonic series and unit-RMS 5.5-8.5 kHz noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / FS
    f0 = 105.0 + 9.0 * (stream % 13)
    voiced = np.zeros(n)
    for h in range(1, 1 + min(16, int(3800.0 // f0))):
        voiced += np.sin(2.0 * np.pi * f0 * h * t + rng.uniform(0.0, 2.0 * np.pi)) / h ** (0.8 + 0.05 * (stream % 5))
    voiced /= np.sqrt(np.mean(voiced * voiced))
    return rng.standard_normal(n) * _amp(FLOOR_DB), voiced, _band_noise(rng, n, 5500.0, 8500.0)


def _voice(parts, seed: int, stream: int, with_vad: bool, kind: str):
    floor, voiced, hiss = parts
    n = floor.size
    rng = np.random.default_rng(seed)
    C = chunks(n)
    bursts = _layout(rng, n // HOP)
    env_v, env_s = np.zeros(C), np.zeros(C)
    for k0, k1, sib in bursts:
        env_v[k0:k1 - sib] = 1.0
        env_s[k1 - sib:k1] = 1.0
    env_v, env_s = np.repeat(env_v, HOP)[:n], np.repeat(env_s, HOP)[:n]
    level = sibilance_db(stream)
    x = floor + voiced * _amp(VOICED_DB) * env_v
    if level is None:
        x += voiced * _amp(VOICED_DB - 6.0) * env_s  # the burst goes on, quieter
    else:
        x += hiss * _amp(level) * env_s + voiced * _amp(VOICED_DB - 20.0) * env_s
    vad = None
    if with_vad:
        n_vad = -(-n // VAD_WINDOW)
        centres = (np.arange(n_vad) + 0.5) * VAD_WINDOW / HOP  # in hops
        vad = 0.04 + 0.1 * rng.random(n_vad)
        if kind == "few_posterior":  # three posterior-active frames at the most: the energy mask is kept
            k0 = bursts[0][0]
            vad[(centres >= k0 + 2) & (centres < k0 + 5)] = 0.9
        else:
            for k0, k1, sib in bursts:
                vad[(centres >= k0 - 1) & (centres < k1 - sib + 0.5)] = 0.8 + 0.15 * rng.random()
                vad[(centres >= k1 - sib + 0.5) & (centres < k1 + 1)] = 0.25 + 0.5 * rng.random()  # sibilants: often below 0.4
    return x + DC, vad


def _masked_window_counts(x: np.ndarray, noise_rms_db: float, vad):
    """The number of active hops in every 0.4 s window, by the rules of :178-212 (only to place the bursts; the fixture
    generator repeats the check with the reference's own mask)."""
    F = frames(x.size)
    sq = np.concatenate([[0.0], np.cumsum(x.astype(np.float64) ** 2)])
    starts = np.arange(F) * HOP
    db = 10.0 * np.log10((sq[starts + FRAME] - sq[starts]) / FRAME + 1e-12)
    floor = max(noise_rms_db + 6.0, float(np.percentile(db, 30.0)) + 2.0)
    active = db >= floor
    if vad is not None:
        p = np.interp(starts + FRAME * 0.5, (np.arange(vad.size) + 0.5) * VAD_WINDOW, np.clip(vad, 0.0, 1.0))
        posterior = ((p >= 0.4) & (db >= max(noise_rms_db + 2.0, floor - 4.0))) | (p >= 0.65)
        if np.count_nonzero(posterior) >= 6:
            active = posterior
    if F >= 3:
        active = np.convolve(active.astype(int), np.ones(3, dtype=int), mode="same") > 0
    mask = np.zeros(chunks(x.size) + 1, dtype=int)
    for f in np.flatnonzero(active):
        mask[f:f + 2] = 1
    return [int(mask[c:c + 20].sum()) for c in range(0, x.size // HOP - 19, 5)]


def rms_db(x: np.ndarray) -> float:
    x = np.asarray(x, dtype=np.float64)
    return float(10.0 * np.log10(np.mean(x * x) + 1e-18)) if x.size else -120.0


@functools.lru_cache(maxsize=None)
def batch(name: str) -> dict:
    """dict(name, kinds, speech [B, n] f32, noise [B, m] f32 | None, noise_rms_db [B], vad [B, n_vad] | None)."""
    B, n, m, with_vad, kinds = BATCHES[name]
    kinds = kinds or ("voice",) * B
    base = 1 + list(BATCHES).index(name)
    speech, noise, vads, levels = [], [], [], []
    for s in range(B):
        rng = np.random.default_rng(90_001 * base + 131 * s)
        z = (rng.standard_normal(max(m, 48_000)) * _amp(FLOOR_DB - 1.0 + 0.1 * (s % 9)) + DC).astype(np.float32)
        level = rms_db(z)  # the level the caller measured on its room tone, whatever part of it the call is handed
        parts = _components(1_000_003 * base + 7919 * s, s, n)
        for attempt in range(200):
            x, vad = _voice(parts, 1_000_003 * base + 7919 * s + 104_729 * (attempt + 1), s, with_vad, kinds[s])
            if kinds[s] == "all_zero":
                x = np.zeros(n)
            elif kinds[s] == "steady":
                x = rng.standard_normal(n) * _amp(-40.0) + DC
            x = x.astype(np.float32)
            if 11 not in _masked_window_counts(x, level, vad):
                break
        else:
            raise AssertionError((name, s, "no layout keeps the loudness windows off the 0.55 cut"))
        if kinds[s] == "nan":
            x[n // 3] = np.nan
        speech.append(x)
        noise.append(z[:m])
        vads.append(vad)
        levels.append(level)
    return dict(name=name, kinds=kinds, speech=np.stack(speech), noise=np.stack(noise) if m else None,
                noise_rms_db=np.array(levels), vad=np.stack(vads) if with_vad else None)


def batches() -> tuple:
    return tuple(batch(name) for name in BATCHES)


_FIXTURE = None


def fixture():
    """tests/golden/speech_features.npz, loaded once and shared."""
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(pathlib.Path(__file__).resolve().parent / "golden" / "speech_features.npz", allow_pickle=False) as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE


# ---- what the other analyses hand the recommendation rules (voice_setup.py:1143-1223): made up per stream, so that the rules
# are tested on their own; every status, dynamics profile and preset, auto-makeup on and off
SETUP_FREQS = np.fft.rfftfreq(4096, 1.0 / FS)
SETUP_STATUS = ("usable", "usable", "questionable", "usable", "invalid")
SETUP_PROFILES = ("gentle", "balanced", "dense", "custom")
SETUP_PRESETS = ("broadcast", "streaming", "podcast", "flat", "something else")


def setup_inputs(stream: int) -> dict:
    """The arguments of mic_eq_mi.recommend_voice_chain for stream `stream` of the main batch (but the features)."""
    rng = np.random.default_rng(55_001 + stream)
    octaves = np.log2(np.maximum(SETUP_FREQS, 50.0) / 1000.0)
    spectrum = -32.0 - (3.0 + 0.2 * (stream % 9)) * octaves + 0.4 * np.cumsum(rng.standard_normal(SETUP_FREQS.size)) / 8.0
    spectrum += (stream % 4) * 2.0 * np.exp(-0.5 * ((SETUP_FREQS - (5200.0 + 450.0 * (stream % 8))) / 900.0) ** 2)
    return dict(freqs=SETUP_FREQS, smoothed_spectrum_db=spectrum, residual_confidence=float(0.55 + 0.44 * rng.random()),
                snr_db=float((3.0, 9.0, 14.0, 25.0, 31.0)[stream % 5] + rng.random()), used_single_spectrum_fallback=stream % 11 == 5,
                noise_quality_score=float(0.55 + 0.44 * rng.random()), noise_status=SETUP_STATUS[(stream // 2) % 5],
                conservative_noise_rms_db=float(batch("main")["noise_rms_db"][stream]), target_preset=SETUP_PRESETS[stream % 5],
                vad_available=stream % 6 != 0, dynamics_intensity=SETUP_PROFILES[stream % 4],
                custom_target_p95_db=0.5 + 1.2 * (stream % 8), custom_peak_cap_db=4.0 + 1.5 * (stream % 7))


# ---- whole capture pairs for the end-to-end operator: the voice captures and posteriors of six streams of the main batch,
# each with 2 s of room tone (the reference's analyze_voice_setup refuses less than 1.5 s, :1099) and its posteriors
CHAIN_STREAMS = (0, 1, 2, 7, 33, 66)
CHAIN_NOISE_SAMPLES = 96_000
# the two argument sets the fixture holds: analyze_voice_setup's defaults, and a custom profile on another preset
CHAIN_ARGUMENTS = (dict(target_preset="broadcast", dynamics_intensity="balanced", custom_target_p95_db=3.5, custom_peak_cap_db=8.0),
                   dict(target_preset="podcast", dynamics_intensity="custom", custom_target_p95_db=5.0, custom_peak_cap_db=9.0))


@functools.lru_cache(maxsize=None)
def chain_batch() -> dict:
    """dict(speech [6, n] f32, vad [6, n_vad], noise [6, m] f32, noise_vad [6, k])."""
    main = batch("main")
    pick = list(CHAIN_STREAMS)
    noise, noise_vad = [], []
    for s in pick:
        rng = np.random.default_rng(77_003 + 17 * s)
        noise.append((rng.standard_normal(CHAIN_NOISE_SAMPLES) * _amp(FLOOR_DB + 0.1 * (s % 5)) + DC).astype(np.float32))
        noise_vad.append(0.03 + 0.05 * rng.random(-(-CHAIN_NOISE_SAMPLES // VAD_WINDOW)))
    return dict(speech=main["speech"][pick], vad=main["vad"][pick], noise=np.stack(noise), noise_vad=np.stack(noise_vad))
