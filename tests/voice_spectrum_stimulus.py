"""Stimuli of the voice spectrum measurement tests: synthetic captures that take every branch of
python/mic_eq/analysis/spectrum.py:69-343, 519-645 -- gated speech with an in-capture noise floor, bursts too short for the
window statistics (the single-spectrum fallback), steady noise (spread below 6 dB), explicit room-noise captures, VAD
posteriors that are accepted and rejected, and the shortest lengths.  tools/gen_golden_voice_spectrum.py ran the reference over
exactly these arrays; tests/golden/voice_spectrum.npz holds their fingerprints (tests/test_voice_spectrum_stimulus.py).

Everything is a function of (case, nperseg, stream index): no state, no files."""
from __future__ import annotations

import hashlib

import numpy as np

FS = 48_000
MAIN_STREAMS = 67
PARTIALS = 29


def main_length(nperseg: int) -> int:
    return 24 * nperseg + 37  # 47 frames and a ragged tail


def _noise(rng, n: int, level_db: float) -> np.ndarray:
    return rng.standard_normal(n) * 10.0 ** (level_db / 20.0)


def _voice(rng, n: int, seed: int) -> np.ndarray:
    """A harmonic voice: f0 = 110 Hz + a seed-dependent offset, 29 partials falling 1/k^0.8, random phases."""
    f0 = 110.0 + 3.7 * (seed % 23)
    t = np.arange(n, dtype=np.float64) / FS
    x = np.zeros(n)
    for k in range(1, PARTIALS + 1):
        x += np.sin(2.0 * np.pi * f0 * k * t + rng.uniform(0.0, 2.0 * np.pi)) / k**0.8
    return x * (0.2 / np.max(np.abs(x)))


def _envelope(n: int, hop: int, seed: int, nperseg: int) -> np.ndarray:
    """On/off in units of the hop, edges smoothed over half a hop.  Seeds 7 mod 8 get one short burst (too few voiced frames:
    the fallback); the others a square wave whose period and duty depend on the seed."""
    pos = np.arange(n, dtype=np.float64) / hop
    if seed % 8 == 7:
        start = 5.0 + (seed // 8) * 3.3 + (0.21 if nperseg >= 512 else 0.0)
        on = (pos >= start) & (pos < start + 2.6 + 0.45 * (seed // 8 % 3))
    else:
        period = 9.0 + (seed % 7) * 1.3
        duty = (0.22, 0.35, 0.5, 0.68, 0.8)[seed % 5]
        on = ((pos + 2.9 * seed) % period) < duty * period
    k = max(2, hop // 2)
    return np.convolve(on.astype(np.float64), np.ones(k) / k, mode="same")


def main_stream(nperseg: int, seed: int, n: int | None = None) -> np.ndarray:
    """Stream `seed` of the main batch.  64, 65, 66: steady material (no envelope): noise at -30 dB, noise at -55 dB (below the
    absolute gate) and an unbroken voice."""
    n = main_length(nperseg) if n is None else n
    rng = np.random.default_rng(100_003 * nperseg + seed)
    if seed == 64:
        x = _noise(rng, n, -30.0)
    elif seed == 65:
        x = _noise(rng, n, -55.0)
    elif seed == 66:
        x = _voice(rng, n, seed) + _noise(rng, n, -62.0)
    else:
        x = _voice(rng, n, seed) * _envelope(n, nperseg // 2, seed, nperseg) + _noise(rng, n, -62.0)
    return (x + 0.003).astype(np.float32)  # a small DC offset: the detrend has something to remove


def main_batch(nperseg: int, streams: int = MAIN_STREAMS) -> np.ndarray:
    return np.stack([main_stream(nperseg, s) for s in range(streams)])


def noise_capture_batch(nperseg: int, streams: int = 3) -> tuple[np.ndarray, np.ndarray]:
    """(audio, noise_audio): gated voices over a -50 dB floor and a separate room-noise capture of 7 * nperseg + 5 samples."""
    n, m = main_length(nperseg), 7 * nperseg + 5
    audio, noise = [], []
    for s in range(streams):
        rng = np.random.default_rng(200_003 * nperseg + s)
        audio.append((_voice(rng, n, 3 + s) * _envelope(n, nperseg // 2, 2 + s, nperseg) + _noise(rng, n, -50.0)).astype(np.float32))
        noise.append((_noise(rng, m, -50.0) + 0.001).astype(np.float32))
    return np.stack(audio), np.stack(noise)


def vad_batch(nperseg: int) -> tuple[np.ndarray, np.ndarray]:
    """(audio, vad_probabilities[4][n_vad]).  Streams 0, 1: posteriors that follow the envelope (0 also marks two quiet windows
    as strong speech): the fused mask is accepted.  Streams 2, 3: posteriors that never reach the evidence threshold, and one
    that is strong in two windows only: fewer than three frames, so the energy mask is used."""
    n = main_length(nperseg)
    win = int(np.ceil(FS * 512 / 16_000))
    n_vad = -(-n // win)
    centres = ((np.arange(n_vad) + 0.5) * win).astype(np.int64).clip(0, n - 1)
    audio, vad = [], []
    for s in range(4):
        rng = np.random.default_rng(300_003 * nperseg + s)
        env = _envelope(n, nperseg // 2, 1 + s, nperseg)
        audio.append((_voice(rng, n, 9 + s) * env + _noise(rng, n, -62.0)).astype(np.float32))
        if s < 2:
            p = 0.08 + 0.8 * env[centres]
            if s == 0:
                quiet = np.flatnonzero(env[centres] < 0.01)[:2]
                p[quiet] = 0.9
        elif s == 2:
            p = 0.05 + 0.3 * env[centres]
        else:
            p = np.full(n_vad, 0.1)
            p[n_vad // 2: n_vad // 2 + 1] = 0.97
        vad.append(p)
    return np.stack(audio), np.stack(vad).astype(np.float64)


def short_batch(nperseg: int, n: int) -> np.ndarray:
    """Two streams of exactly `n` samples (one frame: nperseg and nperseg + hop - 1; three frames: 2 * nperseg)."""
    return np.stack([main_stream(nperseg, s, n) for s in (2, 64)])


SHORT_LENGTHS = lambda nperseg: (nperseg, nperseg + nperseg // 2 - 1, 2 * nperseg)  # noqa: E731


def fingerprint(x: np.ndarray) -> dict:
    """SHA-256 over the little-endian float bytes, with the first and last 8 values."""
    flat = np.ascontiguousarray(x).reshape(-1)
    kind = "<f4" if flat.dtype == np.float32 else "<f8"
    return {"sha256": hashlib.sha256(flat.astype(kind).tobytes()).hexdigest(), "head": flat[:8].astype(np.float64),
            "tail": flat[-8:].astype(np.float64), "size": flat.size}


def gate_margins(frame_rms_db: np.ndarray, voiced_mask: np.ndarray, with_vad: bool, explicit_noise: bool) -> dict:
    """How far (dB) the decisions of spectrum.py:81-97, 208-221, 238-241 and 580-583 are from flipping for one stream: the
    smallest |frame level - gate| per gate and |voiced level - unvoiced level - 3|; inf where a decision is not taken."""
    rms = np.asarray(frame_rms_db, dtype=np.float64)
    mask = np.asarray(voiced_mask, dtype=bool)
    floor_db, peak_db = (float(np.percentile(rms, q)) for q in (20.0, 95.0))
    spread = peak_db - floor_db
    out = {"select_gate": np.inf, "mask_gate": np.inf, "support_gate": np.inf, "noise_level": np.inf, "spread": abs(spread - 6.0)}
    if spread >= 6.0:
        out["select_gate"] = float(np.min(np.abs(rms - max(-48.0, floor_db + 0.60 * spread))))
        out["mask_gate"] = float(np.min(np.abs(rms - max(-48.0, floor_db + 0.60 * max(spread, 6.0)))))
    if with_vad:
        out["support_gate"] = float(np.min(np.abs(rms - max(-48.0, floor_db + 0.25 * max(spread, 6.0)))))
    if not explicit_noise and np.count_nonzero(~mask) >= 3 and np.count_nonzero(mask) > 0:
        out["noise_level"] = abs(float(np.median(rms[mask])) - float(np.median(rms[~mask])) - 3.0)
    return out


def cases() -> list[dict]:
    """Every batch the fixture holds: name, nperseg, audio [streams, n], optional vad / noise."""
    out = [{"name": f"main{n}", "nperseg": n, "audio": main_batch(n)} for n in (256, 512)]
    audio, noise = noise_capture_batch(256)
    out.append({"name": "noise256", "nperseg": 256, "audio": audio, "noise": noise})
    out.append({"name": "shortnoise256", "nperseg": 256, "audio": audio[:1], "noise": noise[:1, :200]})  # below one frame: ignored
    audio, vad = vad_batch(256)
    out.append({"name": "vad256", "nperseg": 256, "audio": audio, "vad": vad})
    for n in SHORT_LENGTHS(256):
        out.append({"name": f"short256_{n}", "nperseg": 256, "audio": short_batch(256, n)})
    out.append({"name": "main4096", "nperseg": 4096, "audio": main_batch(4096, 5)})
    return out


def checkpoint_bins(bins: int) -> np.ndarray:
    """The 16 bins whose values the fixture holds for every stream."""
    return np.linspace(0, bins - 1, 16).astype(np.int64)


_FIXTURE = None


def fixture():
    """tests/golden/voice_spectrum.npz, loaded once and shared."""
    global _FIXTURE
    if _FIXTURE is None:
        import pathlib

        with np.load(pathlib.Path(__file__).resolve().parent / "golden" / "voice_spectrum.npz") as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE


def fixture_case(case: dict) -> dict:
    """One case's arrays of the fixture by field, with its mask unpacked and the stimulus rows the fixture holds."""
    fx, name = fixture(), case["name"]
    out = {k.split("/", 1)[1]: v for k, v in fx.items() if k.startswith(name + "/")}
    frames = int(out["scalars"][0, 0])
    out["voiced_mask"] = np.unpackbits(out["voiced_mask"], axis=1)[:, :frames]
    return out
