"""Stimuli of the reliability statistics' tests (the second half of analyze_voice_spectrum, spectrum.py:647-742): the batches of
tests/voice_spectrum_stimulus.py, which take most of its paths, and `long256`, three captures of 199 frames whose 21 to 33
effective blocks clip the duration term at 1 (no other case reaches 12 blocks), and `closest256`, two three-window captures that
take the closest-windows branch of :281-285 (of the two streams of short256_512 only the first does).  tools/gen_golden_voice_reliability.py ran the
reference over exactly these arrays; tests/golden/voice_reliability.npz holds their fingerprints and the reference's results.

Everything is a function of (case, nperseg, stream index): no state, no files."""
from __future__ import annotations

import pathlib

import numpy as np

import voice_spectrum_stimulus as VS

FS = VS.FS
LONG_SEEDS = (3, 12, 24)
LONG_LENGTH = 100 * 256 + 37
CLOSEST_SEEDS = (8, 14)  # three windows with one shape outlier: two inliers are fewer than the minimum of three
SCALARS = ("snr_db", "spectral_tilt_db_per_octave", "residual_confidence", "measurement_coverage", "outlier_rejection_ratio",
           "phonetic_coverage", "effective_measurement_blocks")
SPECTRA = ("median_spectrum_db", "spectral_repeatability", "measurement_uncertainty_db", "spectral_snr_db")


def long_batch() -> np.ndarray:
    return np.stack([VS.main_stream(256, s, LONG_LENGTH) for s in LONG_SEEDS])


def cases() -> list[dict]:
    """Every batch the fixture holds: name, nperseg, audio [streams, n], optional vad / noise."""
    closest = np.stack([VS.main_stream(256, s, 512) for s in CLOSEST_SEEDS])
    return VS.cases() + [{"name": "long256", "nperseg": 256, "audio": long_batch()}, {"name": "closest256", "nperseg": 256, "audio": closest}]


def fixture_streams(case: dict) -> np.ndarray:
    """The streams of a case the fixture holds (every third of main512, as in tests/golden/voice_spectrum.npz)."""
    streams = np.arange(case["audio"].shape[0])
    return streams[::3] if case["name"] == "main512" else streams


def cutoff_margin(distance: np.ndarray) -> float:
    """How far (dB) the inlier decision of spectrum.py:276-279 is from flipping: the smallest |distance - cutoff|."""
    d = np.asarray(distance, dtype=np.float64)
    mid = float(np.median(d))
    cutoff = mid + 4.0 * max(float(np.median(np.abs(d - mid))), 0.25)
    return float(np.min(np.abs(d - cutoff)))


_FIXTURE = None


def fixture() -> dict:
    """tests/golden/voice_reliability.npz, loaded once and shared."""
    global _FIXTURE
    if _FIXTURE is None:
        with np.load(pathlib.Path(__file__).resolve().parent / "golden" / "voice_reliability.npz") as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE


def fixture_case(name: str) -> dict:
    """One case's arrays of the fixture by field, masks unpacked to [streams, frames]."""
    out = {k.split("/", 1)[1]: v for k, v in fixture().items() if k.startswith(name + "/")}
    frames = int(out["shape"][3])
    for key in ("voiced_mask", "inlier_mask"):
        out[key] = np.unpackbits(out[key], axis=1)[:, :frames]
    return out
