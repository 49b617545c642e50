"""Stimulus of the second-passage measurements: closed-form spectra (no random numbers, so the generator and the tests build
the same bytes), spectral SNR rows and signals.

The spectra drive every clip of the adaptive house curve (target.py:27-56) that a spectrum can drive, to both ends:
low_mid_balance, sibilance_ratio and tilt_norm.  The clips of warmth_offset (|0.9 x| <= 0.9 < 1.2), presence_offset
(|0.8 x - 0.5 y| <= 1.3 < 1.5), the lower one of sibilance_offset (1.2 < 1.8), the flat branch's (0.6 < 0.8, then < 1.0) and the
final +-2 dB (the three Gaussians peak octaves apart: below 1.9 together) cannot bind for any input, by those bounds."""
from __future__ import annotations

import numpy as np

FS = 48_000
PRESETS = ("broadcast", "podcast", "streaming", "flat")
# nperseg -> masked bins 80..12000 Hz: 4096 -> 1018 (even), 2048 -> 509 (odd), 64 -> 16, 16 -> 4 (below 8: +inf)
NPERSEGS = (4096, 2048, 64, 16)
MASKED_BINS = {4096: 1018, 2048: 509, 64: 16, 16: 4}


def grid(nperseg: int) -> np.ndarray:
    return np.fft.rfftfreq(nperseg, 1.0 / FS)


def _octaves(f, centre):
    return np.log2(np.maximum(f, 20.0) / centre)


def _band(f, low, high, gain):
    return np.where((f >= low) & (f <= high), gain, 0.0)


def _voice(f):
    return -34.0 - 2.2 * _octaves(f, 500.0) ** 2 + 1.5 * np.sin(f / 300.0) + 0.7 * np.cos(f / 47.0)


SPECTRA = {
    "voice": _voice,
    "tilt_up": lambda f: _voice(f) + 16.0 * _octaves(f, 1000.0),       # tilt_norm -> +1
    "tilt_down": lambda f: _voice(f) - 8.0 * _octaves(f, 1000.0),     # tilt_norm -> -1
    "body_heavy": lambda f: _voice(f) + _band(f, 180.0, 800.0, 24.0),      # low_mid_balance -> +1
    "presence_heavy": lambda f: _voice(f) + _band(f, 1200.0, 3500.0, 24.0),  # low_mid_balance -> -1, sibilance_ratio -> -1
    "sibilant": lambda f: _voice(f) + _band(f, 5500.0, 8500.0, 30.0),      # sibilance_ratio -> +1
    "level_shifted": lambda f: _voice(f) + 17.25,                      # the error is level-invariant
    "flat_line": lambda f: np.full_like(f, -40.0),
}
# the value each case drives to its end, for the generator's and the tests' assertions: (scalar, sign)
CLIP_CASES = {"tilt_up": ("tilt", 1), "tilt_down": ("tilt", -1), "body_heavy": ("low_mid_balance", 1),
              "presence_heavy": ("low_mid_balance", -1), "sibilant": ("sibilance", 1)}


def spectrum(name: str, nperseg: int) -> np.ndarray:
    return np.asarray(SPECTRA[name](grid(nperseg)), dtype=np.float64)


def spectral_snr(nperseg: int, variant: int = 0) -> np.ndarray:
    f = grid(nperseg)
    return 18.0 - 3.0 * _octaves(f, 1500.0) ** 2 * 0.4 + 2.0 * np.sin(f / (210.0 + 13.0 * variant)) + 0.25 * variant


def batch(nperseg: int, n_streams: int):
    """original, before, after [streams, bins], snr [streams, bins] with NaN rows, and the preset names: every spectrum and every
    preset occurs from 8 streams on; stream 1's SNR has a NaN in the body band, stream 2's in every band."""
    names = list(SPECTRA)
    before = np.stack([spectrum(names[s % len(names)], nperseg) for s in range(n_streams)])
    after = np.stack([spectrum(names[(s + 3) % len(names)], nperseg) + 0.5 * np.sin(grid(nperseg) / 900.0 + s) for s in range(n_streams)])
    original = np.stack([spectrum(names[s % len(names)], nperseg) + 0.8 * np.cos(grid(nperseg) / 650.0 + 0.3 * s) + 2.0
                         for s in range(n_streams)])
    snr = np.stack([spectral_snr(nperseg, s) for s in range(n_streams)])
    f = grid(nperseg)
    if n_streams > 1:
        snr[1, np.argmax(f >= 250.0)] = np.nan
    if n_streams > 2:
        snr[2, ::3] = np.nan
    presets = [PRESETS[(s + s // 4) % 4] for s in range(n_streams)]
    return original, before, after, snr, presets


LENGTHS = (1, 63, 64, 65, 4097, 201_600)  # around the pairwise sum's blocks of 128, its eight lanes, and one 4.2 s passage


def signal(n: int, seed: int = 0) -> np.ndarray:
    """A voiced-looking deterministic signal of n samples, peak below 0.9."""
    t = np.arange(n, dtype=np.float64)
    x = 0.5 * np.sin(t * (0.031 + 0.002 * seed)) * (0.6 + 0.4 * np.sin(t * 0.00043 + seed)) + 0.2 * np.sin(t * 0.37 + 0.5 * seed)
    return x.astype(np.float32)


# ---- whole verification runs: the six chain pairs of tests/speech_features_stimulus.py, each with a second passage
GENTLE = {"enabled": True, "threshold_db": -18.0, "ratio": 2.0, "attack_ms": 10.0, "release_ms": 200.0}
TREBLE_BOOST = {"band_freqs": [80.0, 160.0, 320.0, 640.0, 1280.0, 2500.0, 5000.0, 8000.0, 12000.0, 16000.0],
                "band_gains": [0.0, 0.0, 0.0, 0.0, 0.0, 6.0, 6.0, 6.0, 6.0, 0.0], "band_qs": [1.41] * 10}
# (name, chain pair, peak the setup passage is scaled to or None, gain of the verification passage on top, setup result)
RUN_CASES = (
    ("gentle_0", 0, None, 1.0, {"compressor_settings": GENTLE}),
    ("gentle_1", 1, None, 1.0, {"compressor_settings": GENTLE, "deesser_settings": {}}),
    ("limiter_0", 2, 0.95, 1.0, {"compressor_settings": dict(GENTLE, threshold_db=-6.0)}),
    ("limiter_1", 3, 0.95, 1.0, {"compressor_settings": dict(GENTLE, threshold_db=-6.0)}),
    ("hard_compressor_0", 4, None, 1.0, {"compressor_settings": dict(GENTLE, threshold_db=-30.0, ratio=3.0)}),
    ("hard_compressor_1", 5, None, 1.0, {"compressor_settings": dict(GENTLE, threshold_db=-45.0, ratio=8.0)}),
    ("treble_boost", 0, None, 1.0, {"compressor_settings": GENTLE, "eq_settings": TREBLE_BOOST}),
    ("level_mismatch_0", 1, 0.95, 0.25, {"compressor_settings": GENTLE}),
    ("level_mismatch_1", 2, 0.95, 0.25, {"compressor_settings": GENTLE}),
    ("clipped", 3, None, 1.0, {"compressor_settings": GENTLE}),
)
RUN_PRESETS = ("broadcast", "podcast", "streaming", "flat")
SHORT_SAMPLES = 100_000  # the third retry route, a call of its own (a batch shares its length)


def run_batch() -> dict:
    """dict(noise, original, verification [cases, n] f32, setups, presets): the second passage is the setup passage played
    backwards (the same delivery and level, another order of sounds); "clipped" has one sample at 1.0."""
    import speech_features_stimulus as ST

    c = ST.chain_batch()
    noise, original, verification, setups, presets = [], [], [], [], []
    for k, (name, pair, peak, gain, setup) in enumerate(RUN_CASES):
        speech = c["speech"][pair].astype(np.float32)
        if peak is not None:
            speech = (speech * np.float32(peak / float(np.max(np.abs(speech))))).astype(np.float32)
        second = np.ascontiguousarray(speech[::-1] * np.float32(gain))
        if name == "clipped":
            second[second.size // 2] = np.float32(1.0)
        noise.append(c["noise"][pair].astype(np.float32))
        original.append(speech)
        verification.append(second)
        setups.append(setup)
        presets.append(RUN_PRESETS[k % 4])
    return dict(noise=np.stack(noise), original=np.stack(original), verification=np.stack(verification), setups=setups, presets=presets)


# ---- the offline validation: analyze_voice_setup on the six chain pairs, without and with a caller's EQ
OFFLINE_EQ = {"band_freqs": [80.0, 160.0, 320.0, 640.0, 1280.0, 2500.0, 5000.0, 8000.0, 12000.0, 16000.0],
              "band_gains": [0.0, -1.0, 0.0, 0.0, 0.0, 2.0, 1.0, 0.0, 0.0, 0.0], "band_qs": [1.41] * 10}


def offline_eq(stream: int) -> dict:
    """The caller's EQ of a stream: analysis_confidence on all, apply_recommended False on the odd ones, absent on stream 4."""
    eq = dict(OFFLINE_EQ, analysis_confidence=0.62 + 0.05 * stream)
    if stream % 2:
        eq["apply_recommended"] = False
    elif stream != 4:
        eq["apply_recommended"] = True
    return eq
