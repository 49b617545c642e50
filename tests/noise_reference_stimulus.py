"""Stimuli of the room-noise reference analysis tests: seeded broadband capture pairs that between them take every branch of
python/mic_eq/analysis/noise_reference.py:118-546 -- every status, every reason audio can cause (short, non-finite, silent,
clipped at both levels, both stationarity levels, both transient levels, both consistency levels in both directions), the
contamination levels and the in-capture selection with and without VAD posteriors, age and metadata reasons through the
arguments, no voice capture, and a noise capture shorter than one analysis frame.  tools/gen_golden_noise_reference.py ran the
reference over exactly these arrays; tests/golden/noise_reference.npz holds their fingerprints
(tests/test_noise_reference_stimulus.py).

Everything is a function of (batch, stream index): no state, no files."""
from __future__ import annotations

import functools

import numpy as np

from voice_spectrum_stimulus import checkpoint_bins, fingerprint  # noqa: F401  (shared with the other fixtures)

RATES = (2560, 3000, 3150, 4410, 48_000)
NOISE_FRAMES, VOICE_FRAMES = 15, 24  # 1.6 s of room tone (the shortest the reference accepts is 1.5 s), 2.5 s of voice
FLOOR_DB, SPEECH_DB = -50.0, -22.0
DC = 0.0002  # a small offset: the frames' detrend has something to remove
MARGIN = 1e-6  # the project's MARGIN_DB: how far every decision quantity stays from its threshold

# the kinds of the main batches; stream s of a main batch is kind MAIN_KINDS[s % len(MAIN_KINDS)] (48 kHz: MAIN_48K)
MAIN_KINDS = ("usable", "non_finite", "silent", "clipped", "isolated_clip", "ramp_questionable", "ramp_invalid", "tilt_strong",
              "tilt_dominant", "quieter_15", "quieter_9", "louder_16", "louder_25", "steady_voice", "stale", "maybe_stale",
              "negative_age", "device", "channel_mode", "channel_count", "noise_rate", "voice_rate", "rate_changed",
              "voice_non_finite")
# (the fixture holds the first stream's spectra in full: at 9600-sample frames that one has no in-capture spectrum, which keeps
# the file below the largest fixture already there; the other streams' in-capture spectra are held at the checkpoint bins)
MAIN_48K = ("steady_voice", "tilt_dominant", "quieter_9", "non_finite", "isolated_clip", "usable")
MAIN_STREAMS = {2560: 24, 3000: 67, 3150: 24, 4410: 24, 48_000: 6}
VAD_KINDS = ("vad_clean", "vad_speech_present", "vad_possible_speech", "vad_too_few_frames", "vad_clean")
# metadata kinds -> (noise metadata, voice metadata) overrides; "fs" stands for the analysis rate, "fs+1" for another
METADATA = {
    "device": ({"input_device": "mic A"}, {"input_device": "mic B"}),
    "channel_mode": ({"channel_mode": "left"}, {"channel_mode": "average"}),
    "channel_count": ({"channel_count": 1}, {"channel_count": 2}),
    "noise_rate": ({"sample_rate": "fs+1"}, {}),
    "voice_rate": ({}, {"sample_rate": "fs+1"}),
    "rate_changed": ({"sample_rate": "fs+1"}, {"sample_rate": "fs"}),
}
MISMATCH_BITS = {"device": 1, "channel_mode": 2, "channel_count": 4, "noise_rate": 8, "voice_rate": 16, "rate_changed": 8 | 32}
AGES = {"stale": 700.0, "maybe_stale": 200.0, "negative_age": -5.0}


def frame_size(fs: int) -> int:
    return max(512, int(round(fs * 0.20)))


def _shaped(rng, n: int, tilt_db_per_octave: float = 0.0) -> np.ndarray:
    """Unit-RMS Gaussian noise whose power rises by `tilt` dB per octave."""
    x = rng.standard_normal(n)
    if tilt_db_per_octave:
        X = np.fft.rfft(x)
        k = np.arange(X.size, dtype=np.float64)
        k[0] = 1.0
        X *= k ** (tilt_db_per_octave / (20.0 * np.log10(2.0)))
        x = np.fft.irfft(X, n)
    return x / np.sqrt(np.mean(x * x))


def _amp(db: float) -> float:
    return 10.0 ** (db / 20.0)


def _voice(rng, n: int, hop: int, steady: bool = False) -> np.ndarray:
    """A noise floor with louder bursts over hops 3-7, 11-15 and 19-22: seven frames stay on the floor."""
    x = _shaped(rng, n) * _amp(FLOOR_DB)
    if not steady:
        pos = np.arange(n, dtype=np.float64) / hop
        on = ((pos >= 3) & (pos < 8)) | ((pos >= 11) & (pos < 16)) | ((pos >= 19) & (pos < 23))
        k = max(2, hop // 4)
        inner = np.convolve(on.astype(np.float64), np.ones(k) / k, mode="same") * on  # fades stay inside the bursts
        x = x + _shaped(rng, n, -3.0) * _amp(SPEECH_DB) * inner
    return x + DC


def _tilt_for(fs: int, dominant: bool) -> float:
    """dB per octave of the tilted stretch: the flux is the median over the bands of the change, so it grows with the band count."""
    if fs * 0.49 > 2828.0:  # six or seven bands
        return 18.0 if dominant else 4.5
    return 30.0 if dominant else (8.0 if fs * 0.49 > 1414.0 else 12.0)


def _pair(kind: str, fs: int, seed: int, n_noise: int, n_voice: int):
    N = frame_size(fs)
    hop = N // 2
    rng = np.random.default_rng(7_000_003 * fs + 1009 * seed + 17)
    noise = _shaped(rng, n_noise) * _amp(FLOOR_DB) + DC
    voice = _voice(rng, n_voice, hop, steady=kind == "steady_voice") if n_voice else None
    if kind == "non_finite":
        noise[7 % n_noise], noise[min(100, n_noise - 1)] = np.inf, np.nan
    elif kind == "silent":
        noise[:] = 0.0
    elif kind == "clipped":
        noise[5::97] = 1.0
        noise[50::97] = -1.0
    elif kind == "isolated_clip":
        noise[n_noise // 2 + 11] = 1.0
    elif kind in ("ramp_questionable", "ramp_invalid"):
        noise = (noise - DC) * _amp(np.linspace(0.0, 10.0 if kind == "ramp_questionable" else 24.0, n_noise)) + DC
    elif kind in ("tilt_strong", "tilt_dominant"):
        a, b = 5 * hop, 9 * hop
        noise[a:b] = _shaped(rng, b - a, _tilt_for(fs, kind == "tilt_dominant")) * _amp(FLOOR_DB) + DC
    elif kind in ("quieter_15", "quieter_9", "louder_16", "louder_25"):
        noise = (noise - DC) * _amp({"quieter_15": -16.0, "quieter_9": -9.0, "louder_16": 16.0, "louder_25": 25.0}[kind]) + DC
    elif kind == "voice_non_finite":
        voice[3], voice[n_voice // 2] = np.nan, -np.inf
    return noise.astype(np.float32), None if voice is None else voice.astype(np.float32)


def _metadata(kind: str, fs: int, age):
    """(noise metadata, voice metadata) as the reference takes them, or (None, None)."""
    a, b = {}, {}
    if kind in METADATA:
        sub = {"fs": fs, "fs+1": fs + 1}
        a = {k: sub.get(v, v) if isinstance(v, str) and v.startswith("fs") else v for k, v in METADATA[kind][0].items()}
        b = {k: sub.get(v, v) if isinstance(v, str) and v.startswith("fs") else v for k, v in METADATA[kind][1].items()}
    if age is not None:
        a["captured_at_unix_s"], b["captured_at_unix_s"] = 1_700_000_000.0 - min(age, 0.0), 1_700_000_000.0 + max(age, 0.0)
    return (a or None), (b or None)


def _vad_pair(kind: str, n_noise_vad: int, n_voice_vad: int, seed: int):
    rng = np.random.default_rng(31 * seed + 5)
    nv = 0.03 + 0.04 * rng.random(n_noise_vad)
    sv = 0.05 + 0.1 * rng.random(n_voice_vad)
    pos = (np.arange(n_voice_vad) + 0.5) / n_voice_vad * (VOICE_FRAMES + 1)  # in hops
    sv[((pos >= 2.5) & (pos < 8.5)) | ((pos >= 10.5) & (pos < 16.5)) | ((pos >= 18.5) & (pos < 23.5))] = 0.9
    if kind == "vad_speech_present":
        nv[: (2 * n_noise_vad) // 5] = 0.8
    elif kind == "vad_possible_speech":
        nv[-2:] = 0.8
    elif kind == "vad_too_few_frames":
        sv[:] = 0.9
        sv[:2] = 0.1
    return nv, sv


@functools.lru_cache(maxsize=None)
def batches() -> tuple:
    """Every batch: dict(name, fs, kinds, noise [B, n], speech [B, m] | None, noise_vad, speech_vad [B, .] | None, age [B] (NaN:
    unknown), mismatch [B] uint32, metadata [(noise, voice)] per stream)."""
    out = []

    def add(name, fs, kinds, n_noise, n_voice, vad=False):
        B = len(kinds)
        pairs = [_pair(kind, fs, s, n_noise, n_voice) for s, kind in enumerate(kinds)]
        ages = [AGES.get(kind) for kind in kinds]
        item = dict(name=name, fs=fs, kinds=tuple(kinds), noise=np.stack([p[0] for p in pairs]),
                    speech=np.stack([p[1] for p in pairs]) if n_voice else None, noise_vad=None, speech_vad=None,
                    age=np.array([np.nan if a is None else a for a in ages]),
                    mismatch=np.array([MISMATCH_BITS.get(kind, 0) for kind in kinds], dtype=np.uint32),
                    metadata=[_metadata(kind, fs, age) for kind, age in zip(kinds, ages)])
        if vad:
            v = [_vad_pair(kind, 11, 31, s) for s, kind in enumerate(kinds)]
            item["noise_vad"], item["speech_vad"] = np.stack([p[0] for p in v]), np.stack([p[1] for p in v])
        assert B == item["noise"].shape[0]
        out.append(item)

    for fs in RATES:
        N = frame_size(fs)
        hop = N // 2
        kinds = MAIN_48K if fs == 48_000 else [MAIN_KINDS[s % len(MAIN_KINDS)] for s in range(MAIN_STREAMS[fs])]
        add(f"main@{fs}", fs, kinds, N + (NOISE_FRAMES - 1) * hop, N + (VOICE_FRAMES - 1) * hop + 5)
    for fs in (3150, 4410):
        N = frame_size(fs)
        add(f"vad@{fs}", fs, VAD_KINDS, N + (NOISE_FRAMES - 1) * (N // 2) + 3, N + (VOICE_FRAMES - 1) * (N // 2), vad=True)
    N = frame_size(2560)
    add("short@2560", 2560, ("usable", "louder_16"), N + 11 * (N // 2), N + (VOICE_FRAMES - 1) * (N // 2))
    add("no_voice@3000", 3000, ("usable", "ramp_questionable", "maybe_stale"), 600 + 14 * 300 + 7, 0)
    add("sub_frame@3150", 3150, ("usable", "steady_voice", "quieter_15"), 630 // 2 + 3, 630 + 23 * 315)
    add("sub_frame@2560", 2560, ("usable",), 1, N + (VOICE_FRAMES - 1) * (N // 2))
    return tuple(out)


def batch(name: str) -> dict:
    return next(b for b in batches() if b["name"] == name)


def margins(metrics: dict, speech_frame_rms=None, speech_posteriors=None, noise_posteriors=None) -> float:
    """How far the decision quantities of one stream stay from the thresholds of :315-470 and the cuts of :252-277: the
    smallest |quantity - threshold| over every comparison the stream can reach (None / NaN quantities are skipped)."""
    table = (("duration_s", (1.5,)), ("noise_rms_db", (-95.0,)), ("zero_fraction", (0.995,)), ("noise_peak_db", (-90.0,)),
             ("clipped_fraction", (0.001,)), ("rms_spread_db", (12.0, 6.0)), ("octave_stability_db", (14.0, 8.0)),
             ("spectral_flux_db", (10.0, 6.0)), ("crest_factor_db", (24.0,)), ("vad_contamination_ratio", (0.30, 0.08)),
             ("vad_contamination_p90", (0.55,)), ("capture_age_s", (600.0, 120.0)),
             ("in_capture_level_delta_db", (12.0, 6.0, -20.0, -12.0)), ("spectral_shape_distance_db", (10.0, 5.5)))
    worst = np.inf
    for key, cuts in table:
        value = metrics.get(key)
        if value is None or np.isnan(value):
            continue
        worst = min(worst, min(abs(float(value) - c) for c in cuts))
    if noise_posteriors is not None:
        worst = min(worst, float(np.min(np.abs(np.asarray(noise_posteriors) - 0.35))))
    if speech_frame_rms is not None and len(speech_frame_rms) >= 4:
        rms = np.asarray(speech_frame_rms, dtype=np.float64)
        if speech_posteriors is not None:
            worst = min(worst, float(np.min(np.abs(np.asarray(speech_posteriors) - 0.25))))
            cut = float(np.percentile(rms, 35.0))
        else:
            spread = float(np.percentile(rms, 90.0) - np.percentile(rms, 10.0))
            worst = min(worst, abs(spread - 6.0))
            cut = float(np.percentile(rms, 15.0))
        others = np.abs(rms - cut)
        worst = min(worst, float(np.min(others[others > 0.0])) if np.any(others > 0.0) else np.inf)  # the cut itself may be a level
    return worst


_FIXTURE = None


def fixture():
    """tests/golden/noise_reference.npz, loaded once and shared."""
    global _FIXTURE
    if _FIXTURE is None:
        import pathlib

        with np.load(pathlib.Path(__file__).resolve().parent / "golden" / "noise_reference.npz", allow_pickle=False) as z:
            _FIXTURE = {k: z[k] for k in z.files}
    return _FIXTURE
