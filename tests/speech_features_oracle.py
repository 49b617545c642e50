"""ctypes front of tests/ref/speech_features_ref.c: the reference's speech-feature measurement (voice_setup.py:161-458, 48 kHz)
in the kernels' operation order, one stream per call.  Used by the tests only (CPU side of a comparison)."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import numpy as np

from voice_spectrum_oracle import CFLAGS

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "ref" / "speech_features_ref.c"
CSRC = HERE.parent / "audio-forge_amd" / "csrc"
SHARED = [CSRC / name for name in ("af_speech_features_math.h", "af_voice_setup_math.h", "af_numpy_rules.h")]  # shared with the library
LIB = HERE / "ref" / "libspeech_features_ref.so"

FRAME, HOP, BAND_FIELDS, FEATURES = 1920, 960, 8, 6
COUNTS = ("non_finite", "frames", "active_frames", "spectral_frames", "noise_frames", "vad_probability_used", "short_term_window_count",
          "loudness_window_count", "evidence_available", "reserved")
LEVELS = ("active_duration_s", "active_ratio", "vad_active_frame_ratio", "short_term_lufs", "momentary_lufs", "active_loudness_spread_db",
          "loudness_range_db", "band_low_db", "band_body_db", "band_presence_db", "band_sibilance_db", "sibilance_excess_db", "confidence",
          "frame_probability_p90", "frame_probability_top_mean", "temporal_score", "absolute_hf_strength_p90", "noise_reliability_p90",
          "excess_p90_db", "temporal_contrast_db", "candidate_frame_ratio", "candidate_snr_db", "peak_hz", "adaptive_floor_db")


class Row(C.Structure):
    _fields_ = [(name, C.c_int32) for name in COUNTS] + [(name, C.c_double) for name in LEVELS]


def build(force: bool = False) -> pathlib.Path:
    """Compile the restatement next to its source (git-ignored) unless it is there and newer than its sources."""
    newest = max(p.stat().st_mtime for p in [SRC, *SHARED])
    if force or not LIB.exists() or LIB.stat().st_mtime < newest:
        subprocess.run(["gcc", *CFLAGS, "-shared", "-o", str(LIB), str(SRC), "-lm"], check=True)
    return LIB


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(str(build()))
        dp, fp, ip, i64 = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int64
        L.sfr_sibilance_bins.restype = C.c_int
        L.sfr_sibilance_freqs.restype = None
        L.sfr_sibilance_freqs.argtypes = [dp]
        L.sfr_analyze.restype = C.c_int
        L.sfr_analyze.argtypes = [fp, i64, C.c_double, dp, i64, fp, i64, dp, C.POINTER(Row), dp, C.POINTER(C.c_uint8), ip, dp, dp,
                                  dp, dp, dp, dp, ip, dp, dp, dp, ip]
        _LIB = L
    return _LIB


def frames(n: int) -> int:
    return 0 if n < FRAME else (n - FRAME) // HOP + 1


def chunks(n: int) -> int:
    return -(-n // HOP)


def sibilance_freqs() -> np.ndarray:
    f = np.zeros(lib().sfr_sibilance_bins())
    lib().sfr_sibilance_freqs(f.ctypes.data_as(C.POINTER(C.c_double)))
    return f


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def analyze(speech, noise_rms_db: float, vad=None, noise=None, model=None) -> dict:
    """One stream: the fields of af_speech_features_row, the per-frame arrays (frame_db, active_frame_mask over every frame;
    frame_indices, frame_probabilities, frame_feature_rows over the spectrally active ones) and what the kernels leave."""
    x = np.ascontiguousarray(speech, dtype=np.float32)
    z = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32)
    v = None if vad is None else np.ascontiguousarray(vad, dtype=np.float64)
    w = None if model is None else np.ascontiguousarray(model, dtype=np.float64)
    F, Cn, Fn, S = frames(x.size), chunks(x.size), 0 if z is None else frames(z.size), lib().sfr_sibilance_bins()
    row = Row()
    out = dict(frame_db=np.zeros(F), active_frame_mask=np.zeros(F, dtype=np.uint8), frame_indices=np.zeros(F, dtype=np.int32),
               frame_probabilities=np.zeros(F), frame_feature_rows=np.zeros((F, FEATURES)), frame_power=np.zeros(F),
               chunk_energy=np.zeros(Cn), band_sums=np.zeros((F, BAND_FIELDS)), sibilance_middles=np.zeros((F, 2)),
               sibilance_argmax=np.zeros(F, dtype=np.int32), sibilance_rows=np.zeros((F, S)), noise_band_sums=np.zeros(Fn),
               weighted_sums=np.zeros(S), weighted_argmax=np.zeros(1, dtype=np.int32))
    d, i = C.c_double, C.c_int32
    rc = lib().sfr_analyze(_p(x, C.c_float), x.size, float(noise_rms_db), None if v is None else _p(v, d), 0 if v is None else v.size,
                           None if z is None else _p(z, C.c_float), 0 if z is None else z.size, None if w is None else _p(w, d),
                           C.byref(row), _p(out["frame_db"], d), _p(out["active_frame_mask"], C.c_uint8), _p(out["frame_indices"], i),
                           _p(out["frame_probabilities"], d), _p(out["frame_feature_rows"], d), _p(out["frame_power"], d),
                           _p(out["chunk_energy"], d), _p(out["band_sums"], d), _p(out["sibilance_middles"], d),
                           _p(out["sibilance_argmax"], i), _p(out["sibilance_rows"], d), _p(out["noise_band_sums"], d),
                           _p(out["weighted_sums"], d), _p(out["weighted_argmax"], i))
    if rc != 0:
        raise ValueError("speech capture is shorter than one analysis frame")
    for name, _ in Row._fields_:
        out[name] = getattr(row, name)
    A = out["spectral_frames"]
    for name in ("frame_indices", "frame_probabilities", "frame_feature_rows", "band_sums", "sibilance_middles", "sibilance_argmax",
                 "sibilance_rows"):
        out[name] = out[name][:A]
    out["weighted_argmax"] = int(out["weighted_argmax"][0])
    return out


# ---- the recommendation rules (csrc/af_voice_setup_math.h through the restatement's library)
STATUS = ("usable", "questionable", "invalid")
PROFILES = ("gentle", "balanced", "dense", "custom")
TARGET_LUFS = {"broadcast": -16.0, "streaming": -16.0, "podcast": -17.0, "flat": -18.0}


def _setup_types():
    from mic_eq_mi import _lib  # the struct mirrors only; the arithmetic below is the restatement library's

    return _lib.VoiceSetupInputs, _lib.VoiceSetupRecommendation


def recommend(result: dict, *, freqs, smoothed_spectrum_db, residual_confidence, snr_db, used_single_spectrum_fallback, noise_quality_score,
              noise_status, conservative_noise_rms_db, target_preset="broadcast", vad_available=True, dynamics_intensity="balanced",
              custom_target_p95_db=3.5, custom_peak_cap_db=8.0, enable_probability_threshold=None) -> dict:
    """The rules for one stream's analyze() result: every field of af_voice_setup_recommendation by name."""
    Inputs, Recommendation = _setup_types()
    L = lib()
    row = Row(**{name: result[name] for name, _ in Row._fields_})
    frame_db = np.ascontiguousarray(result["frame_db"], dtype=np.float64)
    mask = np.ascontiguousarray(result["active_frame_mask"], dtype=np.uint8)
    f, db = np.ascontiguousarray(freqs, dtype=np.float64), np.ascontiguousarray(smoothed_spectrum_db, dtype=np.float64)
    inputs, out = Inputs(), Recommendation()
    L.sfr_default_inputs(C.byref(inputs))
    d = C.POINTER(C.c_double)
    inputs.features = C.cast(C.pointer(row), type(inputs.features))
    inputs.frame_db, inputs.active_frame_mask = frame_db.ctypes.data_as(d), mask.ctypes.data_as(C.POINTER(C.c_uint8))
    inputs.freqs, inputs.spectrum_db, inputs.bins = f.ctypes.data_as(d), db.ctypes.data_as(d), f.size
    inputs.used_single_spectrum_fallback = int(used_single_spectrum_fallback)
    inputs.residual_confidence, inputs.snr_db = residual_confidence, snr_db
    inputs.noise_quality_score, inputs.conservative_noise_rms_db = noise_quality_score, conservative_noise_rms_db
    inputs.noise_status, inputs.vad_available = STATUS.index(noise_status), int(vad_available)
    inputs.target_lufs = TARGET_LUFS.get(target_preset, -18.0)
    inputs.dynamics_intensity = PROFILES.index(dynamics_intensity) if dynamics_intensity in PROFILES else 1
    inputs.custom_target_p95_db, inputs.custom_peak_cap_db = custom_target_p95_db, custom_peak_cap_db
    if enable_probability_threshold is not None:
        inputs.enable_probability_threshold = enable_probability_threshold
    L.sfr_recommend(C.byref(inputs), C.byref(out))
    got = {name: getattr(out, name) for name, _ in Recommendation._fields_ if name != "reserved"}
    got["deesser_clip_features"] = np.array(list(out.deesser_clip_features))
    return got
