"""ctypes front of tests/ref/speech_features_rates_ref.c: the reference's speech-feature measurement (voice_setup.py:161-458) at
the device rates, in the kernels' operation order, one stream per call -- resample_poly of signal and sample mask included.
Used by the tests only (CPU side of a comparison)."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import numpy as np

from speech_features_oracle import BAND_FIELDS, COUNTS, FEATURES, LEVELS, Row  # noqa: F401  (one row layout for both families)
from voice_spectrum_oracle import CFLAGS

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "ref" / "speech_features_rates_ref.c"
CSRC = HERE.parent / "audio-forge_amd" / "csrc"
SHARED = [CSRC / name for name in ("af_speech_features_math.h", "af_numpy_rules.h")]  # shared with the library
LIB = HERE / "ref" / "libspeech_features_rates_ref.so"

RATES = (16_000, 22_050, 24_000, 32_000, 44_100, 48_000, 88_200, 96_000)
GEOMETRY = ("rate", "frame", "hop", "vad_window", "up", "down", "half", "pre", "rem", "taps")


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
        dp, fp, ip, bp, i64 = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.c_int64
        L.sfq_geometry.argtypes = [i64, ip]
        for name in ("sfq_frames", "sfq_chunks", "sfq_resampled_length"):
            getattr(L, name).restype = i64
            getattr(L, name).argtypes = [i64, i64]
        L.sfq_sibilance_bins.argtypes = [i64]
        L.sfq_sibilance_freqs.restype = None
        L.sfq_sibilance_freqs.argtypes = [i64, dp]
        L.sfq_phase_table.argtypes = [i64, dp]
        L.sfq_resample.argtypes = [i64, fp, i64, bp, dp, bp, ip]
        L.sfq_analyze.argtypes = [i64, fp, i64, C.c_double, dp, i64, fp, i64, dp, C.POINTER(Row), dp, bp, ip, dp, dp,
                                  dp, dp, dp, dp, ip, dp, dp, dp, ip, dp, bp, ip, dp]
        L.sfq_forms_agree_at_48k.argtypes = [dp, C.c_int, dp, i64, C.c_double, dp, i64]
        _LIB = L
    return _LIB


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def geometry(fs: int) -> dict:
    g = np.zeros(len(GEOMETRY), dtype=np.int32)
    if lib().sfq_geometry(fs, _p(g, C.c_int32)) != 0:
        raise ValueError(f"{fs} Hz is not a listed rate")
    return dict(zip(GEOMETRY, (int(v) for v in g)))


def frames(fs: int, n: int) -> int:
    return int(lib().sfq_frames(fs, n))


def chunks(fs: int, n: int) -> int:
    return int(lib().sfq_chunks(fs, n))


def resampled_length(fs: int, n: int) -> int:
    return int(lib().sfq_resampled_length(fs, n))


def sibilance_freqs(fs: int) -> np.ndarray:
    f = np.zeros(lib().sfq_sibilance_bins(fs))
    lib().sfq_sibilance_freqs(fs, _p(f, C.c_double))
    return f


def phase_table(fs: int) -> np.ndarray:
    """[up][taps]: resample_poly's filter as the restatement (and the library) designs it, a row per phase."""
    g = geometry(fs)
    table = np.zeros((g["up"], g["taps"]))
    if lib().sfq_phase_table(fs, _p(table, C.c_double)) != 0:
        raise ValueError("48 kHz is not resampled")
    return table


def resample(fs: int, x, active_frames=None) -> tuple:
    """(signal [n48], mask bytes [n48], counts per chunk of 960) of one capture; active_frames [frames(n)] or None for none."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    F = max(frames(fs, x.size), 0)
    flags = np.zeros(max(F, 1), dtype=np.uint8)
    if active_frames is not None:
        flags[:F] = np.asarray(active_frames, dtype=np.uint8)
    n48 = resampled_length(fs, x.size)
    y, mask, counts = np.zeros(n48), np.zeros(n48, dtype=np.uint8), np.zeros(max(chunks(fs, x.size), 1), dtype=np.int32)
    if lib().sfq_resample(fs, _p(x, C.c_float), x.size, _p(flags, C.c_uint8), _p(y, C.c_double), _p(mask, C.c_uint8),
                          _p(counts, C.c_int32)) != 0:
        raise ValueError(f"{fs} Hz is not resampled")
    return y, mask, counts


def analyze(fs: int, speech, noise_rms_db: float, vad=None, noise=None, model=None) -> dict:
    """One stream at `fs`: speech_features_oracle.analyze's dict, plus resampled, resampled_mask, chunk_counts and
    masked_chunk_energy (what the resampling left; zeros at 48 kHz)."""
    x = np.ascontiguousarray(speech, dtype=np.float32)
    z = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32)
    v = None if vad is None else np.ascontiguousarray(vad, dtype=np.float64)
    w = None if model is None else np.ascontiguousarray(model, dtype=np.float64)
    F, Cn, Fn, S = max(frames(fs, x.size), 0), chunks(fs, x.size), 0 if z is None else frames(fs, z.size), lib().sfq_sibilance_bins(fs)
    n48 = resampled_length(fs, x.size)
    row = Row()
    out = dict(frame_db=np.zeros(F), active_frame_mask=np.zeros(F, dtype=np.uint8), frame_indices=np.zeros(F, dtype=np.int32),
               frame_probabilities=np.zeros(F), frame_feature_rows=np.zeros((F, FEATURES)), frame_power=np.zeros(F),
               chunk_energy=np.zeros(Cn), band_sums=np.zeros((F, BAND_FIELDS)), sibilance_middles=np.zeros((F, 2)),
               sibilance_argmax=np.zeros(F, dtype=np.int32), sibilance_rows=np.zeros((F, S)), noise_band_sums=np.zeros(Fn),
               weighted_sums=np.zeros(S), weighted_argmax=np.zeros(1, dtype=np.int32), resampled=np.zeros(n48),
               resampled_mask=np.zeros(n48, dtype=np.uint8), chunk_counts=np.zeros(Cn, dtype=np.int32), masked_chunk_energy=np.zeros(Cn))
    d, i, b = C.c_double, C.c_int32, C.c_uint8
    rc = lib().sfq_analyze(fs, _p(x, C.c_float), x.size, float(noise_rms_db), None if v is None else _p(v, d), 0 if v is None else v.size,
                           None if z is None else _p(z, C.c_float), 0 if z is None else z.size, None if w is None else _p(w, d),
                           C.byref(row), _p(out["frame_db"], d), _p(out["active_frame_mask"], b), _p(out["frame_indices"], i),
                           _p(out["frame_probabilities"], d), _p(out["frame_feature_rows"], d), _p(out["frame_power"], d),
                           _p(out["chunk_energy"], d), _p(out["band_sums"], d), _p(out["sibilance_middles"], d),
                           _p(out["sibilance_argmax"], i), _p(out["sibilance_rows"], d), _p(out["noise_band_sums"], d),
                           _p(out["weighted_sums"], d), _p(out["weighted_argmax"], i), _p(out["resampled"], d),
                           _p(out["resampled_mask"], b), _p(out["chunk_counts"], i), _p(out["masked_chunk_energy"], d))
    if rc == -1:
        raise ValueError("speech capture is shorter than one analysis frame")
    if rc != 0:
        raise ValueError(f"{fs} Hz is not a listed rate")
    for name, _ in Row._fields_:
        out[name] = getattr(row, name)
    A = out["spectral_frames"]
    for name in ("frame_indices", "frame_probabilities", "frame_feature_rows", "band_sums", "sibilance_middles", "sibilance_argmax",
                 "sibilance_rows"):
        out[name] = out[name][:A]
    out["weighted_argmax"] = int(out["weighted_argmax"][0])
    return out


def forms_agree_at_48k(power, energy, n: int, noise_rms_db: float, vad=None) -> bool:
    """The rate-taking forms of af_speech_features_math.h at 48 kHz against the 48 kHz ones, every bit of the row."""
    p, e = np.ascontiguousarray(power, dtype=np.float64), np.ascontiguousarray(energy, dtype=np.float64)
    v = None if vad is None else np.ascontiguousarray(vad, dtype=np.float64)
    return lib().sfq_forms_agree_at_48k(_p(p, C.c_double), p.size, _p(e, C.c_double), n, float(noise_rms_db),
                                        None if v is None else _p(v, C.c_double), 0 if v is None else v.size) == 0
