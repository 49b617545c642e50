"""ctypes front of tests/ref/voice_spectrum_ref.c: the reference's voice spectrum measurement (spectrum.py:69-343, 519-645,
839-967) in the kernels' operation order, one stream per call.  Used by the tests only (CPU side of a comparison)."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "ref" / "voice_spectrum_ref.c"
LIB = HERE / "ref" / "libvoice_spectrum_ref.so"
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=c11", "-Wall", "-Wextra"]

NOISE_SOURCES = ("unavailable", "explicit_capture", "in_capture_non_speech")  # spectrum.py:553, 577, 586
SPECTRA = ("speech_db", "noise_db", "spectral_snr_db", "welch_db")


class Row(C.Structure):
    _fields_ = [("frames", C.c_int32), ("voiced", C.c_int32), ("voiced_window_ratio", C.c_double),
                ("vad_probability_used", C.c_int32), ("vad_active_window_ratio", C.c_double),
                ("noise_reference_source", C.c_int32), ("used_single_spectrum_fallback", C.c_int32),
                ("welch_segments", C.c_int32)]


def build(force: bool = False) -> pathlib.Path:
    """Compile the restatement next to its source (git-ignored) unless it is there and newer than the source."""
    if force or not LIB.exists() or LIB.stat().st_mtime < SRC.stat().st_mtime:
        subprocess.run(["gcc", *CFLAGS, "-shared", "-o", str(LIB), str(SRC), "-lm"], check=True)
    return LIB


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(str(build()))
        dp, fp, i, i64 = C.POINTER(C.c_double), C.POINTER(C.c_float), C.c_int, C.c_int64
        L.vsr_analyze.restype = i
        L.vsr_analyze.argtypes = [fp, i64, dp, i64, fp, i64, i, i, C.POINTER(Row), dp, dp, C.POINTER(C.c_uint8)] + [dp] * 9
        L.vsr_octave_bands.restype = i
        L.vsr_octave_bands.argtypes = [i, dp, dp, dp]
        L.vsr_freqs.restype = None
        L.vsr_freqs.argtypes = [i, i, dp]
        L.vsr_smooth.restype = None
        L.vsr_smooth.argtypes = [dp, i, i, dp]
        _LIB = L
    return _LIB


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def freqs(fs: int, nperseg: int) -> np.ndarray:
    f = np.zeros(nperseg // 2 + 1)
    lib().vsr_freqs(fs, nperseg, _dp(f))
    return f


def octave_bands(fraction: int):
    c, lo, up = np.zeros(256), np.zeros(256), np.zeros(256)
    n = lib().vsr_octave_bands(fraction, _dp(c), _dp(lo), _dp(up))
    return c[:n].copy(), lo[:n].copy(), up[:n].copy()


def smooth(db: np.ndarray, fs: int, nperseg: int) -> np.ndarray:
    db = np.ascontiguousarray(db, dtype=np.float64)
    out = np.zeros_like(db)
    lib().vsr_smooth(_dp(db), fs, nperseg, _dp(out))
    return out


def analyze(audio, fs: int, nperseg: int, vad=None, noise=None) -> dict:
    """One stream: the fields of af_voice_spectrum_row, the spectra, frame levels, mask, the voiced frames' window spectra
    and the gate levels the decisions compared against."""
    a = np.ascontiguousarray(audio, dtype=np.float32)
    if a.size < nperseg:
        raise ValueError(f"Audio too short for FFT: need {nperseg} samples, got {a.size} ({a.size / fs:.2f} seconds)")
    K, F = nperseg // 2 + 1, (a.size - nperseg) // (nperseg // 2) + 1
    fp = C.POINTER(C.c_float)
    v = None if vad is None else np.ascontiguousarray(vad, dtype=np.float64)
    z = None if noise is None else np.ascontiguousarray(noise, dtype=np.float32)
    row = Row()
    out = {k: np.zeros(K) for k in SPECTRA + ("welch_sum",)}
    out.update(frame_power=np.zeros(F), frame_rms_db=np.zeros(F), voiced_mask=np.zeros(F, dtype=np.uint8), gates=np.zeros(4))
    win = [np.zeros((F, K)) for _ in range(3)]
    rc = lib().vsr_analyze(a.ctypes.data_as(fp), a.size, None if v is None else _dp(v), 0 if v is None else v.size,
                           None if z is None else z.ctypes.data_as(fp), 0 if z is None else z.size, fs, nperseg, C.byref(row),
                           _dp(out["frame_power"]), _dp(out["frame_rms_db"]), out["voiced_mask"].ctypes.data_as(C.POINTER(C.c_uint8)),
                           _dp(out["speech_db"]), _dp(out["noise_db"]), _dp(out["spectral_snr_db"]), _dp(out["welch_db"]),
                           _dp(out["welch_sum"]), _dp(win[0]), _dp(win[1]), _dp(win[2]), _dp(out["gates"]))
    assert rc == 0
    for name, _ in Row._fields_:
        out[name] = getattr(row, name)
    out["win_linear"], out["win_db"], out["win_smooth"] = (w[: row.voiced].copy() for w in win)
    return out
