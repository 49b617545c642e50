"""ctypes front of tests/ref/voice_reliability_ref.c: the second half of the reference's analyze_voice_spectrum
(spectrum.py:647-742 with :250-290 and :381-495) in the kernels' operation order, one stream per call, from what
voice_spectrum_oracle.analyze returns.  Used by the tests only (CPU side of a comparison)."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import numpy as np

import voice_spectrum_oracle as VO

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "ref" / "voice_reliability_ref.c"
LIB = HERE / "ref" / "libvoice_reliability_ref.so"
CFLAGS = VO.CFLAGS

SPECTRA = ("median_spectrum_db", "spectral_repeatability", "measurement_uncertainty_db", "spectral_snr_db")
LEVEL_FIELDS = 7


class Row(C.Structure):
    _fields_ = [("snr_db", C.c_double), ("spectral_tilt_db_per_octave", C.c_double), ("residual_confidence", C.c_double),
                ("measurement_coverage", C.c_double), ("outlier_rejection_ratio", C.c_double), ("phonetic_coverage", C.c_double),
                ("effective_measurement_blocks", C.c_double), ("voiced", C.c_int32), ("independent", C.c_int32),
                ("blocks", C.c_int32), ("inliers", C.c_int32), ("used_closest_windows", C.c_int32), ("reserved", C.c_int32)]


SCALARS = tuple(name for name, kind in Row._fields_ if kind is C.c_double)
COUNTS = ("voiced", "independent", "blocks", "inliers", "used_closest_windows")


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
        dp, i = C.POINTER(C.c_double), C.c_int
        L.vrr_analyze.restype = i
        L.vrr_analyze.argtypes = [dp, i, C.POINTER(C.c_int64), dp, i, i, C.POINTER(Row), dp, dp, dp, dp, dp, C.POINTER(C.c_uint8),
                                  dp, dp, dp]
        L.vrr_estimate_snr.restype = C.c_double
        L.vrr_estimate_snr.argtypes = [dp, dp, i, i]
        L.vrr_estimate_tilt.restype = C.c_double
        L.vrr_estimate_tilt.argtypes = [dp, i, i]
        _LIB = L
    return _LIB


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def analyze(smoothed, frame_starts, noise_db, fs: int, nperseg: int) -> dict:
    """One stream of the main branch: smoothed [voiced, bins] rows of the voiced windows, their first samples, the noise
    reference [bins] or None."""
    S = np.ascontiguousarray(smoothed, dtype=np.float64)
    V, K = S.shape
    assert K == nperseg // 2 + 1
    starts = np.ascontiguousarray(frame_starts, dtype=np.int64)
    z = None if noise_db is None else np.ascontiguousarray(noise_db, dtype=np.float64)
    row = Row()
    out = {k: np.zeros(K) for k in SPECTRA}
    out.update(window_distance=np.zeros(V), inlier_mask=np.zeros(V, dtype=np.uint8), levels=np.zeros((V, LEVEL_FIELDS)),
               block_rows=np.zeros((V, K)), stats=np.zeros(4))
    rc = lib().vrr_analyze(_dp(S), V, starts.ctypes.data_as(C.POINTER(C.c_int64)), None if z is None else _dp(z), fs, nperseg,
                           C.byref(row), *(_dp(out[k]) for k in SPECTRA), _dp(out["window_distance"]),
                           out["inlier_mask"].ctypes.data_as(C.POINTER(C.c_uint8)), _dp(out["levels"]), _dp(out["block_rows"]),
                           _dp(out["stats"]))
    assert rc == 0
    for name, _ in Row._fields_:
        out[name] = getattr(row, name)
    out["block_rows"] = out["block_rows"][: row.blocks].copy()
    return out


def from_first_half(first: dict, fs: int, nperseg: int) -> dict:
    """The complete second half of one stream from voice_spectrum_oracle.analyze's result: the main branch through the
    restatement, the fallback return's constants (:620-644) otherwise.  window_distance and inlier_mask are per frame."""
    K, F = nperseg // 2 + 1, int(first["frames"])
    mask = first["voiced_mask"].astype(bool)
    noise = None if np.isnan(first["noise_db"][0]) else first["noise_db"]
    if first["used_single_spectrum_fallback"]:
        welch = np.ascontiguousarray(first["welch_db"])
        out = {"median_spectrum_db": welch.copy(), "spectral_repeatability": np.zeros(K), "measurement_uncertainty_db": np.full(K, np.inf),
               "spectral_snr_db": first["spectral_snr_db"].copy(), "window_distance": np.full(F, np.nan),
               "inlier_mask": np.zeros(F, dtype=np.uint8)}
        out.update(dict.fromkeys(SCALARS, 0.0), **dict.fromkeys(COUNTS, 0))
        out["snr_db"] = lib().vrr_estimate_snr(_dp(welch), None if noise is None else _dp(np.ascontiguousarray(noise)), fs, nperseg)
        out["spectral_tilt_db_per_octave"] = lib().vrr_estimate_tilt(_dp(welch), fs, nperseg)
        out["measurement_coverage"] = 0.45
        return out
    out = analyze(first["win_smooth"], np.flatnonzero(mask) * (nperseg // 2), noise, fs, nperseg)
    distance, inlier = np.full(F, np.nan), np.zeros(F, dtype=np.uint8)
    distance[mask], inlier[mask] = out["window_distance"], out["inlier_mask"]
    out["window_distance"], out["inlier_mask"] = distance, inlier
    return out
