"""ctypes front of tests/ref/noise_reference_ref.c: the reference's room-noise reference analysis (noise_reference.py:118-546)
in the kernels' operation order, one stream per call.  Used by the tests only (CPU side of a comparison)."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import numpy as np

from voice_spectrum_oracle import CFLAGS

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "ref" / "noise_reference_ref.c"
LIB = HERE / "ref" / "libnoise_reference_ref.so"

STATUS = ("usable", "questionable", "invalid")
# one text per bit of `reasons` / `guidance`, in the order noise_reference.py:315-470 appends them
REASONS = (
    "room-noise capture is too short",
    "room-noise capture contains non-finite samples",
    "room-noise capture is suspiciously silent",
    "room-noise capture is clipped",
    "room-noise capture contains isolated clipped samples",
    "room-noise capture has too few analysis windows",
    "room-noise capture is dominated by changing events",
    "room-noise capture is not stationary",
    "room-noise capture contains dominant transient events",
    "room-noise capture contains strong transients",
    "speech is present in the room-noise capture",
    "possible speech contamination in room-noise capture",
    "input device changed between noise and voice captures",
    "input channel mode changed between noise and voice captures",
    "channel count changed between noise and voice captures",
    "noise capture sample rate does not match analysis",
    "voice capture sample rate does not match analysis",
    "sample rate changed between noise and voice captures",
    "room-noise reference is stale",
    "room-noise reference may be stale",
    "room noise does not match conditions during the voice capture",
    "room-noise reference only partly matches the voice capture",
    "room-noise level changed substantially before the voice capture",
    "room-noise reference is much louder than in-capture quiet frames",
)
GUIDANCE = (
    "Record at least 1.5 seconds of room tone.",
    "Restart the audio stream and record the room tone again.",
    "Check the selected microphone and record normal room tone again.",
    "Lower input gain or remove the transient source, then recapture.",
    "Recapture without taps or handling noise for a cleaner reference.",
    "Wait for the room to settle and record a new reference.",
    "Avoid movement, speech, and intermittent sounds while recapturing.",
    "Recapture without keyboard, handling, or impact sounds.",
    "Remain silent and record the room noise again.",
    "Record another room-noise sample without voices.",
    "Use the same microphone, channel mode, and sample rate for both captures.",
    "Record room noise immediately before the voice sample.",
    "Recapture room noise under the current conditions.",
    "Recapture room noise and voice without changing the environment.",
    "Recapture both samples for a more reliable correction.",
    "Record room noise and voice under the same conditions.",
    "Check whether the noise source changed between captures.",
)
METRICS = ("duration_s", "finite_fraction", "noise_rms_db", "conservative_noise_rms_db", "noise_peak_db", "crest_factor_db",
           "clipped_fraction", "zero_fraction", "rms_spread_db", "octave_stability_db", "spectral_flux_db", "vad_contamination_ratio",
           "vad_contamination_p90", "capture_age_s", "in_capture_level_delta_db", "spectral_shape_distance_db")
SPECTRA = ("explicit_spectrum_db", "conservative_spectrum_db", "in_capture_spectrum_db")


class Row(C.Structure):
    _fields_ = ([("status", C.c_int32), ("conservative", C.c_int32), ("reasons", C.c_uint32), ("guidance", C.c_uint32),
                 ("quality_score", C.c_double)]
                + [(name, C.c_double) for name in METRICS + ("noise_sum_squares", "noise_peak")]
                + [(name, C.c_int64) for name in ("finite_samples", "clipped_samples", "zero_samples")]
                + [(name, C.c_int32) for name in ("in_capture_noise_frame_count", "noise_frames", "speech_frames", "n_bands",
                                                  "has_in_capture_spectrum", "reserved")])


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
        L.nrr_frame_size.restype = i
        L.nrr_frame_size.argtypes = [i]
        L.nrr_plan.restype = i
        L.nrr_plan.argtypes = [i, C.POINTER(i)]
        L.nrr_freqs.restype = None
        L.nrr_freqs.argtypes = [i, i, dp]
        L.nrr_analyze.restype = i
        L.nrr_analyze.argtypes = ([fp, i64, fp, i64, dp, i64, dp, i64, C.c_double, C.c_uint32, i, C.POINTER(Row)] + [dp] * 12
                                  + [C.POINTER(C.c_uint8)])
        _LIB = L
    return _LIB


def frame_size(fs: int) -> int:
    return int(lib().nrr_frame_size(int(fs)))


def plan(fs: int):
    """The factors of half the frame in the order the transform takes them, or None when it does not take the frame."""
    N = frame_size(fs)
    if N % 2:
        return None
    factors = (C.c_int * 16)()
    n = lib().nrr_plan(N // 2, factors)
    return None if n < 0 else list(factors[:n])


def frames(fs: int, n: int) -> int:
    N = frame_size(fs)
    return 0 if n < N else (n - N) // (N // 2) + 1


def bins(fs: int, n_noise: int) -> int:
    N = frame_size(fs)
    return N // 2 + 1 if n_noise >= N else max(2, n_noise) // 2 + 1


def texts(mask: int, table) -> list[str]:
    return [text for bit, text in enumerate(table) if mask >> bit & 1]


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def analyze(noise, speech, fs: int, noise_vad=None, speech_vad=None, age=float("nan"), mismatch: int = 0) -> dict:
    """One stream: the fields of af_noise_reference_row, the three spectra on the returned grid, the frame levels and band
    levels of the noise capture, what the kernels leave (chunk sums, frame powers, PSD rows, band sums, the medians' middles)
    and the quiet-frame mask of the voice capture."""
    fp = C.POINTER(C.c_float)
    z = np.ascontiguousarray(noise, dtype=np.float32)
    v = None if speech is None else np.ascontiguousarray(speech, dtype=np.float32)
    nv = None if noise_vad is None else np.ascontiguousarray(noise_vad, dtype=np.float64)
    sv = None if speech_vad is None else np.ascontiguousarray(speech_vad, dtype=np.float64)
    K, Ko = frame_size(fs) // 2 + 1, bins(fs, z.size)
    F, Fv = frames(fs, z.size), 0 if v is None else frames(fs, v.size)
    row = Row()
    out = {name: np.zeros(Ko) for name in SPECTRA}
    out.update(frame_rms_db=np.zeros(F), band_levels_db=np.zeros((F, 7)), noise_chunk_sums=np.zeros((F + 1 if F else 0, 2)),
               noise_frame_power=np.zeros(F), speech_frame_power=np.zeros(Fv), noise_psd=np.zeros((F, K)), band_power=np.zeros((F, 7)),
               explicit_middles=np.zeros((2, K)), in_capture_middles=np.zeros((2, K)), quiet_mask=np.zeros(Fv, dtype=np.uint8))
    rc = lib().nrr_analyze(z.ctypes.data_as(fp), z.size, None if v is None else v.ctypes.data_as(fp), 0 if v is None else v.size,
                           None if nv is None else _dp(nv), 0 if nv is None else nv.size, None if sv is None else _dp(sv),
                           0 if sv is None else sv.size, float(age), int(mismatch), int(fs), C.byref(row),
                           *(_dp(out[name]) for name in SPECTRA + ("frame_rms_db", "band_levels_db", "noise_chunk_sums",
                                                                   "noise_frame_power", "speech_frame_power", "noise_psd",
                                                                   "band_power", "explicit_middles", "in_capture_middles")),
                           out["quiet_mask"].ctypes.data_as(C.POINTER(C.c_uint8)))
    if rc != 0:
        raise NotImplementedError(f"sample rate {fs} Hz: the transform does not take the analysis frame")
    for name, _ in Row._fields_:
        out[name] = getattr(row, name)
    out["frequencies"] = np.zeros(Ko)
    lib().nrr_freqs(int(fs), frame_size(fs) if F else max(2, z.size), _dp(out["frequencies"]))
    return out
