"""ctypes front of tests/ref/setup_verification_ref.c: the measurements of validate_voice_setup_verification
(voice_setup.py:1446-1679) -- adaptive house curve, shape error, repeatability delta, SNR band medians, levels -- through
csrc/af_setup_verification_math.h, one stream per call.  Used by the tests only (CPU side of a comparison)."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import numpy as np

from voice_spectrum_oracle import CFLAGS

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "ref" / "setup_verification_ref.c"
CSRC = HERE.parent / "audio-forge_amd" / "csrc"
SHARED = [CSRC / "af_setup_verification_math.h", CSRC / "af_numpy_rules.h", HERE.parent / "include" / "audioforge_mi.h"]
LIB = HERE / "ref" / "libsetup_verification_ref.so"

PRESETS = ("broadcast", "podcast", "streaming", "flat")
SIGNALS = ("noise", "original", "verification", "rendered", "rendered_noise")
BANDS = ("low", "body", "presence", "sibilance")
SCALARS = ("body_db", "presence_db", "sibilance_db", "tilt_db_per_octave", "low_mid_balance", "flat_scale", "warmth_offset",
           "presence_offset", "sibilance_offset")


class Row(C.Structure):  # af_setup_verification_row
    _fields_ = [("masked_bins", C.c_int32), ("snr_available", C.c_int32), ("band_present", C.c_int32 * 4),
                ("non_finite", C.c_int32 * 5), ("clipped_0999", C.c_int32 * 5), ("clipped_1", C.c_int32 * 5), ("reserved", C.c_int32),
                ("spectral_target_error_before_db", C.c_double), ("spectral_target_error_after_db", C.c_double),
                ("shape_delta_db", C.c_double), ("band_snr_db", C.c_double * 4), ("offsets_before", C.c_double * 5),
                ("offsets_after", C.c_double * 5), ("sum_squares", C.c_double * 5), ("peak", C.c_double * 5), ("rms_db", C.c_double * 5)]


ROW_DTYPE = np.dtype(Row)


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
        L.svr_preset_id.restype, L.svr_preset_id.argtypes = C.c_int, [C.c_char_p]
        L.svr_target_curve.restype, L.svr_target_curve.argtypes = None, [dp, dp, C.c_int, C.c_int, dp, dp]
        L.svr_shape_error_db.restype, L.svr_shape_error_db.argtypes = C.c_double, [dp, dp, C.c_int, C.c_int, dp]
        L.svr_repeatability_delta_db.restype, L.svr_repeatability_delta_db.argtypes = C.c_double, [dp, dp, C.c_int, dp, dp, C.c_int]
        L.svr_snr_band_medians.restype, L.svr_snr_band_medians.argtypes = None, [dp, dp, C.c_int, dp, ip]
        L.svr_sum_squares.restype, L.svr_sum_squares.argtypes = C.c_double, [fp, i64]
        L.svr_rms_db.restype, L.svr_rms_db.argtypes = C.c_double, [C.c_double, i64]
        L.svr_measure_row.restype = None
        L.svr_measure_row.argtypes = [dp, C.c_int, dp, dp, dp, dp, C.c_int, C.POINTER(fp), C.POINTER(i64), C.POINTER(Row)]
        L.svr_reason_text.restype, L.svr_reason_text.argtypes = C.c_char_p, [C.c_int]
        _LIB = L
    return _LIB


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def preset_id(name: str) -> int:
    """AF_TARGET_* of a name; the reference's ValueError for any other (target.py:78-79)."""
    p = lib().svr_preset_id(str(name).encode())
    if p < 0:
        raise ValueError(f"Unknown target preset: {name}")
    return p


def grid(nperseg: int, fs: int = 48_000) -> np.ndarray:
    return np.fft.rfftfreq(nperseg, 1.0 / fs)


def target_curve(freqs, preset: str, measured_db=None):
    """get_target_curve(freqs, preset, measured_db, "adaptive") and the scalars behind its offsets, by name."""
    f = _f64(freqs)
    m = None if measured_db is None else _f64(measured_db)
    out, scalars = np.zeros(f.size), np.zeros(len(SCALARS))
    lib().svr_target_curve(_d(f), None if m is None else _d(m), f.size, preset_id(preset), _d(out), _d(scalars))
    return out, dict(zip(SCALARS, scalars))


def shape_error_db(freqs, db, preset: str):
    """_shape_error_db and the five reported scalars."""
    f, m, scalars = _f64(freqs), _f64(db), np.zeros(5)
    err = lib().svr_shape_error_db(_d(f), _d(m), f.size, preset_id(preset), _d(scalars))
    return float(err), scalars


def repeatability_delta_db(freqs, before_db, original_freqs, original_db) -> float:
    f, b, f0, o = _f64(freqs), _f64(before_db), _f64(original_freqs), _f64(original_db)
    return float(lib().svr_repeatability_delta_db(_d(f), _d(b), f.size, _d(f0), _d(o), f0.size))


def snr_band_medians(freqs, snr_db) -> dict:
    """frequency_dependent_snr_db, voice_setup.py:1634-1645."""
    f = _f64(freqs)
    s = None if snr_db is None else _f64(snr_db)
    medians, present = np.zeros(4), np.zeros(4, dtype=np.int32)
    lib().svr_snr_band_medians(_d(f), None if s is None else _d(s), f.size, _d(medians), present.ctypes.data_as(C.POINTER(C.c_int32)))
    return {name: float(medians[b]) for b, name in enumerate(BANDS) if present[b]}


def sum_squares(x) -> float:
    """np.sum(x.astype(float) ** 2), in NumPy's order."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    return float(lib().svr_sum_squares(a.ctypes.data_as(C.POINTER(C.c_float)), a.size))


def rms_db(x) -> float:
    a = np.ascontiguousarray(x, dtype=np.float32)
    return float(lib().svr_rms_db(sum_squares(a), a.size))


def measure_row(freqs, original_db, before_db, after_db, after_snr_db, preset: str, audio) -> np.ndarray:
    """One stream's af_setup_verification_row as a ROW_DTYPE scalar; ``audio``: five 1-D float32 arrays or None."""
    f, o, b, a = _f64(freqs), _f64(original_db), _f64(before_db), _f64(after_db)
    s = None if after_snr_db is None else _f64(after_snr_db)
    fp = C.POINTER(C.c_float)
    signals = [None if x is None else np.ascontiguousarray(x, dtype=np.float32) for x in audio]
    pointers = (fp * 5)(*[C.cast(None, fp) if x is None else x.ctypes.data_as(fp) for x in signals])
    lengths = (C.c_int64 * 5)(*[0 if x is None else x.size for x in signals])
    row = Row()
    lib().svr_measure_row(_d(f), f.size, _d(o), _d(b), _d(a), None if s is None else _d(s), preset_id(preset), pointers, lengths,
                          C.byref(row))
    return np.frombuffer(bytes(row), dtype=ROW_DTYPE)[0]


# ---- the rules (svm_decide through the restatement's library)
DECISIONS = ("accept", "reduce", "rollback", "retry")


def decide(case: dict) -> dict:
    """One hand-made case of tests/setup_verification_rules_stimulus.py -> the reference's result dict, as far as the rules make it:
    the three keys of an early exit (and simulation_backend when the renderer is not the native one), or every key of :1647-1679."""
    from mic_eq_mi import _lib  # the struct mirrors only; the arithmetic is the restatement library's

    L = lib()
    L.svr_decide.restype, L.svr_decide.argtypes = None, [C.POINTER(Row), C.POINTER(_lib.SetupVerificationEvidence),
                                                         C.POINTER(_lib.SetupVerificationResult)]
    row, e, out = Row(), _lib.SetupVerificationEvidence(), _lib.SetupVerificationResult()
    for k, name in enumerate(SIGNALS):
        row.rms_db[k] = case["rms"][name]
    peak, rendered_peak = float(np.float32(case["peak"])), float(np.float32(case["rendered_peak"]))
    row.non_finite[2], row.clipped_0999[2], row.clipped_1[2] = int(case["non_finite"]), int(peak >= 0.999), int(peak >= 1.0)
    row.clipped_0999[3], row.clipped_1[3] = int(rendered_peak >= 0.999), int(rendered_peak >= 1.0)
    row.spectral_target_error_before_db, row.spectral_target_error_after_db = case["error_before"], case["error_after"]
    row.shape_delta_db = case["shape_delta"]
    settings = {"target_p95_reduction_db": case["compressor"].get("target_p95_reduction_db"),
                "peak_reduction_cap_db": case["compressor"].get("peak_reduction_cap_db"),
                "deesser_max_reduction_db": case["deesser"].get("max_reduction_db")}
    for bit, key in enumerate(_lib.SETUP_EVIDENCE_KEYS):
        value = case["sim"].get(key) if key not in settings else settings[key]
        if value is not None:
            e.present |= 1 << bit
            setattr(e, key, value)
    e.backend_is_rust, e.verification_samples, e.sample_rate = int(case["backend"] == "rust"), case["samples"], 48_000.0
    e.before_snr_db, e.after_snr_db = case["snr_before"], case["snr_after"]
    e.loudness_variation_before_db, e.loudness_variation_after_db = case["spread_before"], case["spread_after"]
    L.svr_decide(C.byref(row), C.byref(e), C.byref(out))
    result = {"decision": DECISIONS[out.decision], "reasons": [L.svr_reason_text(out.reason).decode()], "perceptual_validation": False}
    if out.early_exit:
        if case["backend"] != "rust" and out.reason == _lib.SETUP_REASON_NO_RENDERER:
            result["simulation_backend"] = case["backend"]
        return result
    result.update({name: getattr(out, name) for name, _ in _lib.SetupVerificationResult._fields_[5:-2]})
    result["compressor_gain_reduction_peak_db"] = out.compressor_gain_reduction_peak_db
    result.update(evidence_scope="repeatability_and_exact_native_chain_constraints", frequency_dependent_snr_db={},
                  limiter_activity_events=int(out.limiter_activity_events), clipped=bool(out.clipped), simulation_backend="rust")
    return result


# ---- the offline validation (svm_offline_validation through the restatement's library)
UNCERTAINTY_BITS = 6


def offline_validation(inputs, validation, eq, backend_is_rust: bool = True) -> dict:
    """``inputs``: a row of the fixture's offline/.../inputs; ``validation``: output true peak, compressor peak and p95, de-esser
    peak of the simulated setup passage; ``eq``: the caller's EQ dict or None.  Returns the rules' diagnostics (the noise
    reference's own reasons, which lead the reference's list, are the caller's)."""
    from mic_eq_mi import _lib

    L = lib()
    L.svr_offline_validation.restype, L.svr_offline_validation.argtypes = None, [C.POINTER(_lib.SetupOfflineInputs), C.POINTER(_lib.SetupOfflineResult)]
    L.svr_uncertainty_text.restype, L.svr_uncertainty_text.argtypes = C.c_char_p, [C.c_int]
    i, r = _lib.SetupOfflineInputs(), _lib.SetupOfflineResult()
    (i.capture_confidence, i.speech_dynamic_range_db, i.conservative_noise_rms_db, i.noise_referenced_snr_db, i.active_duration_s,
     i.deesser_frame_evidence_confidence) = (float(v) for v in inputs[:6])
    i.deesser_enabled, i.noise_status_usable = int(inputs[6]), int(inputs[7])
    i.peak_reduction_cap_db, i.target_p95_reduction_db, i.limiter_effective_ceiling_db = float(inputs[8]), float(inputs[9]), float(inputs[10])
    snr = (i.noise_referenced_snr_db - 6.0) / 12.0  # snr_confidence, voice_setup.py:1167 (_clamp)
    i.snr_confidence = max(0.0, min(1.0, snr))
    i.has_eq_settings = int(bool(eq))
    if eq and "analysis_confidence" in eq:
        i.eq_has_analysis_confidence, i.eq_analysis_confidence = 1, float(eq["analysis_confidence"])
    i.eq_apply_recommended = int(bool(eq.get("apply_recommended", True))) if eq else 0
    i.simulation_available, i.backend_is_rust = 1, int(backend_is_rust)
    i.present = (1 << 0) | (1 << 1) | (1 << 2) | (1 << 3) | _lib.SETUP_HAS_DEESSER_PEAK
    i.output_true_peak_db, i.compressor_gain_reduction_db, i.compressor_gain_reduction_p95_db, i.deesser_gain_reduction_db = (
        float(v) for v in validation)
    L.svr_offline_validation(C.byref(i), C.byref(r))
    out = {name: getattr(r, name) for name, _ in _lib.SetupOfflineResult._fields_}
    out["reasons"] = [L.svr_uncertainty_text(b).decode() for b in range(UNCERTAINTY_BITS) if r.uncertainty_reasons >> b & 1]
    return out
