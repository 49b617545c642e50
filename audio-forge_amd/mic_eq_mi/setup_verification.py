"""Second-passage verification, the measurements (python/mic_eq/analysis/voice_setup.py:1446-1679).

``validate_voice_setup_verification`` renders a second passage and the room tone through the recommended chain and then measures
both sides.  The spectra and the speech features have operators of their own (``analyze_voice_spectrum_batch``,
``measure_speech_features_batch``); what this module adds is the rest of the measuring, on the device, for a batch of streams:
``_shape_error_db`` against the adaptive house curve before and after, the repeatability delta against the setup passage, the
band medians of the rendered side's spectral SNR, and the levels and clipped tests of the five signals
(csrc/af_setup_verification.hip), and the accept / reduce / rollback / retry rules on top of these numbers
(``decide_voice_setup_verification``), and the operator that renders the passages and runs all of it in the reference's
order (``verify_voice_setup_batch``, ``validate_voice_setup_verification``).
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import numpy as np

from . import _lib
from ._lib import SETUP_SIGNALS, TARGET_PRESETS, SetupVerificationAudio, SetupVerificationRow

ROW_DTYPE = np.dtype(SetupVerificationRow)
assert ROW_DTYPE.itemsize == C.sizeof(SetupVerificationRow)
SNR_BANDS = ("low", "body", "presence", "sibilance")  # voice_setup.py:1637-1642
OFFSET_SCALARS = ("body_db", "presence_db", "sibilance_db", "tilt_db_per_octave", "low_mid_balance")  # target.py:24-43


def preset_ids(target_preset, n_streams: int) -> np.ndarray:
    """One name or one per stream -> AF_TARGET_* ids; an unknown name is the reference's ValueError (target.py:78-79)."""
    names = [target_preset] * n_streams if isinstance(target_preset, str) else list(target_preset)
    if len(names) != n_streams:
        raise ValueError(f"expected one target preset or one per stream ({n_streams}), got {len(names)}")
    for name in names:
        if name not in TARGET_PRESETS:
            raise ValueError(f"Unknown target preset: {name}")
    return np.array([TARGET_PRESETS.index(name) for name in names], dtype=np.int32)


def _signal(value, n_streams: int):
    """[streams, n] float32, or one 1-D array per stream (zero-extended to the longest) -> (array, per-stream lengths or None)."""
    if value is None:
        return None, None
    if isinstance(value, np.ndarray) and value.ndim == 2:
        rows, lengths = np.ascontiguousarray(value, dtype=np.float32), None
    else:
        parts = [np.asarray(v, dtype=np.float32).reshape(-1) for v in value]
        lengths = np.array([p.size for p in parts], dtype=np.int64)
        rows = np.zeros((len(parts), int(lengths.max()) if len(parts) else 0), dtype=np.float32)
        for row, part in zip(rows, parts):
            row[:part.size] = part
    if rows.shape[0] != n_streams:
        raise ValueError(f"expected {n_streams} streams of audio, got {rows.shape[0]}")
    return rows, lengths


class SetupVerification:
    """The measurement kernels for up to ``max_streams`` streams on one spectrum grid (af_setup_verification_*)."""

    def __init__(self, sample_rate: int = 48_000, nperseg: int = 4096, max_streams: int = 64, device: int = 0):
        self._lib = _lib.load()
        handle = C.c_void_p()
        _lib.check(self._lib.af_setup_verification_create(int(sample_rate), int(nperseg), int(max_streams), int(device), C.byref(handle)))
        self._h = handle
        self.sample_rate, self.nperseg, self.max_streams = int(sample_rate), int(nperseg), int(max_streams)
        self.bins = self.nperseg // 2 + 1

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_setup_verification_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def measure(self, original_db, before_db, after_db, target_preset, after_snr_db=None, *, noise=None, original=None,
                verification=None, rendered=None, rendered_noise=None) -> np.ndarray:
        """Median spectra [streams, nperseg / 2 + 1] in dB of the setup passage, the verification passage and the rendered one, the
        rendered side's spectral SNR or None, and any of the five signals ([streams, n] float32 or one 1-D array per stream).
        Returns one ROW_DTYPE record per stream."""
        spectra = [np.ascontiguousarray(a, dtype=np.float64) for a in (original_db, before_db, after_db)]
        if any(a.ndim != 2 or a.shape != spectra[0].shape or a.shape[1] != self.bins for a in spectra):
            raise ValueError(f"expected three spectra of shape [streams, {self.bins}]")
        B = spectra[0].shape[0]
        snr = None if after_snr_db is None else np.ascontiguousarray(after_snr_db, dtype=np.float64)
        if snr is not None and snr.shape != spectra[0].shape:
            raise ValueError(f"expected a spectral SNR of shape [streams, {self.bins}]")
        ids = preset_ids(target_preset, B)
        audio, keep = (SetupVerificationAudio * len(SETUP_SIGNALS))(), []
        for k, value in enumerate((noise, original, verification, rendered, rendered_noise)):
            rows, lengths = _signal(value, B)
            if rows is None:
                continue
            keep += [rows, lengths]
            audio[k].samples, audio[k].stride, audio[k].length = rows.ctypes.data, rows.shape[1], rows.shape[1]
            if lengths is not None:
                audio[k].lengths = lengths.ctypes.data_as(C.POINTER(C.c_int64))
        out = np.zeros(B, dtype=ROW_DTYPE)
        dp = C.POINTER(C.c_double)
        _lib.check(self._lib.af_setup_verification_measure_host(
            self._h, B, spectra[0].ctypes.data_as(dp), spectra[1].ctypes.data_as(dp), spectra[2].ctypes.data_as(dp), self.bins,
            None if snr is None else snr.ctypes.data_as(dp), self.bins, ids.ctypes.data_as(C.POINTER(C.c_int32)), audio,
            out.ctypes.data_as(C.POINTER(SetupVerificationRow))))
        return out

    def measure_device(self, n_streams: int, original_db: int, before_db: int, after_db: int, spectrum_stride: int, target_preset,
                       after_snr_db: int = 0, snr_stride: int = 0, audio: Sequence | None = None, rows: int = 0, stream: int = 0) -> None:
        """As ``measure`` over device pointers (integers); ``audio``: up to five (pointer, stride, length, lengths or None), a
        None entry for an absent signal; ``rows``: device memory for ``n_streams`` ROW_DTYPE records.  Enqueues on ``stream``."""
        ids = preset_ids(target_preset, int(n_streams))
        signals, keep = (SetupVerificationAudio * len(SETUP_SIGNALS))(), []
        for k, entry in enumerate(audio or ()):
            if entry is None:
                continue
            pointer, stride, length, lengths = entry
            signals[k].samples, signals[k].stride, signals[k].length = int(pointer), int(stride), int(length)
            if lengths is not None:
                keep.append(np.ascontiguousarray(lengths, dtype=np.int64))
                if keep[-1].size != int(n_streams):
                    raise ValueError(f"expected {int(n_streams)} lengths, got {keep[-1].size}")
                signals[k].lengths = keep[-1].ctypes.data_as(C.POINTER(C.c_int64))
        _lib.check(self._lib.af_setup_verification_measure_device(
            self._h, int(n_streams), C.c_void_p(original_db), C.c_void_p(before_db), C.c_void_p(after_db), int(spectrum_stride),
            C.c_void_p(after_snr_db or None), int(snr_stride), ids.ctypes.data_as(C.POINTER(C.c_int32)), signals, C.c_void_p(rows),
            C.c_void_p(stream or None)))


def row_to_dict(row) -> dict:
    """One record under the reference's key names where it has them (voice_setup.py:1647-1679)."""
    out = {
        "spectral_target_error_before_db": float(row["spectral_target_error_before_db"]),
        "spectral_target_error_after_db": float(row["spectral_target_error_after_db"]),
        "shape_delta_db": float(row["shape_delta_db"]),
        "frequency_dependent_snr_db": {name: float(row["band_snr_db"][b]) for b, name in enumerate(SNR_BANDS) if row["band_present"][b]},
        "adaptive_offsets_before": dict(zip(OFFSET_SCALARS, map(float, row["offsets_before"]))),
        "adaptive_offsets_after": dict(zip(OFFSET_SCALARS, map(float, row["offsets_after"]))),
        "levels": {},
    }
    for k, name in enumerate(SETUP_SIGNALS):
        out["levels"][name] = {"rms_db": float(row["rms_db"][k]), "peak": float(row["peak"][k]), "sum_squares": float(row["sum_squares"][k]),
                               "non_finite": bool(row["non_finite"][k]), "clipped_0999": bool(row["clipped_0999"][k]),
                               "clipped": bool(row["clipped_1"][k])}
    return out


def measure_setup_verification_batch(original_db, before_db, after_db, fs: int, target_preset, after_snr_db=None, *, noise=None,
                                     original=None, verification=None, rendered=None, rendered_noise=None, device: int = 0) -> list[dict]:
    """The measurements of one batch as dicts (``row_to_dict``); the grid is the one of the spectra's bin count at ``fs``."""
    bins = np.asarray(before_db).shape[-1]
    if int(fs) != 48_000:
        raise NotImplementedError(f"sample rate {fs}: the second-passage verification is built for 48000 Hz")
    B = np.asarray(before_db).shape[0]
    handle = SetupVerification(int(fs), 2 * (bins - 1), max(B, 1), device)
    try:
        rows = handle.measure(original_db, before_db, after_db, target_preset, after_snr_db, noise=noise, original=original,
                              verification=verification, rendered=rendered, rendered_noise=rendered_noise)
    finally:
        handle.close()
    return [row_to_dict(row) for row in rows]


def decide_voice_setup_verification(row, simulation, setup_result, *, verification_samples: int, sample_rate: float = 48_000.0,
                                    before_snr_db: float, after_snr_db: float, loudness_variation_before_db: float,
                                    loudness_variation_after_db: float) -> dict:
    """The rules of validate_voice_setup_verification (voice_setup.py:1484-1495, :1590-1679) for one stream: a measured record
    (``SetupVerification.measure``), the simulation dict of the rendered verification passage (``simulate_auto_eq_chain_batch``;
    a missing key takes the reference's default), the setup result (``compressor_settings`` / ``deesser_settings``, or the
    ``compressor`` / ``deesser`` of a ``recommend_voice_chain_batch`` record), the SNR of the two spectra and the
    active_loudness_spread_db of the two feature runs.  Returns the reference's dict: three keys for an early exit."""
    lib = _lib.load()
    compressor = setup_result.get("compressor_settings") or setup_result.get("compressor") or {}
    deesser = setup_result.get("deesser_settings") or setup_result.get("deesser") or {}
    values = dict(simulation)
    values.update(target_p95_reduction_db=compressor.get("target_p95_reduction_db"), peak_reduction_cap_db=compressor.get("peak_reduction_cap_db"),
                  deesser_max_reduction_db=deesser.get("max_reduction_db"))
    record = np.zeros(1, dtype=ROW_DTYPE)
    record[0] = row
    evidence, out = _lib.SetupVerificationEvidence(), _lib.SetupVerificationResult()
    for bit, key in enumerate(_lib.SETUP_EVIDENCE_KEYS):
        if values.get(key) is not None:
            evidence.present |= 1 << bit
            setattr(evidence, key, int(values[key]) if key == "true_peak_limited_events" else float(values[key]))
    backend = simulation.get("simulation_backend", "unavailable")
    evidence.backend_is_rust = int(backend == "rust")
    evidence.verification_samples, evidence.sample_rate = int(verification_samples), float(sample_rate)
    evidence.before_snr_db, evidence.after_snr_db = float(before_snr_db), float(after_snr_db)
    evidence.loudness_variation_before_db, evidence.loudness_variation_after_db = float(loudness_variation_before_db), float(loudness_variation_after_db)
    _lib.check(lib.af_setup_verification_decide(record.ctypes.data_as(C.POINTER(SetupVerificationRow)), C.byref(evidence), C.byref(out)))
    result = {"decision": _lib.SETUP_DECISIONS[out.decision], "reasons": [lib.af_setup_verification_reason_text(out.reason).decode()],
              "perceptual_validation": False}
    if out.early_exit:
        if not evidence.backend_is_rust and out.reason == _lib.SETUP_REASON_NO_RENDERER:  # :1532-1537
            result["simulation_backend"] = backend
        return result
    measured = row_to_dict(record[0])
    result.update({name: getattr(out, name) for name, ctype in _lib.SetupVerificationResult._fields_ if ctype is C.c_double})
    del result["level_difference_db"], result["shape_delta_db"]
    result.update(evidence_scope="repeatability_and_exact_native_chain_constraints",
                  frequency_dependent_snr_db=measured["frequency_dependent_snr_db"], limiter_activity_events=int(out.limiter_activity_events),
                  clipped=bool(out.clipped), simulation_backend=backend)
    return result


# ---- the operator: render, spectra, features, measurement, rules (voice_setup.py:1468-1679)
SPEECH_MIN_DURATION_S = 3.0  # voice_setup.py:43
NPERSEG = 4096               # analyze_voice_spectrum's default, spectrum.py:498-501
EQ_FREQUENCIES = (80.0, 160.0, 320.0, 640.0, 1280.0, 2500.0, 5000.0, 8000.0, 12000.0, 16000.0)  # config_parts/settings.py:11-22
_VERIFICATION_LIMITER = {"limiter_enabled": True, "limiter_ceiling_db": -1.5, "limiter_release_ms": 80.0,
                         "limiter_careful_output_enabled": True}  # :1507-1512
# auto_eq_parts/headroom.py:53-76: the flat key of every de-esser and compressor setting with its default
_DEESSER_KEYS = (("enabled", False), ("auto_enabled", True), ("auto_amount", 0.5), ("low_cut_hz", 4000.0), ("high_cut_hz", 11000.0),
                 ("threshold_db", -28.0), ("ratio", 4.0), ("attack_ms", 2.0), ("release_ms", 80.0), ("max_reduction_db", 6.0))
_COMPRESSOR_KEYS = (("enabled", True), ("threshold_db", -20.0), ("ratio", 4.0), ("attack_ms", 10.0), ("release_ms", 200.0),
                    ("makeup_gain_db", 0.0), ("adaptive_release", False), ("base_release_ms", 50.0), ("auto_makeup_enabled", False),
                    ("target_lufs", -18.0), ("sidechain_highpass_enabled", True))


def _chain_of(setup_result) -> tuple[list, dict, dict, dict]:
    """(bands, flat settings, deesser, compressor) of one setup result: the reference's shape (``eq_settings``, ``deesser_settings``,
    ``compressor_settings``) or a recommend_voice_chain_batch record (``deesser``, ``compressor``, optional ``eq_settings``).  Without
    EQ settings the flat ten bands apply (:1497-1503); the flat keys and defaults are those of auto_eq_parts/headroom.py:42-84."""
    eq = dict(setup_result.get("eq_settings") or {})
    if not eq:
        eq = {"band_freqs": list(EQ_FREQUENCIES), "band_gains": [0.0] * 10, "band_qs": [1.41] * 10}
    freqs, gains, qs = (list(eq.get(key) or []) for key in ("band_freqs", "band_gains", "band_qs"))
    if not (len(freqs) == len(gains) == len(qs) == 10):
        raise ValueError("Auto-EQ settings must contain 10 frequencies, gains, and Q values")
    bands = [(float(f), float(g), float(q)) for f, g, q in zip(freqs, gains, qs)]
    deesser = dict(setup_result.get("deesser_settings") or setup_result.get("deesser") or {})
    compressor = dict(setup_result.get("compressor_settings") or setup_result.get("compressor") or {})
    flat = dict(_VERIFICATION_LIMITER)
    for prefix, source, keys in (("deesser", deesser, _DEESSER_KEYS), ("compressor", compressor, _COMPRESSOR_KEYS)):
        for key, default in keys:
            value = source.get(key)
            flat[f"{prefix}_{key}"] = type(default)(default if value is None else value)
    return bands, flat, deesser, compressor


def _render(audio: np.ndarray, fs: float, bands: list, flats: list, device: int):
    """simulate_auto_eq_chain_batch with per-stream settings.  One engine call takes several presets only when all of them enable
    the same stages, so the streams go in one call per set of enabled stages and come back in the caller's order."""
    from . import mic_eq_core as core

    out = np.empty_like(audio)
    dicts: list = [None] * audio.shape[0]
    groups: dict = {}
    for s, flat in enumerate(flats):
        stages = (flat["deesser_enabled"], flat["compressor_enabled"], flat["compressor_auto_makeup_enabled"])
        groups.setdefault(stages, []).append(s)
    for members in groups.values():
        rendered, simulation = core.simulate_auto_eq_chain_batch(np.ascontiguousarray(audio[members]), fs, [bands[s] for s in members],
                                                                 [flats[s] for s in members], device)
        out[members] = rendered
        for s, d in zip(members, simulation):
            dicts[s] = d
    return out, dicts


def _early_exit(reason: str) -> dict:
    return {"decision": "retry", "reasons": [reason], "perceptual_validation": False}


def verify_voice_setup_batch(noise, original_speech, verification_speech, fs: int, setup_results, target_preset, device: int = 0,
                             _rendered=None) -> list[dict]:
    """validate_voice_setup_verification (voice_setup.py:1468-1679) for every stream of noise [streams, m], original_speech
    [streams, n0] and verification_speech [streams, n] (float32, 48 kHz): the reference's dict per stream, early-exit dicts (three
    keys) included; a stream that exits early does not stop the batch.  ``setup_results``: one mapping or one per stream.

    Order of work: the level kernel and the early exits; one render of the verification passages and one of the room tones through
    simulate_auto_eq_chain_batch with per-stream settings (limiter at -1.5 dB / 80 ms / careful output); the three voice spectra
    (:1541-1551); the measurement kernels; the two speech-feature runs (:1578-1589, energy path, no posteriors); the rules.  The
    rendered audio passes through host memory between the engine and the analyses."""
    from . import mic_eq_core as core

    if int(fs) != 48_000:
        raise NotImplementedError(f"sample rate {fs}: the second-passage verification is built for 48000 Hz")
    noise, original, verification = (np.ascontiguousarray(a, dtype=np.float32) for a in (noise, original_speech, verification_speech))
    if noise.ndim != 2 or original.ndim != 2 or verification.ndim != 2 or not (noise.shape[0] == original.shape[0] == verification.shape[0]):
        raise ValueError("expected noise [streams, m], original_speech [streams, n0] and verification_speech [streams, n]")
    B = verification.shape[0]
    setups = list(setup_results) if isinstance(setup_results, (list, tuple)) else [setup_results] * B
    if len(setups) != B:
        raise ValueError(f"expected one setup result or one per stream ({B}), got {len(setups)}")
    presets = [target_preset] * B if isinstance(target_preset, str) else list(target_preset)
    preset_ids(presets, B)  # the reference's ValueError for an unknown name, before any GPU work
    chains = [_chain_of(s) for s in setups]
    if verification.shape[1] < int(fs * SPEECH_MIN_DURATION_S):  # :1484
        return [_early_exit("verification passage was too short") for _ in range(B)]

    handle = SetupVerification(int(fs), NPERSEG, B, device)
    try:
        nothing = np.zeros((B, handle.bins))
        levels = handle.measure(nothing, nothing, nothing, presets, verification=verification)
        out: list = [None] * B
        for s in range(B):  # :1490
            if levels["non_finite"][s][2] or levels["clipped_0999"][s][2]:
                out[s] = _early_exit("verification passage was non-finite or clipped")
        live = [s for s in range(B) if out[s] is None]
        if not live:
            return out
        bands, flats = [chains[s][0] for s in live], [chains[s][1] for s in live]
        if _rendered is None:
            rendered, simulation = _render(verification[live], float(fs), bands, flats, device)
            rendered_noise, _ = _render(noise[live], float(fs), bands, flats, device)
        else:  # a test's own render of the same streams: (rendered, rendered_noise, simulation dicts)
            rendered, rendered_noise, simulation = _rendered
        spectra = [core.analyze_voice_spectrum_batch(original[live], int(fs), NPERSEG, device=device),
                   core.analyze_voice_spectrum_batch(verification[live], int(fs), NPERSEG, noise_audio=noise[live], device=device),
                   core.analyze_voice_spectrum_batch(rendered, int(fs), NPERSEG, noise_audio=rendered_noise, device=device)]
        median = lambda results: np.stack([r.median_spectrum_db for r in results])  # noqa: E731
        snr = [r.spectral_snr_db for r in spectra[2]]
        rows = handle.measure(median(spectra[0]), median(spectra[1]), median(spectra[2]), [presets[s] for s in live],
                              None if any(x is None for x in snr) else np.stack(snr), noise=noise[live], original=original[live],
                              verification=verification[live], rendered=rendered, rendered_noise=rendered_noise)
    finally:
        handle.close()
    features = [core.measure_speech_features_batch(verification[live], int(fs), rows["rms_db"][:, 0], noise_audio=noise[live], device=device),
                core.measure_speech_features_batch(rendered, int(fs), rows["rms_db"][:, 4], noise_audio=rendered_noise, device=device)]
    for i, s in enumerate(live):
        out[s] = decide_voice_setup_verification(
            rows[i], dict(simulation[i], simulation_backend="rust"), {"compressor_settings": chains[s][3], "deesser_settings": chains[s][2]},
            verification_samples=verification.shape[1], sample_rate=float(fs), before_snr_db=spectra[1][i].snr_db,
            after_snr_db=spectra[2][i].snr_db, loudness_variation_before_db=features[0][i]["active_loudness_spread_db"],
            loudness_variation_after_db=features[1][i]["active_loudness_spread_db"])
    return out


def validate_voice_setup_verification(noise_audio, original_speech_audio, verification_speech_audio, sample_rate: int, setup_result,
                                      target_preset: str) -> dict:
    """The reference's signature (voice_setup.py:1468-1475): a batch of one."""
    row = lambda x: np.asarray(x, dtype=np.float32).reshape(1, -1)  # noqa: E731
    return verify_voice_setup_batch(row(noise_audio), row(original_speech_audio), row(verification_speech_audio), sample_rate,
                                    setup_result, target_preset)[0]


# ---- the offline validation and the confidences behind apply_recommended (voice_setup.py:1265-1364)
def offline_validation_diagnostics(records, noise_reasons, speech, fs: int, eq_settings=None, device: int = 0) -> list[dict]:
    """Per recommend_voice_chain_batch record the reference's ``diagnostics`` keys of :1372-1442 that this backend builds:
    setup_confidence, recommendation_uncertainty, confidence_semantics, uncertainty_reasons, weak_capture, apply_recommended, the
    four stage confidences, offline_validation_passed and offline_validation (the simulation dict of the setup passage through
    the recommended chain, :1297-1312).  ``noise_reasons``: the noise reference's reasons per stream (they lead the list, :1333).
    ``eq_settings``: one dict or one per stream, or None: the flat ten bands, and Auto-EQ counts as abstained (:1351-1356)."""
    from . import mic_eq_core as core

    lib = _lib.load()
    audio = np.ascontiguousarray(speech, dtype=np.float32)
    B = audio.shape[0]
    eqs = list(eq_settings) if isinstance(eq_settings, (list, tuple)) else [eq_settings] * B
    if len(eqs) != B or len(records) != B or len(noise_reasons) != B:
        raise ValueError(f"expected one record, one list of noise reasons and one or {B} eq_settings for {B} streams")
    chains = [_chain_of({"eq_settings": eq, "deesser": rec["deesser"], "compressor": rec["compressor"]}) for eq, rec in zip(eqs, records)]
    _, simulation = _render(audio, float(fs), [c[0] for c in chains], [c[1] for c in chains], device)
    keys = (("output_true_peak_db", 1 << 2), ("limiter_effective_ceiling_db", 1 << 3), ("compressor_gain_reduction_db", 1 << 1),
            ("compressor_gain_reduction_p95_db", 1 << 0), ("deesser_gain_reduction_db", _lib.SETUP_HAS_DEESSER_PEAK))
    out = []
    for rec, eq, reasons, sim in zip(records, eqs, noise_reasons, simulation):
        i, r = _lib.SetupOfflineInputs(), _lib.SetupOfflineResult()
        i.capture_confidence, i.snr_confidence = float(rec["capture_confidence"]), float(rec["snr_confidence"])
        i.speech_dynamic_range_db = float(rec["features"]["loudness_range_db"])
        i.conservative_noise_rms_db, i.noise_referenced_snr_db = float(rec["conservative_noise_rms_db"]), float(rec["noise_referenced_snr_db"])
        i.active_duration_s = float(rec["features"]["active_duration_s"])
        i.deesser_frame_evidence_confidence = float(rec["deesser_diagnostics"]["frame_evidence_confidence"])
        i.deesser_enabled = int(bool(rec["deesser_diagnostics"]["enabled"]))
        i.peak_reduction_cap_db = float(rec["compressor_diagnostics"]["peak_reduction_cap_db"])
        i.target_p95_reduction_db = float(rec["compressor_diagnostics"]["target_p95_reduction_db"])
        i.noise_status_usable = int(rec["noise_reference_status"] == "usable")
        i.has_eq_settings = int(bool(eq))
        if eq and eq.get("analysis_confidence") is not None:
            i.eq_has_analysis_confidence, i.eq_analysis_confidence = 1, float(eq["analysis_confidence"])
        i.eq_apply_recommended = int(bool(eq.get("apply_recommended", True))) if eq else 0
        i.simulation_available = i.backend_is_rust = 1
        for key, bit in keys:
            if sim.get(key) is not None:
                i.present |= bit
                setattr(i, key, float(sim[key]))
        _lib.check(lib.af_setup_offline_validation(C.byref(i), C.byref(r)))
        texts = [lib.af_setup_offline_reason_text(b).decode() for b in range(6) if r.uncertainty_reasons >> b & 1]
        out.append({
            "setup_confidence": r.setup_confidence, "recommendation_uncertainty": r.recommendation_uncertainty,
            "confidence_semantics": "bounded_quality_score", "uncertainty_reasons": list(reasons) + texts,
            "weak_capture": bool(r.weak_capture), "apply_recommended": bool(r.apply_recommended),
            "capture_confidence": float(rec["capture_confidence"]), "eq_confidence": r.eq_confidence, "gate_confidence": r.gate_confidence,
            "deesser_confidence": r.deesser_confidence, "compressor_confidence": r.compressor_confidence,
            "offline_validation_passed": bool(r.offline_validation_passed),
            "offline_validation": dict(sim, simulation_backend="rust", safety_authority="authoritative")})
    return out
