"""Loader for libaudioforge_mi.so (the C ABI of include/audioforge_mi.h).

There is no CPU fallback: if the HIP library is missing or does not load, every call
raises ImportError, exactly like the reference's `_missing_core`
(python/mic_eq/__init__.py:48-52).
"""
from __future__ import annotations

import ctypes as C
import pathlib

PKG_DIR = pathlib.Path(__file__).resolve().parents[1]
import os

# AF_LIB_PATH: load another build of the same library (same-box A/B runs of kernel variants)
LIB_PATH = pathlib.Path(os.environ.get("AF_LIB_PATH") or (PKG_DIR / "libaudioforge_mi.so"))

AF_OK = 0
AF_ERR_INVALID_ARGUMENT = -1
AF_ERR_BACKEND = -2
AF_ERR_NON_FINITE = -3
AF_ERR_STATE = -4
AF_ERR_UNSUPPORTED = -5

LAYOUT_STREAM_MAJOR = 0
LAYOUT_TIME_MAJOR = 1
KERNEL_AUTO, KERNEL_LANE_PER_STREAM, KERNEL_PHASED, KERNEL_QUAD, KERNEL_STAGED, KERNEL_ROLES = 0, 1, 2, 3, 4, 5


class EqBandConfig(C.Structure):
    _fields_ = [
        ("filter_type", C.c_int32),
        ("frequency_hz", C.c_double),
        ("gain_db", C.c_double),
        ("q", C.c_double),
        ("slope_db_per_octave", C.c_int32),
        ("enabled", C.c_int32),
    ]


class BlockStats(C.Structure):
    _fields_ = [
        ("input_sample_peak", C.c_float),
        ("output_sample_peak", C.c_float),
        ("true_peak_limiter_input_peak", C.c_float),
        ("output_true_peak", C.c_float),
        ("limiter_peak_gain_reduction_db", C.c_float),
        ("true_peak_limiter_gain_reduction_db", C.c_float),
        ("compressor_gain_reduction_db", C.c_float),
        ("deesser_gain_reduction_db", C.c_float),
        ("input_square_sum", C.c_double),
        ("output_square_sum", C.c_double),
        ("true_peak_limited_events", C.c_uint32),
        ("non_finite_output", C.c_uint32),
        ("compressor_makeup_gain_db", C.c_float),
        ("auto_makeup_activity", C.c_float),
        ("auto_makeup_reliability", C.c_float),
        ("reserved", C.c_float),
    ]


class VoiceSpectrumRow(C.Structure):
    _fields_ = [
        ("frames", C.c_int32),
        ("voiced", C.c_int32),
        ("voiced_window_ratio", C.c_double),
        ("vad_active_window_ratio", C.c_double),
        ("vad_probability_used", C.c_int32),
        ("noise_reference_source", C.c_int32),
        ("used_single_spectrum_fallback", C.c_int32),
        ("welch_segments", C.c_int32),
    ]


class VoiceSpectrumOutputs(C.Structure):
    _fields_ = [
        ("rows", C.POINTER(VoiceSpectrumRow)),
        ("speech_db", C.POINTER(C.c_double)),
        ("noise_db", C.POINTER(C.c_double)),
        ("spectral_snr_db", C.POINTER(C.c_double)),
        ("welch_db", C.POINTER(C.c_double)),
        ("welch_sum", C.POINTER(C.c_double)),
        ("frame_power", C.POINTER(C.c_double)),
        ("frame_rms_db", C.POINTER(C.c_double)),
        ("voiced_mask", C.POINTER(C.c_uint8)),
        ("keep_windows", C.c_int32),
    ]


class VoiceSpectrumReliabilityRow(C.Structure):
    _fields_ = [
        ("snr_db", C.c_double),
        ("spectral_tilt_db_per_octave", C.c_double),
        ("residual_confidence", C.c_double),
        ("measurement_coverage", C.c_double),
        ("outlier_rejection_ratio", C.c_double),
        ("phonetic_coverage", C.c_double),
        ("effective_measurement_blocks", C.c_double),
        ("voiced", C.c_int32),
        ("independent", C.c_int32),
        ("blocks", C.c_int32),
        ("inliers", C.c_int32),
        ("used_closest_windows", C.c_int32),
        ("reserved", C.c_int32),
    ]


class VoiceSpectrumReliabilityOutputs(C.Structure):
    _fields_ = [
        ("rows", C.POINTER(VoiceSpectrumReliabilityRow)),
        ("median_spectrum_db", C.POINTER(C.c_double)),
        ("spectral_repeatability", C.POINTER(C.c_double)),
        ("measurement_uncertainty_db", C.POINTER(C.c_double)),
        ("spectral_snr_db", C.POINTER(C.c_double)),
        ("window_distance", C.POINTER(C.c_double)),
        ("inlier_mask", C.POINTER(C.c_uint8)),
    ]


class NoiseReferenceRow(C.Structure):
    _fields_ = ([("status", C.c_int32), ("conservative", C.c_int32), ("reasons", C.c_uint32), ("guidance", C.c_uint32)]
                + [(name, C.c_double) for name in (
                    "quality_score", "duration_s", "finite_fraction", "noise_rms_db", "conservative_noise_rms_db", "noise_peak_db",
                    "crest_factor_db", "clipped_fraction", "zero_fraction", "rms_spread_db", "octave_stability_db",
                    "spectral_flux_db", "vad_contamination_ratio", "vad_contamination_p90", "capture_age_s",
                    "in_capture_level_delta_db", "spectral_shape_distance_db", "noise_sum_squares", "noise_peak")]
                + [(name, C.c_int64) for name in ("finite_samples", "clipped_samples", "zero_samples")]
                + [(name, C.c_int32) for name in ("in_capture_noise_frame_count", "noise_frames", "speech_frames", "n_bands",
                                                  "has_in_capture_spectrum", "reserved")])


class NoiseReferenceOutputs(C.Structure):
    _fields_ = [("rows", C.POINTER(NoiseReferenceRow))] + [(name, C.POINTER(C.c_double)) for name in (
        "explicit_spectrum_db", "conservative_spectrum_db", "in_capture_spectrum_db", "frame_rms_db", "band_levels_db",
        "noise_chunk_sums", "noise_frame_power", "speech_frame_power", "noise_psd", "band_power", "explicit_middles",
        "in_capture_middles")]


class SpeechFeaturesRow(C.Structure):
    _fields_ = ([(name, C.c_int32) for name in (
                    "non_finite", "frames", "active_frames", "spectral_frames", "noise_frames", "vad_probability_used",
                    "short_term_window_count", "loudness_window_count", "evidence_available", "reserved")]
                + [(name, C.c_double) for name in (
                    "active_duration_s", "active_ratio", "vad_active_frame_ratio", "short_term_lufs", "momentary_lufs",
                    "active_loudness_spread_db", "loudness_range_db", "band_low_db", "band_body_db", "band_presence_db",
                    "band_sibilance_db", "sibilance_excess_db", "confidence", "frame_probability_p90", "frame_probability_top_mean",
                    "temporal_score", "absolute_hf_strength_p90", "noise_reliability_p90", "excess_p90_db", "temporal_contrast_db",
                    "candidate_frame_ratio", "candidate_snr_db", "peak_hz", "adaptive_floor_db")])


class SpeechFeaturesOutputs(C.Structure):
    _fields_ = [("rows", C.POINTER(SpeechFeaturesRow)), ("frame_db", C.POINTER(C.c_double)), ("active_frame_mask", C.POINTER(C.c_uint8)),
                ("frame_indices", C.POINTER(C.c_int32)), ("frame_probabilities", C.POINTER(C.c_double)),
                ("frame_feature_rows", C.POINTER(C.c_double)), ("frame_power", C.POINTER(C.c_double)),
                ("chunk_energy", C.POINTER(C.c_double)), ("band_sums", C.POINTER(C.c_double)),
                ("sibilance_middles", C.POINTER(C.c_double)), ("sibilance_argmax", C.POINTER(C.c_int32)),
                ("sibilance_rows", C.POINTER(C.c_double)), ("noise_band_sums", C.POINTER(C.c_double)),
                ("weighted_sums", C.POINTER(C.c_double)), ("weighted_argmax", C.POINTER(C.c_int32))]


class VoiceSetupInputs(C.Structure):
    _fields_ = [("features", C.POINTER(SpeechFeaturesRow)), ("frame_db", C.POINTER(C.c_double)),
                ("active_frame_mask", C.POINTER(C.c_uint8)), ("freqs", C.POINTER(C.c_double)), ("spectrum_db", C.POINTER(C.c_double)),
                ("bins", C.c_int32), ("used_single_spectrum_fallback", C.c_int32), ("residual_confidence", C.c_double),
                ("snr_db", C.c_double), ("noise_quality_score", C.c_double), ("conservative_noise_rms_db", C.c_double),
                ("noise_status", C.c_int32), ("vad_available", C.c_int32), ("target_lufs", C.c_double),
                ("dynamics_intensity", C.c_int32), ("reserved", C.c_int32), ("custom_target_p95_db", C.c_double),
                ("custom_peak_cap_db", C.c_double), ("enable_probability_threshold", C.c_double)]


class VoiceSetupRecommendation(C.Structure):
    _fields_ = ([(name, C.c_double) for name in (
                    "speech_floor_db", "speech_body_db", "speech_frame_peak_db", "speech_snr_db", "snr_confidence", "capture_confidence",
                    "gate_threshold_db", "gate_vad_threshold", "gate_vad_hold_time_ms", "gate_vad_pre_gain", "gate_margin_db")]
                + [(name, C.c_int32) for name in ("gate_mode", "gate_auto_threshold_enabled", "deesser_enabled",
                                                  "deesser_frame_evidence_available", "deesser_invalid_evidence", "reserved")]
                + [(name, C.c_double) for name in (
                    "deesser_auto_amount", "deesser_low_cut_hz", "deesser_high_cut_hz", "deesser_ratio", "deesser_max_reduction_db",
                    "deesser_sibilance_excess_db", "deesser_peak_hz", "deesser_frame_evidence_confidence",
                    "deesser_detection_probability")]
                + [("deesser_clip_features", C.c_double * 6)]
                + [(name, C.c_int32) for name in ("compressor_auto_makeup_enabled", "compressor_profile")]
                + [(name, C.c_double) for name in (
                    "compressor_threshold_db", "compressor_ratio", "compressor_attack_ms", "compressor_release_ms",
                    "compressor_makeup_gain_db", "compressor_base_release_ms", "compressor_target_lufs", "compressor_target_p95_db",
                    "compressor_target_median_db", "compressor_peak_cap_db", "compressor_noise_reference_reliability")])


class CompressorCandidate(C.Structure):
    _fields_ = [("capture", C.c_int32), ("reserved", C.c_int32), ("threshold_db", C.c_double), ("ratio", C.c_double),
                ("attack_ms", C.c_double), ("release_ms", C.c_double)]


class CompressorBase(C.Structure):
    _fields_ = [("makeup_gain_db", C.c_double), ("base_release_ms", C.c_double), ("adaptive_release", C.c_int32),
                ("sidechain_highpass_enabled", C.c_int32)]


class ChainSimulation(C.Structure):
    _fields_ = ([(name, C.c_float) for name in (
                    "input_sample_peak_db", "input_rms_db", "output_sample_peak_db", "pre_limiter_true_peak_db", "output_true_peak_db",
                    "output_rms_db", "limiter_effective_ceiling_db", "sample_headroom_db", "pre_limiter_true_peak_headroom_db",
                    "true_peak_headroom_db", "limiter_gain_reduction_db", "true_peak_limiter_gain_reduction_db")]
                + [("true_peak_limited_events", C.c_uint64)]
                + [(name, C.c_float) for name in (
                    "compressor_gain_reduction_db", "deesser_gain_reduction_db", "compressor_gain_reduction_median_db",
                    "compressor_gain_reduction_p95_db", "compressor_gain_reduction_active_ratio", "active_output_gain_db",
                    "silence_output_gain_db", "silence_level_delta_db", "compressor_pumping_score_db")]
                + [("non_finite_output", C.c_int32)]
                + [(name, C.c_float) for name in ("deesser_gain_reduction_median_db", "deesser_gain_reduction_p95_db", "analysis_block_ms",
                                                  "active_analysis_threshold_db")]
                + [("active_analysis_block_count", C.c_uint64), ("processed_samples", C.c_uint64)]
                + [(name, C.c_float) for name in ("output_sample_peak", "pre_limiter_true_peak", "output_true_peak", "output_rms")])


class CompressorSearchSettings(C.Structure):
    _fields_ = ([(name, C.c_double) for name in ("threshold_db", "ratio", "attack_ms", "release_ms", "makeup_gain_db", "base_release_ms")]
                + [(name, C.c_int32) for name in ("adaptive_release", "sidechain_highpass_enabled", "auto_makeup_enabled", "reserved")]
                + [(name, C.c_double) for name in ("target_lufs", "measured_short_term_lufs", "target_p95_db", "target_median_db",
                                                   "peak_cap_db")])


class CompressorSearchResult(C.Structure):
    _fields_ = ([(name, C.c_int32) for name in ("backend_available", "expanded_search_selected", "peak_cap_passed", "iterations",
                                                  "candidate_count", "evaluated_count", "winner", "verification_equals_evaluation")]
                + [(name, C.c_double) for name in (
                    "threshold_db", "ratio", "attack_ms", "release_ms", "measured_median_gain_reduction_db",
                    "measured_p95_gain_reduction_db", "measured_peak_gain_reduction_db", "active_reduction_ratio", "total_objective",
                    "incumbent_objective", "threshold_only_objective", "expanded_candidate_objective", "active_output_gain_db",
                    "silence_output_gain_db", "compressor_pumping_score_db", "output_true_peak_db", "pre_limiter_true_peak_headroom_db")]
                + [("evaluated", (C.c_double * 4) * 67), ("scores", C.c_double * 67)])


TARGET_PRESETS = ("broadcast", "podcast", "streaming", "flat")  # AF_TARGET_*
SETUP_SIGNALS = ("noise", "original", "verification", "rendered", "rendered_noise")  # AF_SETUP_SIGNAL_*


class SetupVerificationAudio(C.Structure):
    _fields_ = [("samples", C.c_void_p), ("stride", C.c_int64), ("length", C.c_int64), ("lengths", C.POINTER(C.c_int64))]


class SetupVerificationRow(C.Structure):
    _fields_ = [("masked_bins", C.c_int32), ("snr_available", C.c_int32), ("band_present", C.c_int32 * 4),
                ("non_finite", C.c_int32 * 5), ("clipped_0999", C.c_int32 * 5), ("clipped_1", C.c_int32 * 5), ("reserved", C.c_int32),
                ("spectral_target_error_before_db", C.c_double), ("spectral_target_error_after_db", C.c_double),
                ("shape_delta_db", C.c_double), ("band_snr_db", C.c_double * 4), ("offsets_before", C.c_double * 5),
                ("offsets_after", C.c_double * 5), ("sum_squares", C.c_double * 5), ("peak", C.c_double * 5), ("rms_db", C.c_double * 5)]


SETUP_DECISIONS = ("accept", "reduce", "rollback", "retry")  # AF_SETUP_*
SETUP_REASON_NO_RENDERER = 6  # AF_SETUP_REASON_NO_RENDERER: the one early exit that also reports simulation_backend
# the bits of SetupVerificationEvidence.present, AF_SETUP_HAS_*, in bit order
SETUP_EVIDENCE_KEYS = ("compressor_gain_reduction_p95_db", "compressor_gain_reduction_db", "output_true_peak_db",
                       "limiter_effective_ceiling_db", "true_peak_limited_events", "output_rms_db", "input_rms_db",
                       "deesser_gain_reduction_p95_db", "compressor_gain_reduction_median_db", "deesser_gain_reduction_median_db",
                       "target_p95_reduction_db", "peak_reduction_cap_db", "deesser_max_reduction_db")


class SetupVerificationEvidence(C.Structure):
    _fields_ = ([("present", C.c_uint32), ("backend_is_rust", C.c_int32), ("verification_samples", C.c_int64),
                 ("sample_rate", C.c_double), ("true_peak_limited_events", C.c_uint64)]
                + [(name, C.c_double) for name in (
                    "compressor_gain_reduction_p95_db", "compressor_gain_reduction_db", "output_true_peak_db",
                    "limiter_effective_ceiling_db", "output_rms_db", "input_rms_db", "deesser_gain_reduction_p95_db",
                    "compressor_gain_reduction_median_db", "deesser_gain_reduction_median_db", "target_p95_reduction_db",
                    "peak_reduction_cap_db", "deesser_max_reduction_db", "before_snr_db", "after_snr_db",
                    "loudness_variation_before_db", "loudness_variation_after_db")])


class SetupVerificationResult(C.Structure):
    _fields_ = ([(name, C.c_int32) for name in ("decision", "reason", "early_exit", "clipped")]
                + [("limiter_activity_events", C.c_uint64)]
                + [(name, C.c_double) for name in (
                    "spectral_target_error_before_db", "spectral_target_error_after_db", "loudness_variation_before_db",
                    "loudness_variation_after_db", "noise_floor_change_db", "relative_noise_floor_change_db", "snr_change_db",
                    "compressor_gain_reduction_median_db", "compressor_gain_reduction_p95_db", "compressor_gain_reduction_peak_db",
                    "deesser_gain_reduction_median_db", "deesser_gain_reduction_p95_db", "output_true_peak_db",
                    "level_difference_db", "shape_delta_db")])


SETUP_HAS_DEESSER_PEAK = 1 << 13  # AF_SETUP_HAS_DEESSER_PEAK


class SetupOfflineInputs(C.Structure):
    _fields_ = ([(name, C.c_double) for name in (
                    "capture_confidence", "snr_confidence", "speech_dynamic_range_db", "conservative_noise_rms_db",
                    "noise_referenced_snr_db", "active_duration_s", "deesser_frame_evidence_confidence", "peak_reduction_cap_db",
                    "target_p95_reduction_db", "eq_analysis_confidence")]
                + [(name, C.c_int32) for name in ("deesser_enabled", "noise_status_usable", "has_eq_settings", "eq_has_analysis_confidence",
                                                  "eq_apply_recommended", "simulation_available", "backend_is_rust")]
                + [("present", C.c_uint32)]
                + [(name, C.c_double) for name in ("output_true_peak_db", "limiter_effective_ceiling_db", "compressor_gain_reduction_db",
                                                   "compressor_gain_reduction_p95_db", "deesser_gain_reduction_db")])


class SetupOfflineResult(C.Structure):
    _fields_ = ([(name, C.c_int32) for name in ("offline_validation_passed", "weak_capture", "apply_recommended")]
                + [("uncertainty_reasons", C.c_uint32)]
                + [(name, C.c_double) for name in ("eq_confidence", "gate_confidence", "deesser_confidence", "compressor_confidence",
                                                   "setup_confidence", "recommendation_uncertainty")])


class LaneChainSettings(C.Structure):
    """af_lane_chain_settings: one stream's settings of the streaming lane chain."""
    _fields_ = ([("bands", (C.c_double * 3) * 10)]
                + [(name, C.c_double) for name in ("compressor_threshold_db", "compressor_ratio", "compressor_attack_ms",
                                                   "compressor_release_ms", "compressor_makeup_gain_db", "compressor_base_release_ms",
                                                   "limiter_ceiling_db", "limiter_release_ms")]
                + [(name, C.c_int32) for name in ("eq_enabled", "compressor_enabled", "limiter_enabled", "compressor_adaptive_release",
                                                  "compressor_sidechain_highpass_enabled", "limiter_careful_output_enabled")])


# every symbol include/audioforge_mi.h declares: name -> (restype, argtypes)
_vp, _i32, _i64, _d, _f, _sz = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_float, C.c_size_t
_fp, _dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
SIGNATURES = {
    "af_version": (C.c_int, []),
    "af_last_error": (C.c_char_p, []),
    "af_device_count": (C.c_int, []),
    "af_engine_create": (C.c_int, [_d, _i32, _i32, C.POINTER(_vp)]),
    "af_engine_destroy": (None, [_vp]),
    "af_engine_reset": (C.c_int, [_vp]),
    "af_engine_n_streams": (_i32, [_vp]),
    "af_engine_set_live_control": (C.c_int, [_vp, _i32]),
    "af_engine_live_control_pending": (C.c_int, [_vp, C.POINTER(_i32)]),
    "af_engine_last_retune_ms": (C.c_int, [_vp, _dp]),
    "af_engine_set_stream_lifecycle": (C.c_int, [_vp, _i32]),
    "af_engine_restart_streams": (C.c_int, [_vp, C.POINTER(_i32), _i32]),
    "af_engine_stream_state_size": (C.c_int, [_vp, C.POINTER(_sz)]),
    "af_engine_export_stream_state": (C.c_int, [_vp, C.POINTER(_i32), _i32, _vp]),
    "af_engine_import_stream_state": (C.c_int, [_vp, C.POINTER(_i32), _i32, _vp]),
    "af_engine_stream_samples_processed": (C.c_int, [_vp, _i32, C.POINTER(_i64)]),
    "af_engine_set_deesser_enabled": (C.c_int, [_vp, _i32]),
    "af_engine_set_eq_enabled": (C.c_int, [_vp, _i32]),
    "af_engine_set_compressor_enabled": (C.c_int, [_vp, _i32]),
    "af_engine_set_limiter_enabled": (C.c_int, [_vp, _i32]),
    "af_engine_set_eq_before_deesser": (C.c_int, [_vp, _i32]),
    "af_engine_set_control_block_samples": (C.c_int, [_vp, _i32]),
    "af_engine_set_input_scrub_enabled": (C.c_int, [_vp, _i32]),
    "af_engine_set_input_clamp_enabled": (C.c_int, [_vp, _i32]),
    "af_engine_set_prefilter_enabled": (C.c_int, [_vp, _i32, _i32]),
    "af_engine_set_suppressor_enabled": (C.c_int, [_vp, _i32]),
    "af_engine_set_suppressor_strength": (C.c_int, [_vp, _f]),
    "af_suppressor_set_synthetic_weights": (C.c_int, [_vp, C.c_uint64]),
    "af_suppressor_load_weights": (C.c_int, [_vp, C.c_char_p, _sz]),
    "af_suppressor_set_raw_protocol": (C.c_int, [_vp, _i32]),
    "af_suppressor_latency_samples": (_i32, [_vp]),
    "af_suppressor_debug_read": (C.c_int, [_vp, _i32, _i32, _fp, _fp, _fp]),
    "af_suppressor_debug_read_pitch": (C.c_int, [_vp, _i32, _i32, _fp, C.POINTER(_i32), _fp]),
    "af_suppressor_debug_pitch_search": (C.c_int, [_fp, _i32, _i32, _fp, C.POINTER(_i32), _i32]),
    "af_suppressor_debug_read_model_input": (C.c_int, [_vp, _i32, _fp, _i64, C.POINTER(_i64)]),
    "af_eq_set_band_frequency": (C.c_int, [_vp, _i32, _d]),
    "af_eq_set_band_gain": (C.c_int, [_vp, _i32, _d]),
    "af_eq_set_band_q": (C.c_int, [_vp, _i32, _d]),
    "af_eq_set_band_config": (C.c_int, [_vp, _i32, C.POINTER(EqBandConfig)]),
    "af_eq_reset": (C.c_int, [_vp]),
    "af_eq_band_config_validate": (C.c_int, [C.POINTER(EqBandConfig), _i32, _d]),
    "af_compressor_set_threshold": (C.c_int, [_vp, _d]),
    "af_compressor_set_ratio": (C.c_int, [_vp, _d]),
    "af_compressor_set_attack_time": (C.c_int, [_vp, _d]),
    "af_compressor_set_release_time": (C.c_int, [_vp, _d]),
    "af_compressor_set_makeup_gain": (C.c_int, [_vp, _d]),
    "af_compressor_set_adaptive_release": (C.c_int, [_vp, _i32]),
    "af_compressor_set_base_release_time": (C.c_int, [_vp, _d]),
    "af_compressor_set_auto_makeup_enabled": (C.c_int, [_vp, _i32]),
    "af_compressor_set_target_lufs": (C.c_int, [_vp, _d]),
    "af_compressor_set_sidechain_highpass_enabled": (C.c_int, [_vp, _i32]),
    "af_compressor_set_noise_reference_reliability": (C.c_int, [_vp, _d]),
    "af_compressor_set_activity_evidence": (C.c_int, [_vp, _dp, _i64, _i32, _d, _d, _d]),
    "af_limiter_set_ceiling": (C.c_int, [_vp, _d]),
    "af_limiter_set_release_time": (C.c_int, [_vp, _d]),
    "af_limiter_set_lookahead_ms": (C.c_int, [_vp, _d]),
    "af_limiter_ceiling_db": (_d, [_vp]),
    "af_limiter_lookahead_samples": (_i32, [_vp]),
    "af_true_peak_limiter_set_release_ms": (C.c_int, [_vp, _f]),
    "af_deesser_set_auto_enabled": (C.c_int, [_vp, _i32]),
    "af_deesser_set_auto_amount": (C.c_int, [_vp, _d]),
    "af_deesser_set_low_cut_hz": (C.c_int, [_vp, _d]),
    "af_deesser_set_high_cut_hz": (C.c_int, [_vp, _d]),
    "af_deesser_set_threshold_db": (C.c_int, [_vp, _d]),
    "af_deesser_set_ratio": (C.c_int, [_vp, _d]),
    "af_deesser_set_attack_ms": (C.c_int, [_vp, _d]),
    "af_deesser_set_release_ms": (C.c_int, [_vp, _d]),
    "af_deesser_set_max_reduction_db": (C.c_int, [_vp, _d]),
    "af_engine_process_device": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _i32, _vp]),
    "af_engine_process_host": (C.c_int, [_vp, _fp, _fp, _i64, _i32]),
    "af_engine_synchronize": (C.c_int, [_vp]),
    "af_engine_stream_host": (C.c_int, [_vp, _fp, _i64, _fp, _i64, C.POINTER(_i64)]),
    "af_engine_pending_input": (_i64, [_vp]),
    "af_engine_last_output_samples": (_i64, [_vp]),
    "af_suppressor_debug_scale_for_model": (C.c_int, [_fp, _fp, _i64, _i32]),
    "af_suppressor_set_trace_enabled": (C.c_int, [_vp, _i32]),
    "af_suppressor_trace_frames": (_i64, [_vp]),
    "af_suppressor_read_trace": (C.c_int, [_vp, C.POINTER(_i32), _i64]),
    # NoiseSuppressor (noise_suppressor.rs:18-194)
    "af_noise_model_from_id": (C.c_int, [C.c_char_p, C.POINTER(_i32)]),
    "af_noise_model_id": (C.c_char_p, [_i32]),
    "af_noise_model_display_name": (C.c_char_p, [_i32]),
    "af_noise_model_available": (_i32, [C.POINTER(_i32), _i32]),
    "af_noise_suppressor_create": (C.c_int, [_i32, _i32, _i32, C.POINTER(_vp)]),
    "af_noise_suppressor_destroy": (None, [_vp]),
    "af_noise_suppressor_engine": (_vp, [_vp]),
    "af_noise_suppressor_push_samples": (_i64, [_vp, _fp, _i64, _i64]),
    "af_noise_suppressor_process_frames": (C.c_int, [_vp]),
    "af_noise_suppressor_available_samples": (_i64, [_vp]),
    "af_noise_suppressor_pending_input": (_i64, [_vp]),
    "af_noise_suppressor_pop_samples_into": (_i64, [_vp, _fp, _i64, _i64]),
    "af_noise_suppressor_drain_pending_input": (_i64, [_vp, _fp, _i64, _i64]),
    "af_noise_suppressor_set_strength": (C.c_int, [_vp, _f]),
    "af_noise_suppressor_get_strength": (_f, [_vp]),
    "af_noise_suppressor_set_enabled": (C.c_int, [_vp, _i32]),
    "af_noise_suppressor_is_enabled": (_i32, [_vp]),
    "af_noise_suppressor_soft_reset": (C.c_int, [_vp]),
    "af_noise_suppressor_reset": (C.c_int, [_vp]),
    "af_noise_suppressor_model_type": (_i32, [_vp]),
    "af_noise_suppressor_latency_samples": (_i32, [_vp]),
    "af_noise_suppressor_backend_available": (_i32, [_vp]),
    "af_noise_suppressor_backend_failed": (_i32, [_vp]),
    "af_noise_suppressor_backend_error": (C.c_char_p, [_vp]),
    "af_engine_last_block_count": (_i64, [_vp]),
    "af_engine_read_block_stats": (C.c_int, [_vp, C.POINTER(BlockStats), _i64]),
    "af_engine_samples_processed": (_i64, [_vp]),
    "af_engine_set_preset_count": (C.c_int, [_vp, _i32]),
    "af_engine_preset_count": (_i32, [_vp]),
    "af_engine_select_preset": (C.c_int, [_vp, _i32]),
    "af_engine_assign_presets": (C.c_int, [_vp, C.POINTER(_i32), _i32]),
    "af_engine_set_kernel": (C.c_int, [_vp, _i32]),
    "af_engine_set_ring_variant": (C.c_int, [_vp, _i32, _i32]),
    "af_engine_set_timing_enabled": (C.c_int, [_vp, _i32]),
    "af_engine_last_kernel_ms": (C.c_int, [_vp, _dp, C.POINTER(_i32)]),
    "af_engine_last_stage_ms": (C.c_int, [_vp, _dp, _dp]),
    # noise gate stage
    "af_engine_set_gate_enabled": (C.c_int, [_vp, _i32]),
    "af_gate_set_threshold": (C.c_int, [_vp, _d]),
    "af_gate_set_attack_time": (C.c_int, [_vp, _d]),
    "af_gate_set_release_time": (C.c_int, [_vp, _d]),
    "af_gate_set_mode": (C.c_int, [_vp, _i32]),
    "af_gate_threshold_db": (_d, [_vp]),
    "af_engine_gate_enabled": (_i32, [_vp]),
    "af_engine_read_gate_state": (C.c_int, [_vp, _fp, C.POINTER(C.c_uint64), C.POINTER(_i32), _i32]),
    # the VAD-fused gate modes
    "af_gate_set_vad_auto_gate_enabled": (C.c_int, [_vp, _i32]),
    "af_gate_set_vad_threshold": (C.c_int, [_vp, _d]),
    "af_gate_set_hold_time": (C.c_int, [_vp, _d]),
    "af_gate_set_margin": (C.c_int, [_vp, _d]),
    "af_gate_set_auto_threshold": (C.c_int, [_vp, _i32]),
    "af_gate_read_vad_controls": (C.c_int, [_vp, _dp, _dp, _dp, C.POINTER(_i32), C.POINTER(_i32)]),
    "af_gate_set_vad_evidence": (C.c_int, [_vp, _fp, C.POINTER(C.c_uint8), _i64, _i32]),
    "af_engine_read_gate_vad_decisions": (C.c_int, [_vp, _fp, _fp, C.POINTER(_i32), _i64]),
    "af_engine_read_gate_vad_state": (C.c_int, [_vp, _fp, _fp, _fp, _fp, C.POINTER(_i32), C.POINTER(_i32), _i32]),
    "af_engine_last_chain_launch_ms": (C.c_int, [_vp, _dp, _dp, C.POINTER(_i32)]),
    # product resampler
    "af_engine_last_kernel": (C.c_int, [_vp]),
    "af_engine_debug_detector_reuse_chunks": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "af_resampler_calculate_cutoff": (C.c_int, [_i32, _i32, C.POINTER(C.c_float)]),
    "af_resampler_create": (C.c_int, [C.c_uint32, C.c_uint32, _i64, _i32, _i32, _i32, C.POINTER(_vp)]),
    "af_resampler_destroy": (None, [_vp]),
    "af_resampler_output_delay": (C.c_int, [_vp]),
    "af_resampler_expected_frames": (_i64, [_vp, _i64]),
    "af_resampler_sinc_len": (C.c_int, [_vp]),
    "af_resampler_copy_sinc_table": (C.c_int, [_vp, _dp]),
    "af_resampler_plan": (C.c_int, [_vp, _i64, C.POINTER(_i64), C.POINTER(_i64)]),
    "af_resampler_process_device": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i64, _i64, _vp]),
    "af_resampler_process_host": (C.c_int, [_vp, _dp, _dp, _i64, _i32, _i64, _i64]),
    "af_resampler_last_kernel_ms": (C.c_int, [_vp, _dp]),
    "af_resampler_launch_form": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    # streaming product resampler + the engine's device-rate I/O
    "af_stream_resampler_create": (C.c_int, [C.c_uint32, C.c_uint32, _i64, _i32, _i32, _i32, _i32, C.POINTER(_vp)]),
    "af_stream_resampler_destroy": (None, [_vp]),
    "af_stream_resampler_push_host": (C.c_int, [_vp, _fp, _i64, _i64, _fp, _i64, _i64, C.POINTER(_i64)]),
    "af_stream_resampler_push_device": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, C.POINTER(_i64), _vp]),
    "af_stream_resampler_output_frames": (_i64, [_vp, _i64]),
    "af_stream_resampler_pending_input": (_i64, [_vp]),
    "af_stream_resampler_output_delay": (C.c_int, [_vp]),
    "af_stream_resampler_frames_in": (_i64, [_vp]),
    "af_stream_resampler_frames_out": (_i64, [_vp]),
    "af_stream_resampler_reset": (C.c_int, [_vp]),
    "af_stream_resampler_clear_pending": (C.c_int, [_vp]),
    "af_stream_resampler_last_kernel_ms": (C.c_int, [_vp, _dp]),
    "af_stream_resampler_launch_form": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "af_engine_set_io_sample_rates": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "af_engine_stream_plan": (C.c_int, [_vp, _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "af_engine_io_resampler_delay": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32)]),
    "af_engine_io_resampler_pending": (C.c_int, [_vp, C.POINTER(_i64), C.POINTER(_i64)]),
    "af_mixdown_create": (C.c_int, [_i32, _i32, _i32, _i32, C.POINTER(_vp)]),
    "af_mixdown_destroy": (None, [_vp]),
    "af_mixdown_set_mode": (C.c_int, [_vp, _i32]),
    "af_mixdown_mode": (_i32, [_vp]),
    "af_mixdown_channels": (_i32, [_vp]),
    "af_mixdown_push_host": (C.c_int, [_vp, _fp, _i64, _i64, _fp, _i64]),
    "af_mixdown_push_device": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, _vp]),
    "af_mixdown_read_diagnostics": (C.c_int, [_vp, _fp, C.POINTER(C.c_uint64), C.POINTER(_i32), _fp, C.POINTER(_i32), _i32]),
    "af_mixdown_reset": (C.c_int, [_vp]),
    "af_mixdown_last_kernel_ms": (C.c_int, [_vp, _dp, _dp]),
    "af_output_writer_default_config": (C.c_int, [_i32, _vp]),
    "af_output_writer_create": (C.c_int, [_vp, _i32, _i32, C.POINTER(_vp)]),
    "af_output_writer_destroy": (None, [_vp]),
    "af_output_writer_set_limiter": (C.c_int, [_vp, _i32, C.c_float]),
    "af_output_writer_reset": (C.c_int, [_vp]),
    "af_output_writer_max_output_frames": (_i64, [_vp, _i64]),
    "af_output_writer_push_host": (C.c_int, [_vp, _fp, _i64, _i64, C.POINTER(_i64), _i32, _fp, _i64, _i64, C.POINTER(_i64)]),
    "af_output_writer_push_device": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _i32, _vp, _i64, _i64, _vp, _vp]),
    "af_output_writer_read_counters": (C.c_int, [_vp] + [C.POINTER(C.c_uint64)] * 6 + [_i32]),
    "af_output_writer_read_meters": (C.c_int, [_vp, _fp, _fp, _fp, _fp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), _i32]),
    "af_output_writer_read_state": (C.c_int, [_vp, _fp, _fp, C.POINTER(_i32), _fp, _i32]),
    "af_output_writer_last_kernel_ms": (C.c_int, [_vp, _dp]),
    "af_output_writer_last_pass_ms": (C.c_int, [_vp, _dp]),
    "af_engine_set_output_writer": (C.c_int, [_vp, _i32]),
    "af_engine_set_output_queue_fill": (C.c_int, [_vp, C.POINTER(_i64), _i32]),
    "af_engine_read_output_written": (C.c_int, [_vp, C.POINTER(_i64), _i32]),
    "af_engine_read_output_counters": (C.c_int, [_vp] + [C.POINTER(C.c_uint64)] * 6 + [_i32]),
    "af_engine_read_output_meters": (C.c_int, [_vp, _fp, _fp, _fp, _fp, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), _i32]),
    "af_engine_set_input_channels": (C.c_int, [_vp, _i32, _i32]),
    "af_engine_set_input_channel_mode": (C.c_int, [_vp, _i32]),
    "af_engine_read_input_phase": (C.c_int, [_vp, _fp, C.POINTER(C.c_uint64), C.POINTER(_i32), _fp, C.POINTER(_i32), _i32]),
    "af_voice_spectrum_create": (C.c_int, [C.c_uint32, _i32, _i32, C.POINTER(_vp)]),
    "af_voice_spectrum_destroy": (None, [_vp]),
    "af_voice_spectrum_bins": (_i32, [_vp]),
    "af_voice_spectrum_frames": (_i64, [_vp, _i64]),
    "af_voice_spectrum_octave_bands": (C.c_int, [_i32, _dp, _dp, _dp, _i32, C.POINTER(_i32)]),
    "af_voice_spectrum_analyze_host": (C.c_int, [_vp, _fp, _i64, _i32, _i64, _dp, _i64, _fp, _i64, _i64, C.POINTER(VoiceSpectrumOutputs)]),
    "af_voice_spectrum_analyze_device": (C.c_int, [_vp, _vp, _i64, _i32, _i64, _dp, _i64, _vp, _i64, _i64, C.POINTER(VoiceSpectrumOutputs)]),
    "af_voice_spectrum_read_windows": (C.c_int, [_vp, _i32, _dp, _dp, _dp, _i32, C.POINTER(_i32)]),
    "af_voice_spectrum_last_kernel_ms": (C.c_int, [_vp, _dp]),
    "af_voice_spectrum_set_reliability": (C.c_int, [_vp, _i32]),
    "af_voice_spectrum_last_reliability_kernel_ms": (C.c_int, [_vp, _dp, _i32]),
    "af_voice_spectrum_read_reliability": (C.c_int, [_vp, C.POINTER(VoiceSpectrumReliabilityOutputs)]),
    "af_voice_spectrum_set_noise_override": (C.c_int, [_vp, _dp, _dp, _i32, _i32, _i64, _i32]),
    "af_voice_spectrum_smooth_rows": (C.c_int, [_vp, _dp, _i32, _dp]),
    "af_noise_reference_create": (C.c_int, [C.c_uint32, _i32, C.POINTER(_vp)]),
    "af_noise_reference_destroy": (None, [_vp]),
    "af_noise_reference_frame_size": (_i32, [_vp]),
    "af_noise_reference_bins": (_i32, [_vp, _i64]),
    "af_noise_reference_frames": (_i64, [_vp, _i64]),
    "af_noise_reference_analyze_host": (C.c_int, [_vp, _fp, _i64, _i32, _i64, _fp, _i64, _i64, _dp, _i64, _dp, _i64, _dp,
                                                  C.POINTER(C.c_uint32), C.POINTER(NoiseReferenceOutputs)]),
    "af_noise_reference_analyze_device": (C.c_int, [_vp, _vp, _i64, _i32, _i64, _vp, _i64, _i64, _dp, _i64, _dp, _i64, _dp,
                                                    C.POINTER(C.c_uint32), C.POINTER(NoiseReferenceOutputs)]),
    "af_noise_reference_last_kernel_ms": (C.c_int, [_vp, _dp, _i32]),
    "af_speech_features_create": (C.c_int, [C.c_uint32, _i32, _i64, _i64, _i32, C.POINTER(_vp)]),
    "af_speech_features_destroy": (None, [_vp]),
    "af_speech_features_frames": (_i64, [_i64]),
    "af_speech_features_chunks": (_i64, [_i64]),
    "af_speech_features_sibilance_bins": (_i32, [_vp]),
    "af_speech_features_set_frame_model": (C.c_int, [_vp, _d, _dp]),
    "af_speech_features_get_frame_model": (C.c_int, [_vp, _dp, _dp]),
    "af_speech_features_analyze_host": (C.c_int, [_vp, _fp, _i64, _i32, _i64, _dp, _dp, _i64, _fp, _i64, _i64,
                                                  C.POINTER(SpeechFeaturesOutputs)]),
    "af_speech_features_analyze_device": (C.c_int, [_vp, _vp, _i64, _i32, _i64, _dp, _dp, _i64, _vp, _i64, _i64,
                                                    C.POINTER(SpeechFeaturesOutputs)]),
    "af_speech_features_last_kernel_ms": (C.c_int, [_vp, _dp, _i32]),
    "af_device_rate_features_create": (C.c_int, [C.c_uint32, _i32, _i64, _i64, _i32, C.POINTER(_vp)]),
    "af_device_rate_features_destroy": (None, [_vp]),
    "af_device_rate_features_frames": (_i64, [_vp, _i64]),
    "af_device_rate_features_chunks": (_i64, [_vp, _i64]),
    "af_device_rate_features_resampled_length": (_i64, [_vp, _i64]),
    "af_device_rate_features_sibilance_bins": (_i32, [_vp]),
    "af_device_rate_features_set_frame_model": (C.c_int, [_vp, _d, _dp]),
    "af_device_rate_features_get_frame_model": (C.c_int, [_vp, _dp, _dp]),
    "af_device_rate_features_set_scratch_bytes": (C.c_int, [_vp, _i64]),
    "af_device_rate_features_analyze_host": (C.c_int, [_vp, _fp, _i64, _i32, _i64, _dp, _dp, _i64, _fp, _i64, _i64,
                                                       C.POINTER(SpeechFeaturesOutputs)]),
    "af_device_rate_features_analyze_device": (C.c_int, [_vp, _vp, _i64, _i32, _i64, _dp, _dp, _i64, _vp, _i64, _i64,
                                                         C.POINTER(SpeechFeaturesOutputs)]),
    "af_device_rate_features_last_kernel_ms": (C.c_int, [_vp, _dp, _i32]),
    "af_device_rate_features_debug_resample_host": (C.c_int, [_vp, _fp, _i64, _i32, _i64, C.POINTER(C.c_uint8), _dp, C.POINTER(C.c_uint8),
                                                              C.POINTER(_i32)]),
    "af_voice_setup_default_inputs": (None, [C.POINTER(VoiceSetupInputs)]),
    "af_voice_setup_recommend": (C.c_int, [C.POINTER(VoiceSetupInputs), C.POINTER(VoiceSetupRecommendation)]),
    # compressor candidate sweep
    "af_compressor_search_create": (C.c_int, [_d, _i32, C.POINTER(_vp)]),
    "af_compressor_search_destroy": (None, [_vp]),
    "af_compressor_search_set_limiter": (C.c_int, [_vp, _d, _d, _d, _i32]),
    "af_compressor_search_load_host": (C.c_int, [_vp, _fp, _i64, _i32, _i64, C.POINTER(BlockStats)]),
    "af_compressor_search_load_device": (C.c_int, [_vp, _vp, _i64, _i32, _i64, C.POINTER(BlockStats)]),
    "af_compressor_search_sweep": (C.c_int, [_vp, C.POINTER(CompressorCandidate), _i32, C.POINTER(CompressorBase), _i32,
                                             C.POINTER(ChainSimulation)]),
    "af_compressor_search_blocks": (_i64, [_vp]),
    "af_compressor_search_run": (C.c_int, [_vp, C.POINTER(CompressorSearchSettings), C.POINTER(CompressorSearchResult)]),
    "af_compressor_search_last_run_ms": (C.c_int, [_vp, _dp]),
    "af_compressor_search_read_masks": (C.c_int, [_vp, _fp, C.POINTER(C.c_uint8), _fp]),
    "af_compressor_search_read_rows":(C.c_int, [_vp, C.POINTER(BlockStats), _i64]),
    "af_compressor_search_read_audio": (C.c_int, [_vp, _fp, _i64]),
    "af_compressor_search_last_kernel_ms": (C.c_int, [_vp, _dp, _dp]),
    # per-lane EQ
    "af_lane_eq_create": (C.c_int, [_d, _i32, C.POINTER(_vp)]),
    "af_lane_eq_destroy": (None, [_vp]),
    "af_lane_eq_run_host": (C.c_int, [_vp, _fp, _i64, _i32, _i64, C.POINTER(_i32), _i32, _dp]),
    "af_lane_eq_run_device": (C.c_int, [_vp, _vp, _i64, _i32, _i64, C.POINTER(_i32), _i32, _dp]),
    "af_lane_eq_output": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_i64)]),
    "af_lane_eq_read_output": (C.c_int, [_vp, _fp, _i64]),
    "af_lane_eq_last_kernel_ms": (C.c_int, [_vp, _dp]),
    # streaming lane chain
    "af_lane_chain_default_settings": (C.c_int, [C.POINTER(LaneChainSettings)]),
    "af_lane_chain_create": (C.c_int, [_d, _i32, _d, _i32, C.POINTER(_vp)]),
    "af_lane_chain_destroy": (None, [_vp]),
    "af_lane_chain_configure": (C.c_int, [_vp, C.POINTER(_i32), _i32, C.POINTER(LaneChainSettings)]),
    "af_lane_chain_process_host": (C.c_int, [_vp, _fp, _fp, _i64, _i64]),
    "af_lane_chain_process_device": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp]),
    "af_lane_chain_blocks": (_i64, [_vp]),
    "af_lane_chain_read_rows": (C.c_int, [_vp, C.POINTER(BlockStats), _i64]),
    "af_lane_chain_reset": (C.c_int, [_vp]),
    "af_lane_chain_samples_processed": (C.c_int, [_vp, _i32, C.POINTER(_i64)]),
    "af_lane_chain_last_kernel_ms": (C.c_int, [_vp, _dp]),
    # second-passage verification: the measurements
    "af_setup_verification_create": (C.c_int, [C.c_uint32, _i32, _i32, _i32, C.POINTER(_vp)]),
    "af_setup_verification_destroy": (None, [_vp]),
    "af_setup_verification_measure_host": (C.c_int, [_vp, _i32, _dp, _dp, _dp, _i64, _dp, _i64, C.POINTER(_i32),
                                                     C.POINTER(SetupVerificationAudio), C.POINTER(SetupVerificationRow)]),
    "af_setup_verification_measure_device": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i64, _vp, _i64, C.POINTER(_i32),
                                                       C.POINTER(SetupVerificationAudio), _vp, _vp]),
    "af_setup_verification_decide": (C.c_int, [C.POINTER(SetupVerificationRow), C.POINTER(SetupVerificationEvidence),
                                               C.POINTER(SetupVerificationResult)]),
    "af_setup_verification_reason_text": (C.c_char_p, [_i32]),
    "af_setup_offline_validation": (C.c_int, [C.POINTER(SetupOfflineInputs), C.POINTER(SetupOfflineResult)]),
    "af_setup_offline_reason_text": (C.c_char_p, [_i32]),
    # latency calibration (the structures are latency_calibration.py's)
    "af_latency_create": (C.c_int, [_d, _dp, _i64, _i32, _i64, _i32, C.POINTER(_vp)]),
    "af_latency_destroy": (None, [_vp]),
    "af_latency_layout": (C.c_int, [_vp, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "af_latency_analyze_host": (C.c_int, [_vp, _fp, _i64, _i64, _i32, C.POINTER(_i64), _vp]),
    "af_latency_analyze_device": (C.c_int, [_vp, _vp, _i64, _i64, _i32, C.POINTER(_i64), _vp]),
    "af_latency_read_results": (C.c_int, [_vp, _vp, _i32]),
    "af_latency_read_scores": (C.c_int, [_vp, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), _dp, _dp, C.POINTER(_i32), C.POINTER(_i32),
                                         _dp, _i64]),
    "af_latency_last_kernel_ms": (C.c_int, [_vp, _dp, _dp]),
    "af_latency_message_text": (C.c_char_p, [_i32, _i32]),
    "af_latency_debug_rfft": (C.c_int, [_vp, _fp, _i64, _dp]),
    "af_gate_process_host": (C.c_int, [_fp, _fp, _i64, _i32, _i64, _d, _d, _d, _d, _i32, _i32, _fp, C.POINTER(C.c_uint64), _i32]),
    "af_measure_integrated_loudness_device": (C.c_int, [_vp, _i64, _i32, _i64, C.c_uint32, _i32, _dp, C.POINTER(_i32)]),
    "af_measure_integrated_loudness_host": (C.c_int, [_fp, _i64, _i32, _i64, C.c_uint32, _i32, _dp, C.POINTER(_i32)]),
    "af_eq_magnitude_response": (C.c_int, [_dp, _sz, _dp, _d, _dp]),
    "af_eq_magnitude_response_v2": (C.c_int, [_dp, _sz, C.POINTER(EqBandConfig), _d, _dp]),
    "af_engine_eq_magnitude_response": (C.c_int, [_vp, _dp, _sz, _dp]),
}

# entry points whose return value is data, not an af_status
VALUE_FUNCTIONS = {
    "af_version", "af_last_error", "af_device_count", "af_engine_n_streams", "af_limiter_ceiling_db",
    "af_limiter_lookahead_samples", "af_suppressor_latency_samples", "af_engine_last_block_count", "af_engine_samples_processed", "af_engine_destroy", "af_engine_last_kernel",
    "af_engine_pending_input", "af_engine_last_output_samples", "af_suppressor_trace_frames", "af_engine_preset_count",
    "af_noise_model_id", "af_noise_model_display_name", "af_noise_model_available", "af_noise_suppressor_destroy",
    "af_noise_suppressor_engine", "af_noise_suppressor_push_samples", "af_noise_suppressor_available_samples",
    "af_noise_suppressor_pending_input", "af_noise_suppressor_pop_samples_into", "af_noise_suppressor_drain_pending_input",
    "af_noise_suppressor_get_strength", "af_noise_suppressor_is_enabled", "af_noise_suppressor_model_type",
    "af_noise_suppressor_latency_samples", "af_noise_suppressor_backend_available", "af_noise_suppressor_backend_failed",
    "af_noise_suppressor_backend_error",
    "af_resampler_destroy", "af_resampler_output_delay", "af_resampler_expected_frames", "af_resampler_sinc_len",
    "af_gate_threshold_db", "af_engine_gate_enabled",
    "af_stream_resampler_destroy", "af_stream_resampler_output_frames", "af_stream_resampler_pending_input",
    "af_stream_resampler_output_delay", "af_stream_resampler_frames_in", "af_stream_resampler_frames_out",
    "af_mixdown_destroy", "af_mixdown_mode", "af_mixdown_channels",
    "af_output_writer_destroy", "af_output_writer_max_output_frames",
    "af_voice_spectrum_destroy", "af_voice_spectrum_bins", "af_voice_spectrum_frames",
    "af_noise_reference_destroy", "af_noise_reference_frame_size", "af_noise_reference_bins", "af_noise_reference_frames",
    "af_speech_features_destroy", "af_speech_features_frames", "af_speech_features_chunks", "af_speech_features_sibilance_bins",
    "af_device_rate_features_destroy", "af_device_rate_features_frames", "af_device_rate_features_chunks",
    "af_device_rate_features_resampled_length", "af_device_rate_features_sibilance_bins",
    "af_voice_setup_default_inputs",
    "af_compressor_search_destroy", "af_compressor_search_blocks", "af_lane_eq_destroy",
    "af_lane_chain_destroy", "af_lane_chain_blocks",
    "af_setup_verification_destroy", "af_setup_verification_reason_text", "af_setup_offline_reason_text",
    "af_latency_destroy", "af_latency_message_text",
}

_lib = None
_load_error: Exception | None = None


def load() -> C.CDLL:
    """Load the HIP library or raise ImportError (never falls back to a CPU path)."""
    global _lib, _load_error
    if _lib is not None:
        return _lib
    if _load_error is not None:
        raise ImportError(str(_load_error)) from _load_error
    try:
        if not LIB_PATH.exists():
            raise OSError(f"{LIB_PATH} is missing; build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(str(LIB_PATH))
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
    except (OSError, AttributeError) as error:
        _load_error = error
        raise ImportError(
            f"libaudioforge_mi.so (the MI355X HIP backend) is unavailable: {error}. There is no CPU fallback."
        ) from error
    _lib = lib
    return lib


def last_error() -> str:
    return load().af_last_error().decode("utf-8", "replace")


def check(rc: int) -> None:
    """Map af_status to the exception classes the reference binding raises."""
    if rc == AF_OK:
        return
    msg = last_error()
    if rc in (AF_ERR_INVALID_ARGUMENT, AF_ERR_NON_FINITE):
        raise ValueError(msg)  # PyValueError, lib.rs:105-141,225-229
    if rc == AF_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError(msg)  # PyRuntimeError, python_api.rs:332-340
