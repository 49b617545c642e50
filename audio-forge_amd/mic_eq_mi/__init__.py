"""mic_eq_mi -- the MI355X backend behind the reference's ``mic_eq`` offline operator names.

Mirrors python/mic_eq/__init__.py:38-98 of the reference: the names below are the ones the
evaluation harness imports from ``mic_eq``; an operator this backend does not build yet raises
ImportError through ``_missing_core`` (the reference's own degradation path), and nothing here
falls back to a CPU implementation.
"""
from __future__ import annotations

from . import _lib
from ._lib import KERNEL_AUTO, KERNEL_LANE_PER_STREAM, KERNEL_PHASED, KERNEL_QUAD, KERNEL_STAGED, LAYOUT_STREAM_MAJOR, LAYOUT_TIME_MAJOR

_CORE_IMPORT_ERROR = None
try:
    from . import mic_eq_core as _core_module
    _lib.load()
except ImportError as error:  # the HIP library is missing or unloadable
    _core_module = None
    _CORE_IMPORT_ERROR = error


def _missing_core(*args, **kwargs):
    raise ImportError(
        "mic_eq_mi backend (libaudioforge_mi.so) is unavailable or missing this API. Build it with: "
        "python -c 'import __graft_entry__ as g; g.build()'"
    ) from _CORE_IMPORT_ERROR


_OPERATORS = (
    "simulate_auto_eq_chain",
    "simulate_auto_eq_chain_batch",
    "simulate_auto_makeup_control",
    "simulate_gate_suppressor_order",
    "simulate_eq_v2",
    "simulate_product_resampler",
    "product_resampler_configuration",
    "eq_magnitude_response",
    "eq_magnitude_response_v2",
    "measure_integrated_loudness",
    "compute_voice_spectrum",
    "compute_voice_spectrum_batch",
    "measure_voice_spectra",
    "analyze_voice_spectrum",
    "analyze_voice_spectrum_batch",
    "analyze_voice_capture_batch",
    "analyze_noise_reference",
    "analyze_noise_reference_batch",
    "measure_speech_features_batch",
    "recommend_voice_chain",
    "recommend_voice_chain_batch",
    "configure_voice_chain",
    "suppress",
    "rnnoise_benchmark",
)

CORE_AVAILABLE = _core_module is not None
for _name in _OPERATORS:
    globals()[_name] = getattr(_core_module, _name, _missing_core) if _core_module is not None else _missing_core
Engine = getattr(_core_module, "Engine", None) if _core_module is not None else None
NoiseSuppressor = getattr(_core_module, "NoiseSuppressor", None) if _core_module is not None else None
NoiseModel = getattr(_core_module, "NoiseModel", None) if _core_module is not None else None
StreamResampler = getattr(_core_module, "StreamResampler", None) if _core_module is not None else None
Mixdown = getattr(_core_module, "Mixdown", None) if _core_module is not None else None
VoiceSpectrum = getattr(_core_module, "VoiceSpectrum", None) if _core_module is not None else None
VoiceSpectrumResult = getattr(_core_module, "VoiceSpectrumResult", None) if _core_module is not None else None
NoiseReference = getattr(_core_module, "NoiseReference", None) if _core_module is not None else None
NoiseReferenceAnalysis = getattr(_core_module, "NoiseReferenceAnalysis", None) if _core_module is not None else None
SpeechFeatures = getattr(_core_module, "SpeechFeatures", None) if _core_module is not None else None
CaptureMetadata = getattr(_core_module, "CaptureMetadata", None) if _core_module is not None else None
new_noise_suppression_engine = (getattr(_core_module, "new_noise_suppression_engine", _missing_core)
                                if _core_module is not None else _missing_core)
# the compressor candidate sweep lives in a module of its own
if _core_module is not None:
    from .compressor_search import (CompressorSearch, calibrate_compressor, calibrate_compressor_batch, compressor_input_batch,
                                    simulate_compressor_candidates_batch)
else:
    CompressorSearch = None
    compressor_input_batch = simulate_compressor_candidates_batch = calibrate_compressor = calibrate_compressor_batch = _missing_core
# ... and so do the measurements of the second-passage verification
if _core_module is not None:
    from .setup_verification import (SetupVerification, decide_voice_setup_verification, measure_setup_verification_batch,
                                     validate_voice_setup_verification, verify_voice_setup_batch)
else:
    SetupVerification = None
    measure_setup_verification_batch = decide_voice_setup_verification = _missing_core
    verify_voice_setup_batch = validate_voice_setup_verification = _missing_core
# ... and the EQ headroom validation with its per-lane EQ
if _core_module is not None:
    from .headroom import (LaneEq, apply_headroom_validation, apply_headroom_validation_batch, simulate_candidate_chain,
                           simulate_candidate_chain_batch)
else:
    LaneEq = None
    simulate_candidate_chain = simulate_candidate_chain_batch = apply_headroom_validation = apply_headroom_validation_batch = _missing_core
# ... and the latency calibration
if _core_module is not None:
    from .latency_calibration import (LatencyCalibration, LatencyCalibrationResult, analyze_latency, analyze_latency_batch,
                                      generate_probe_signal, result_to_profile)
else:
    LatencyCalibration = LatencyCalibrationResult = None
    generate_probe_signal = analyze_latency = analyze_latency_batch = result_to_profile = _missing_core
# ... and the streaming lane chain (one lane per stream, per-stream settings)
if _core_module is not None:
    from .lane_chain import LaneChain
else:
    LaneChain = None

__all__ = ["LaneChain", "CORE_AVAILABLE", "Engine", "NoiseSuppressor", "NoiseModel", "StreamResampler", "Mixdown", "VoiceSpectrum", "VoiceSpectrumResult", "NoiseReference", "NoiseReferenceAnalysis", "SpeechFeatures", "CaptureMetadata",
           "new_noise_suppression_engine", *_OPERATORS, "CompressorSearch", "compressor_input_batch", "simulate_compressor_candidates_batch", "calibrate_compressor",
           "calibrate_compressor_batch", "SetupVerification", "measure_setup_verification_batch", "decide_voice_setup_verification", "verify_voice_setup_batch", "validate_voice_setup_verification", "LaneEq",
           "simulate_candidate_chain", "simulate_candidate_chain_batch", "apply_headroom_validation", "apply_headroom_validation_batch", "LatencyCalibration",
           "LatencyCalibrationResult", "generate_probe_signal", "analyze_latency", "analyze_latency_batch", "result_to_profile", "LAYOUT_STREAM_MAJOR", "LAYOUT_TIME_MAJOR", "KERNEL_AUTO",
           "KERNEL_LANE_PER_STREAM", "KERNEL_PHASED", "KERNEL_QUAD", "KERNEL_STAGED"]
