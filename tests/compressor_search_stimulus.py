"""Stimulus of the compressor calibration search tests: seven 1 s captures (tests/signals.kat_signal at 48 kHz with a
333-sample tail, so the last control block is partial) with the settings and targets that drive the reference's
_calibrate_compressor_threshold (python/mic_eq/analysis/voice_setup.py:742-1079) through every outcome class the fixture
tests/golden/compressor_search.npz (tools/gen_golden_compressor_search.py) asserts."""
from __future__ import annotations

import pathlib

import numpy as np

import signals as S

FS = 48_000
N = 48_333
FIXTURE = pathlib.Path(__file__).resolve().parent / "golden" / "compressor_search.npz"
CONTROLS = ("threshold_db", "ratio", "attack_ms", "release_ms")
EQ_SETTINGS = {"band_freqs": [80.0, 160.0, 320.0, 640.0, 1280.0, 2500.0, 5000.0, 8000.0, 12000.0, 16000.0],
               "band_gains": [-1.5, 0.5, 0.0, -1.0, 0.5, 1.0, 2.0, 1.5, 0.5, -0.5], "band_qs": [1.41] * 10}
DEESSER_OFF = {"enabled": False}
DEESSER_ON = {"enabled": True, "auto_enabled": True, "auto_amount": 0.6, "low_cut_hz": 4500.0, "high_cut_hz": 10_000.0, "threshold_db": -28.0,
              "ratio": 4.0, "attack_ms": 2.0, "release_ms": 80.0, "max_reduction_db": 6.0}
DEFAULT_TARGETS = (3.5, 1.5, 8.0)  # p95, median, peak cap


def _compressor(threshold, ratio, attack, release, **more) -> dict:
    d = {"enabled": True, "threshold_db": threshold, "ratio": ratio, "attack_ms": attack, "release_ms": release, "makeup_gain_db": 0.0,
         "adaptive_release": True, "base_release_ms": 60.0, "auto_makeup_enabled": False, "target_lufs": -18.0,
         "sidechain_highpass_enabled": True, "measured_short_term_lufs": -19.0, "dynamics_intensity": "balanced"}
    d.update(more)
    return d


# name, level, de-esser, compressor settings, (target_p95_db, target_median_db, peak_cap_db)
CASES = (
    ("local_step", 1.0, DEESSER_OFF, _compressor(-24.0, 4.5, 5.0, 100.0), (6.0, 2.5, 9.0)),
    ("halton", 0.2, DEESSER_OFF, _compressor(-24.0, 5.5, 4.0, 120.0, measured_short_term_lufs=-20.0, adaptive_release=False), (8.0, 4.8, 8.6)),
    ("threshold_only", 1.0, DEESSER_ON, _compressor(-24.0, 2.0, 20.0, 300.0, adaptive_release=False), (2.0, 0.8, 5.0)),
    ("no_feasible", 1.0, DEESSER_OFF, _compressor(-24.0, 4.0, 10.0, 200.0), (3.5, 1.5, -1.0)),
    ("auto_makeup", 0.5, DEESSER_OFF, _compressor(-22.0, 3.0, 8.0, 150.0, auto_makeup_enabled=True, makeup_gain_db=3.0, target_lufs=-16.0,
                                                  measured_short_term_lufs=-24.0), DEFAULT_TARGETS),
    ("out_of_bounds", 0.1, DEESSER_OFF, _compressor(-60.0, 8.0, 1.0, 400.0, sidechain_highpass_enabled=False, makeup_gain_db=1.5,
                                                    measured_short_term_lufs=-38.0), DEFAULT_TARGETS),
    ("grid_point", 0.7, DEESSER_OFF, _compressor(-24.375, 3.0, 10.0, 180.0, measured_short_term_lufs=-21.0), DEFAULT_TARGETS),
)
NAMES = tuple(case[0] for case in CASES)
DIAGNOSTIC_NUMBERS = ("measured_median_gain_reduction_db", "measured_p95_gain_reduction_db", "measured_peak_gain_reduction_db",
                      "active_reduction_ratio", "total_objective", "incumbent_objective", "threshold_only_objective",
                      "expanded_candidate_objective", "active_output_gain_db", "silence_output_gain_db", "compressor_pumping_score_db",
                      "output_true_peak_db", "pre_limiter_true_peak_headroom_db")


def captures() -> np.ndarray:
    base = S.kat_signal(-(-N // 480))[:N].astype(np.float64)
    return np.stack([(level * base).astype(np.float32) for _, level, *_ in CASES])


def arguments() -> dict:
    """The keyword arguments of calibrate_compressor_batch for the whole stimulus."""
    return {"eq_settings": EQ_SETTINGS, "deesser_settings": [dict(c[2]) for c in CASES], "compressor_settings": [dict(c[3]) for c in CASES],
            "target_p95_db": [c[4][0] for c in CASES], "target_median_db": [c[4][1] for c in CASES], "peak_cap_db": [c[4][2] for c in CASES]}


def fixture():
    return np.load(FIXTURE, allow_pickle=False)
