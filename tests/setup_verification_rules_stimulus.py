"""Hand-made inputs for the rules of the second-passage verification (voice_setup.py:1484-1495, :1590-1679): one base case the
reference accepts, and cases that move one quantity to each side of each threshold of the ladder, in the ladder's order, trip two
rungs at once, leave keys out, or take an early exit.  The generator feeds them to the reference's own
validate_voice_setup_verification with its measuring helpers answered from these numbers; the tests feed them to the restatement.

A case is the base with overrides.  `sim` is the simulation dict of the verification passage and `compressor` / `deesser` the
settings; a key set to None is left out of the dict."""
from __future__ import annotations

import copy

FS = 48_000
NUMBER_KEYS = ("spectral_target_error_before_db", "spectral_target_error_after_db", "loudness_variation_before_db",
               "loudness_variation_after_db", "noise_floor_change_db", "relative_noise_floor_change_db", "snr_change_db",
               "compressor_gain_reduction_median_db", "compressor_gain_reduction_p95_db", "compressor_gain_reduction_peak_db",
               "deesser_gain_reduction_median_db", "deesser_gain_reduction_p95_db", "output_true_peak_db")
EARLY_KEYS = {"decision", "reasons", "perceptual_validation"}

BASE = {
    "samples": 201_600, "peak": 0.5, "non_finite": False, "rendered_peak": 0.6, "backend": "rust",
    "rms": {"noise": -60.0, "original": -20.0, "verification": -21.0, "rendered": -19.0, "rendered_noise": -58.5},
    "error_before": 3.0, "error_after": 2.5, "shape_delta": 1.0, "snr_before": 30.0, "snr_after": 29.0,
    "spread_before": 6.5, "spread_after": 4.25,
    "sim": {"compressor_gain_reduction_p95_db": 3.0, "compressor_gain_reduction_db": 5.0, "output_true_peak_db": -1.75,
            "limiter_effective_ceiling_db": -1.5, "true_peak_limited_events": 0, "output_rms_db": -19.0, "input_rms_db": -21.0,
            "deesser_gain_reduction_p95_db": 1.0, "compressor_gain_reduction_median_db": 1.25,
            "deesser_gain_reduction_median_db": 0.5},
    "compressor": {"target_p95_reduction_db": 3.5, "peak_reduction_cap_db": 8.0},
    "deesser": {"max_reduction_db": 6.0},
}

# (name, overrides, the decision the ladder must give as written).  Numbers are binary fractions where a threshold is met exactly.
CASES = [
    ("base", {}, "accept"),
    # :1608 retry
    ("level_8_is_not_more", {"rms": {"verification": -28.0}, "sim": {"input_rms_db": -28.0, "output_rms_db": -26.0}}, "accept"),
    ("level_quieter", {"rms": {"verification": -28.5}, "sim": {"input_rms_db": -28.5, "output_rms_db": -26.5}}, "retry"),
    ("level_louder", {"rms": {"verification": -11.5}, "sim": {"input_rms_db": -11.5, "output_rms_db": -9.5}}, "retry"),
    ("shape_below", {"shape_delta": 4.875}, "accept"),
    ("shape_above", {"shape_delta": 5.125}, "retry"),
    ("retry_beats_rollback", {"shape_delta": 5.125, "error_after": 9.0, "sim": {"compressor_gain_reduction_db": 12.0}}, "retry"),
    # :1611-1617 rollback
    ("error_plus_1_is_not_more", {"error_after": 4.0}, "accept"),
    ("error_worse", {"error_after": 4.125}, "rollback"),
    ("relative_noise_4_is_not_more", {"rms": {"rendered_noise": -54.0}}, "reduce"),  # 6 - 2 = 4: past 3, not past 4
    ("relative_noise_above_4", {"rms": {"rendered_noise": -53.75}}, "rollback"),
    ("snr_minus_4_is_not_less", {"snr_after": 26.0}, "accept"),
    ("snr_lost", {"snr_after": 25.875}, "rollback"),
    ("peak_at_cap_plus_quarter", {"sim": {"compressor_gain_reduction_db": 8.25}}, "accept"),
    ("peak_over_cap", {"sim": {"compressor_gain_reduction_db": 8.375}}, "rollback"),
    ("true_peak_under", {"sim": {"output_true_peak_db": -1.375}}, "accept"),
    ("true_peak_over", {"sim": {"output_true_peak_db": -1.25}}, "rollback"),
    ("rollback_beats_reduce", {"sim": {"compressor_gain_reduction_db": 9.0, "true_peak_limited_events": 3,
                                       "compressor_gain_reduction_p95_db": 6.0}}, "rollback"),
    # :1620-1627 reduce
    ("p95_at_target_plus_three_quarters", {"sim": {"compressor_gain_reduction_p95_db": 4.25}}, "accept"),
    ("p95_over", {"sim": {"compressor_gain_reduction_p95_db": 4.375}}, "reduce"),
    ("limiter_events", {"sim": {"true_peak_limited_events": 1}}, "reduce"),
    ("relative_noise_3_is_not_more", {"rms": {"rendered_noise": -55.0}}, "accept"),
    ("relative_noise_above_3", {"rms": {"rendered_noise": -54.875}}, "reduce"),
    ("deesser_under", {"sim": {"deesser_gain_reduction_p95_db": 5.25}}, "accept"),
    ("deesser_over", {"sim": {"deesser_gain_reduction_p95_db": 5.5}}, "reduce"),
    # settings of another intensity
    ("dense_profile_accepts_more", {"compressor": {"target_p95_reduction_db": 5.5, "peak_reduction_cap_db": 10.0},
                                    "sim": {"compressor_gain_reduction_p95_db": 6.0, "compressor_gain_reduction_db": 10.125}}, "accept"),
    ("dense_profile_over", {"compressor": {"target_p95_reduction_db": 5.5, "peak_reduction_cap_db": 10.0},
                            "sim": {"compressor_gain_reduction_p95_db": 6.375}}, "reduce"),
    # absent keys and their defaults
    ("no_p95_is_120", {"sim": {"compressor_gain_reduction_p95_db": None}}, "reduce"),
    ("no_peak_is_120", {"sim": {"compressor_gain_reduction_db": None}}, "rollback"),
    ("no_true_peak_is_120", {"sim": {"output_true_peak_db": None}}, "rollback"),
    ("no_ceiling_is_minus_1_5", {"sim": {"limiter_effective_ceiling_db": None, "output_true_peak_db": -1.25}}, "rollback"),
    ("no_ceiling_accepts_below", {"sim": {"limiter_effective_ceiling_db": None}}, "accept"),
    ("no_events_is_0", {"sim": {"true_peak_limited_events": None}}, "accept"),
    ("no_rms_keys_use_the_measured_levels", {"sim": {"output_rms_db": None, "input_rms_db": None},
                                             "rms": {"rendered": -18.0, "rendered_noise": -54.875}}, "accept"),  # gain 3: relative 2.125
    ("no_deesser_p95_is_0", {"sim": {"deesser_gain_reduction_p95_db": None, "deesser_gain_reduction_median_db": None,
                                     "compressor_gain_reduction_median_db": None}}, "accept"),
    ("no_target_p95_is_3_5", {"compressor": {"target_p95_reduction_db": None}, "sim": {"compressor_gain_reduction_p95_db": 4.375}}, "reduce"),
    ("no_peak_cap_is_8", {"compressor": {"peak_reduction_cap_db": None}, "sim": {"compressor_gain_reduction_db": 8.375}}, "rollback"),
    ("no_max_reduction_is_6", {"deesser": {"max_reduction_db": None}, "sim": {"deesser_gain_reduction_p95_db": 5.5}}, "reduce"),
    ("larger_max_reduction", {"deesser": {"max_reduction_db": 8.0}, "sim": {"deesser_gain_reduction_p95_db": 5.5}}, "accept"),
    ("no_settings_at_all", {"compressor": {"target_p95_reduction_db": None, "peak_reduction_cap_db": None},
                            "deesser": {"max_reduction_db": None}}, "accept"),
    # the output's own flag does not move the decision
    ("rendered_clipped", {"rendered_peak": 1.0}, "accept"),
    # early exits
    ("too_short", {"samples": 143_999}, "retry"),
    ("just_long_enough", {"samples": 144_000}, "accept"),
    ("clipped_0999", {"peak": 0.999}, "retry"),
    ("below_0999", {"peak": 0.998}, "accept"),
    ("non_finite", {"non_finite": True}, "retry"),
    ("not_rust", {"backend": "python"}, "retry"),
]


def case(overrides: dict) -> dict:
    out = copy.deepcopy(BASE)
    for key, value in overrides.items():
        if isinstance(value, dict):
            out[key].update(value)
        else:
            out[key] = value
    for group in ("sim", "compressor", "deesser"):
        out[group] = {k: v for k, v in out[group].items() if v is not None}
    return out
