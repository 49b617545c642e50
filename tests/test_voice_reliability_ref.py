"""tests/ref/voice_reliability_ref.c (fed by tests/ref/voice_spectrum_ref.c) against what the reference's own
analyze_voice_spectrum returned (tests/golden/voice_reliability.npz, written by tools/gen_golden_voice_reliability.py): discrete
fields equal, every continuous field within four times the largest difference measured between the two on the build host.
This is what holds the restatement to the reference; tests/test_gpu_voice_reliability.py holds the kernels to the restatement."""
import functools

import numpy as np

import voice_reliability_oracle as VR
import voice_reliability_stimulus as RS
import voice_spectrum_oracle as VO
import voice_spectrum_stimulus as VS

# Largest |restatement - reference| per field over every value the fixture holds, measured on the build host (printed by the
# test below); four times that is allowed.  The smoothed rows the statistics start from differ by 2.7e-13 dB (window spectra
# 1.2e-12) between restatement and reference, tests/test_voice_spectrum_ref.py; medians and differences of them inherit that.
# The per-bin SNR and snr_db divide by a difference of nearly equal powers where the median sits on the noise reference.
# outlier_rejection_ratio is 1 - inliers / windows on both sides: the same two IEEE operations, so 0 is asserted as equality.
MEASURED = {"median_spectrum_db": 2.984e-13, "spectral_repeatability": 9.059e-14, "measurement_uncertainty_db": 2.645e-13,
            "spectral_snr_db": 1.027e-10, "window_distance": 5.231e-13, "snr_db": 5.684e-14, "spectral_tilt_db_per_octave": 1.954e-14,
            "residual_confidence": 1.332e-14, "measurement_coverage": 2.776e-15, "outlier_rejection_ratio": 0.0,
            "phonetic_coverage": 4.774e-15, "effective_measurement_blocks": 6.928e-14}


@functools.lru_cache(maxsize=None)
def results():
    """Every fixture case through both restatements, once: [(case, fixture arrays, [per-stream second half])]."""
    out = []
    for case in RS.cases():
        fx = RS.fixture_case(case["name"])
        rows = []
        for s in fx["streams"]:
            vad = case["vad"][s] if "vad" in case else None
            noise = case["noise"][s] if "noise" in case else None
            first = VO.analyze(case["audio"][s], RS.FS, case["nperseg"], vad, noise)
            rows.append((first, VR.from_first_half(first, RS.FS, case["nperseg"])))
        out.append((case, fx, rows))
    return out


def test_discrete_fields_equal_the_reference():
    for case, fx, rows in results():
        for i, (first, r) in enumerate(rows):
            where = (case["name"], int(fx["streams"][i]))
            assert (first["used_single_spectrum_fallback"], first["noise_reference_source"]) == tuple(fx["flags"][i]), where
            assert np.array_equal(first["voiced_mask"], fx["voiced_mask"][i]), where
            assert [r[k] for k in VR.COUNTS] == list(fx["counts"][i]), where
            assert np.array_equal(r["inlier_mask"], fx["inlier_mask"][i]), where


def test_continuous_fields_within_four_times_the_measured_difference():
    worst = dict.fromkeys(MEASURED, 0.0)

    def note(field, got, want):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want)), field
        assert np.array_equal(np.isinf(got), np.isinf(want)), field
        finite = np.isfinite(want)
        if finite.any():
            worst[field] = max(worst[field], float(np.max(np.abs(got[finite] - want[finite]))))

    for case, fx, rows in results():
        chk = VS.checkpoint_bins(case["nperseg"] // 2 + 1)
        full = list(fx["full_streams"])
        for i, (_, r) in enumerate(rows):
            for j, name in enumerate(RS.SCALARS):
                note(name, r[name], fx["scalars"][i, j])
            note("window_distance", r["window_distance"], fx["distance"][i])
            for j, name in enumerate(RS.SPECTRA):
                note(name, r[name][chk], fx["checkpoints"][i, j])
                if i in full:
                    note(name, r[name], fx["full_spectra"][full.index(i), j])
    print("largest |restatement - reference|:", {k: f"{v:.3e}" for k, v in worst.items()})
    for field, value in worst.items():
        assert value <= 4 * MEASURED[field], (field, value)


def test_every_path_is_taken():
    seen = set()
    for case, fx, rows in results():
        for first, r in rows:
            if first["used_single_spectrum_fallback"]:
                seen.add("fallback")
                continue
            seen.add("closest windows" if r["used_closest_windows"] else "cutoff")
            if r["inliers"] < r["voiced"]:
                seen.add("outliers rejected")
            seen.add("one block" if r["blocks"] < 2 else "blocks")
            eff = r["effective_measurement_blocks"]
            seen.add("fractional effective blocks" if eff != round(eff) else "whole effective blocks")
            if eff >= 12.0:
                seen.add("duration term clipped")
            seen.add("snr" if not np.isnan(r["spectral_snr_db"][0]) else "no snr")
            if np.any(r["spectral_snr_db"] == -60.0):
                seen.add("snr clamp")
            if np.isinf(r["measurement_uncertainty_db"]).all():
                seen.add("infinite uncertainty")
                assert not r["spectral_repeatability"].any()
    assert seen >= {"fallback", "closest windows", "cutoff", "outliers rejected", "one block", "blocks", "fractional effective blocks",
                    "whole effective blocks", "duration term clipped", "snr", "no snr", "snr clamp", "infinite uncertainty"}, seen
