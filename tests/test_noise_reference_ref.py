"""tests/ref/noise_reference_ref.c against what the reference's own analyze_noise_reference returned
(tests/golden/noise_reference.npz, written by tools/gen_golden_noise_reference.py): status, flags and the reason and guidance
lists equal, every continuous field within four times the largest difference measured between the two on the build host.  This
is what holds the restatement to the reference; tests/test_gpu_noise_reference.py holds the kernels to the restatement."""
import functools

import numpy as np

import noise_reference_oracle as NO
import noise_reference_stimulus as NS

# Largest |restatement - reference| per field over every value the fixture holds, measured on the build host (printed by the
# test below); four times that is allowed.  The restatement sums in the kernels' order where NumPy sums pairwise, and its
# transform is a mixed-radix one where NumPy's is pocketfft: linear quantities differ in the last bits, their dB by ~1e-14.
# The clipped streams carry the largest differences (spectra 1.6e-13 dB, and 8e-12 dB in the flux, a difference of band levels
# that are equal to 0.05 dB): their frames are dominated by full-scale samples, so every other bin sits 70 dB below the peak
# of the transform.  Fractions and counts are ratios of the same integers: exact.
MEASURED = {"quality_score": 4.441e-16, "duration_s": 0.0, "finite_fraction": 0.0, "noise_rms_db": 1.421e-14,
            "conservative_noise_rms_db": 1.421e-14, "noise_peak_db": 7.105e-15, "crest_factor_db": 1.421e-14, "clipped_fraction": 0.0,
            "zero_fraction": 0.0, "rms_spread_db": 7.105e-15, "octave_stability_db": 5.969e-13, "spectral_flux_db": 8.185e-12,
            "vad_contamination_ratio": 0.0, "vad_contamination_p90": 0.0, "capture_age_s": 0.0,
            "in_capture_level_delta_db": 1.421e-14, "spectral_shape_distance_db": 2.629e-13, "explicit_spectrum_db": 1.634e-13,
            "conservative_spectrum_db": 1.634e-13, "in_capture_spectrum_db": 8.527e-14}


@functools.lru_cache(maxsize=None)
def results():
    """Every stream of every batch through the restatement, once: {batch name: [per-stream dict]}."""
    out = {}
    for b in NS.batches():
        out[b["name"]] = [NO.analyze(b["noise"][s], None if b["speech"] is None else b["speech"][s], b["fs"],
                                     None if b["noise_vad"] is None else b["noise_vad"][s],
                                     None if b["speech_vad"] is None else b["speech_vad"][s], b["age"][s], int(b["mismatch"][s]))
                          for s in range(b["noise"].shape[0])]
    return out


def test_discrete_fields_and_text_lists_equal_the_reference():
    fx = NS.fixture()
    for name, rows in results().items():
        for s, r in enumerate(rows):
            where = (name, s)
            assert r["status"] == fx[f"{name}/status"][s], where
            usable, conservative, _, count = fx[f"{name}/flags"][s]
            assert (r["status"] != 2, bool(r["conservative"]), r["in_capture_noise_frame_count"]) == (bool(usable), bool(conservative), count), where
            reasons, guidance = (int(m) for m in fx[f"{name}/masks"][s])
            assert NO.texts(r["reasons"], NO.REASONS) == NO.texts(reasons, NO.REASONS), where
            assert NO.texts(r["guidance"], NO.GUIDANCE) == NO.texts(guidance, NO.GUIDANCE), where
            assert bool(r["has_in_capture_spectrum"]) == (not np.isnan(fx[f"{name}/checkpoints"][s, 2, 0])), where


def test_continuous_fields_within_four_times_the_measured_difference():
    fx = NS.fixture()
    worst = dict.fromkeys(MEASURED, 0.0)

    def note(field, got, want):
        got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
        assert np.array_equal(np.isnan(got), np.isnan(want)), field
        finite = np.isfinite(want)
        if finite.any():
            worst[field] = max(worst[field], float(np.max(np.abs(got[finite] - want[finite]))))

    for name, rows in results().items():
        chk = NS.checkpoint_bins(rows[0]["frequencies"].size)
        for s, r in enumerate(rows):
            note("quality_score", r["quality_score"], fx[f"{name}/quality"][s])
            for j, field in enumerate(NO.METRICS):
                note(field, r[field], fx[f"{name}/metrics"][s, j])
            for j, field in enumerate(NO.SPECTRA):
                note(field, r[field][chk], fx[f"{name}/checkpoints"][s, j])
        if f"{name}/full_spectra" in fx:
            full = fx[f"{name}/full_spectra"]
            note("explicit_spectrum_db", rows[0]["explicit_spectrum_db"], full[0])
            note("in_capture_spectrum_db", rows[0]["in_capture_spectrum_db"], full[1])
            note("conservative_spectrum_db", rows[0]["conservative_spectrum_db"], np.fmax(full[0], full[1]))
    print("largest |restatement - reference|:", {k: f"{v:.3e}" for k, v in worst.items()})
    for field, value in worst.items():
        assert value <= 4 * MEASURED[field], (field, value)


def test_every_path_is_taken():
    seen, reasons = set(), 0
    for name, rows in results().items():
        b = NS.batch(name)
        for r in rows:
            seen.add(NO.STATUS[r["status"]])
            reasons |= r["reasons"]
            if r["noise_frames"] == 0:
                seen.add("noise below a frame")
                if r["has_in_capture_spectrum"]:
                    seen.add("in-capture on the short grid")
            if b["speech"] is None:
                seen.add("no voice")
            elif r["has_in_capture_spectrum"]:
                seen.add("selected with vad" if b["speech_vad"] is not None else "selected without vad")
            elif b["speech_vad"] is not None and r["in_capture_noise_frame_count"] > 0:
                seen.add("too few frames")
            elif b["speech_vad"] is None:
                seen.add("spread below 6")
            if r["n_bands"] < 7:
                seen.add("empty bands")
    assert reasons == (1 << len(NO.REASONS)) - 1, f"{reasons:#x}"
    assert seen >= {"usable", "questionable", "invalid", "noise below a frame", "in-capture on the short grid", "no voice",
                    "selected with vad", "selected without vad", "too few frames", "spread below 6", "empty bands"}, seen


def test_factor_plans():
    """The factor order the transform takes: largest radix first."""
    assert NO.plan(2560) == [2] * 8 and NO.frame_size(2560) == 512
    assert NO.plan(3000) == [5, 5, 3, 2, 2]            # 600 = 2^3 3 5^2: M = 300
    assert NO.plan(3150) == [7, 5, 3, 3]               # 630: M = 315
    assert NO.plan(4410) == [7, 7, 3, 3]               # 882: M = 441
    assert NO.plan(48_000) == [5, 5, 3, 2, 2, 2, 2, 2, 2] and NO.frame_size(48_000) == 9600
    assert NO.plan(11_025) is None                     # 2205 samples: odd
    assert NO.plan(2750) is None                       # 550: M = 275 = 5^2 11
