"""tests/ref/voice_spectrum_ref.c against what the reference's own spectrum.py returned (tests/golden/voice_spectrum.npz,
written by tools/gen_golden_voice_spectrum.py): discrete fields equal, dB fields within four times the largest difference
measured between the two (pocketfft's operation order is not the kernels'), every branch taken by at least one stream.
This is what holds the restatement to the reference; tests/test_gpu_voice_spectrum.py holds the kernels to the restatement."""
import functools

import numpy as np
import pytest

import voice_spectrum_oracle as VO
import voice_spectrum_stimulus as VS

# Largest |restatement - reference| per field over every value the fixture holds, measured on the build host (printed by the
# test below); four times that is allowed.  The per-bin SNR is the loosest: where speech and noise medians nearly coincide
# it divides a difference of nearly equal powers.
MEASURED_DB = {"frame_rms_db": 1.421e-14, "speech_db": 1.535e-12, "noise_db": 3.837e-13, "spectral_snr_db": 4.811e-09,
               "welch_db": 1.421e-13, "window_db": 1.208e-12, "window_smoothed_db": 2.700e-13}
# The same measurement for the two scalars of the fallback return.  Every fallback stream of the fixture with a noise reference
# sits on the clamp of spectrum.py:364 (-60 dB exactly), so the measured SNR difference is 0; 1e-12 dB (the resolution the GPU
# comparison uses) is added so that an ulp of another libm's log10 does not fail the test.
FALLBACK_MEASURED = {"snr_db": 0.0, "tilt": 7.105e-15}
SPECTRA = ("speech_db", "noise_db", "spectral_snr_db", "welch_db")


@functools.lru_cache(maxsize=None)
def results():
    """Every fixture case through the restatement, once: [(case, fixture arrays, [per-stream result])]."""
    out = []
    for case in VS.cases():
        fx = VS.fixture_case(case)
        rows = []
        for s in fx["streams"]:
            vad = case["vad"][s] if "vad" in case else None
            noise = case["noise"][s] if "noise" in case else None
            rows.append(VO.analyze(case["audio"][s], VS.FS, case["nperseg"], vad, noise))
        out.append((case, fx, rows))
    return out


def test_discrete_fields_equal_the_reference():
    for case, fx, rows in results():
        for i, r in enumerate(rows):
            want = fx["scalars"][i]
            where = (case["name"], int(fx["streams"][i]))
            assert (r["frames"], r["voiced"]) == (want[0], want[1]), where
            assert np.array_equal(r["voiced_mask"], fx["voiced_mask"][i]), where
            assert r["vad_probability_used"] == want[3] and r["noise_reference_source"] == want[5], where
            assert r["used_single_spectrum_fallback"] == want[6], where
            assert r["voiced_window_ratio"] == want[2] and r["vad_active_window_ratio"] == want[4], where


def test_db_fields_within_four_times_the_measured_difference():
    worst = dict.fromkeys(MEASURED_DB, 0.0)

    def note(field, got, want):
        assert np.array_equal(np.isnan(got), np.isnan(want)), field
        if not np.isnan(want).all():
            worst[field] = max(worst[field], float(np.nanmax(np.abs(got - want))))

    for case, fx, rows in results():
        chk = VS.checkpoint_bins(case["nperseg"] // 2 + 1)
        full = list(fx["full_streams"])
        for i, r in enumerate(rows):
            note("frame_rms_db", r["frame_rms_db"], fx["frame_rms_db"][i])
            for j, name in enumerate(SPECTRA):
                note(name, r[name][chk], fx["checkpoints"][i, j])
                if fx["streams"][i] in full:
                    note(name, r[name], fx["full_spectra"][full.index(fx["streams"][i]), j])
            if full and fx["streams"][i] == full[0]:
                note("window_db", r["win_db"][0], fx["full_windows"][0, 0])
                note("window_smoothed_db", r["win_smooth"][0], fx["full_windows"][0, 1])
    print("largest |restatement - reference| in dB:", {k: f"{v:.3e}" for k, v in worst.items()})
    for field, value in worst.items():
        assert value <= 4 * MEASURED_DB[field], (field, value)


def test_every_branch_is_taken():
    seen = set()
    for case, fx, rows in results():
        for i, r in enumerate(rows):
            if r["used_single_spectrum_fallback"]:
                seen.add("fallback")
            seen.add(VO.NOISE_SOURCES[r["noise_reference_source"]])
            if np.isnan(r["gates"][1]):
                seen.add("spread below 6 dB")
                assert r["voiced"] == r["frames"] or r["vad_probability_used"]
            if r["welch_segments"] < r["frames"]:
                seen.add("welch over compacted chunks")
            if r["vad_probability_used"]:
                plain = VO.analyze(case["audio"][fx["streams"][i]], VS.FS, case["nperseg"])
                fused = not np.array_equal(plain["voiced_mask"], r["voiced_mask"])
                seen.add("vad fused and accepted" if fused else "vad fused and rejected")
    assert seen >= {"fallback", "unavailable", "explicit_capture", "in_capture_non_speech", "spread below 6 dB",
                    "welch over compacted chunks", "vad fused and accepted", "vad fused and rejected"}, seen


def test_noise_capture_below_one_frame_is_ignored():
    case, fx, rows = next(r for r in results() if r[0]["name"] == "shortnoise256")
    assert VO.NOISE_SOURCES[rows[0]["noise_reference_source"]] == "in_capture_non_speech"


def test_audio_too_short_error_text():
    with pytest.raises(ValueError, match=r"Audio too short for FFT: need 256 samples, got 255 \(0\.01 seconds\)"):
        VO.analyze(np.zeros(255, dtype=np.float32), VS.FS, 256)


def test_frequency_grid_and_octave_band_tables_equal_the_reference():
    fx = VS.fixture()
    assert np.array_equal(VO.freqs(VS.FS, 256), fx["freqs256"])
    assert np.array_equal(VO.freqs(VS.FS, 4096)[VS.checkpoint_bins(2049)], fx["freqs4096_checkpoints"])
    for fraction in (2, 3, 6, 12):
        assert np.array_equal(np.stack(VO.octave_bands(fraction)), fx[f"octave{fraction}"]), fraction


def test_smoothing_follows_the_band_rule():
    """A flat spectrum stays flat, and a spectrum that steps at 1 kHz is smoothed to a monotone ramp of at most one band's width."""
    K = 129
    assert np.allclose(VO.smooth(np.full(K, -37.0), VS.FS, 256), -37.0, atol=1e-12)
    f = VO.freqs(VS.FS, 256)
    out = VO.smooth(np.where(f < 1000.0, -20.0, -40.0), VS.FS, 256)
    assert np.all(np.diff(out) <= 1e-12) and out[0] == pytest.approx(-20.0, abs=1e-9) and out[-1] == pytest.approx(-40.0, abs=1e-9)


def test_fallback_scalars_from_the_restatement_match_the_reference():
    """snr_db and spectral_tilt_db_per_octave of the fallback return (:626-632) are O(bins) host arithmetic in mic_eq_core;
    fed the restatement's spectra they reproduce the reference's values to what the spectra's own differences allow."""
    from mic_eq_mi import mic_eq_core as core

    worst_snr = worst_tilt = 0.0
    count = 0
    for case, fx, rows in results():
        freqs = VO.freqs(VS.FS, case["nperseg"])
        for i, r in enumerate(rows):
            if not r["used_single_spectrum_fallback"]:
                assert np.isnan(fx["scalars"][i, 7])
                continue
            noise = None if np.isnan(r["noise_db"][0]) else r["noise_db"]
            worst_snr = max(worst_snr, abs(core._estimate_snr_from_spectrum(freqs, r["welch_db"], noise) - fx["scalars"][i, 7]))
            worst_tilt = max(worst_tilt, abs(core._estimate_tilt_db_per_octave(freqs, r["welch_db"]) - fx["scalars"][i, 8]))
            count += 1
    print(f"{count} fallback streams: largest difference snr_db {worst_snr:.3e}, tilt {worst_tilt:.3e} dB/octave")
    assert count >= 8
    assert worst_snr <= 4 * FALLBACK_MEASURED["snr_db"] + 1e-12 and worst_tilt <= 4 * FALLBACK_MEASURED["tilt"] + 1e-12
