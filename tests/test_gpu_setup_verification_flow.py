"""The second-passage measurements on measured spectra: the six chain pairs of tests/speech_features_stimulus.py go through
analyze_voice_spectrum_batch three times (setup passage, verification passage with the room tone, "rendered" passage with the
"rendered" room tone), the records of SetupVerification.measure are held to the restatement on the same spectra and signals, and
decide_voice_setup_verification turns them into the reference's dict -- the order of calls INTEGRATION.md gives.

The chain is not under test here (the operator that renders is not built): the "rendered" side is the verification side at exactly
half the amplitude, a power of two, so every property below is known in advance: the shape error is level-invariant, the noise
floor and the speech fall by the same 6.02 dB."""
import numpy as np
import pytest

import setup_verification_oracle as O
import speech_features_stimulus as ST

pytestmark = pytest.mark.gpu

NPERSEG = 4096
DB_ALLOWED = 1e-12  # kernels against the restatement, as tests/test_gpu_setup_verification_kernels.py


@pytest.fixture(scope="module")
def flow():
    import mic_eq_mi

    cb = ST.chain_batch()
    setup, noise = np.ascontiguousarray(cb["speech"]), np.ascontiguousarray(cb["noise"])
    verification = np.ascontiguousarray(setup[:, ::-1])  # the same delivery, another passage
    rendered, rendered_noise = verification * np.float32(0.5), noise * np.float32(0.5)
    spectra = [
        mic_eq_mi.analyze_voice_spectrum_batch(setup, ST.FS, NPERSEG),
        mic_eq_mi.analyze_voice_spectrum_batch(verification, ST.FS, NPERSEG, noise_audio=noise),
        mic_eq_mi.analyze_voice_spectrum_batch(rendered, ST.FS, NPERSEG, noise_audio=rendered_noise)]
    stack = lambda results, name: np.stack([getattr(r, name) for r in results])  # noqa: E731
    original_db, before_db, after_db = (stack(s, "median_spectrum_db") for s in spectra)
    snr = stack(spectra[2], "spectral_snr_db")
    presets = ["broadcast", "podcast", "streaming", "flat", "broadcast", "podcast"]
    handle = mic_eq_mi.SetupVerification(ST.FS, NPERSEG, setup.shape[0])
    rows = handle.measure(original_db, before_db, after_db, presets, snr, noise=noise, original=setup, verification=verification,
                          rendered=rendered, rendered_noise=rendered_noise)
    handle.close()
    signals = (noise, setup, verification, rendered, rendered_noise)
    return dict(mi=mic_eq_mi, spectra=spectra, original_db=original_db, before_db=before_db, after_db=after_db, snr=snr,
                presets=presets, rows=rows, signals=signals)


def test_records_on_measured_spectra_match_the_restatement(flow):
    f = O.grid(NPERSEG)
    assert np.array_equal(f, flow["spectra"][1][0].freqs)
    worst = 0.0
    for s, got in enumerate(flow["rows"]):
        want = O.measure_row(f, flow["original_db"][s], flow["before_db"][s], flow["after_db"][s], flow["snr"][s], flow["presets"][s],
                             [x[s] for x in flow["signals"]])
        for name in ("masked_bins", "snr_available", "band_present", "band_snr_db", "sum_squares", "peak", "non_finite", "clipped_0999",
                     "clipped_1"):
            assert np.array_equal(got[name], want[name], equal_nan=True), (s, name)
        for name in ("spectral_target_error_before_db", "spectral_target_error_after_db", "shape_delta_db", "rms_db", "offsets_before",
                     "offsets_after"):
            worst = max(worst, float(np.max(np.abs(np.asarray(got[name]) - np.asarray(want[name])))))
    print(f"largest |kernel - restatement| over the dB fields on measured spectra = {worst:.3e}")
    assert worst <= DB_ALLOWED


def test_a_pure_gain_changes_nothing_the_rules_read(flow):
    rows = flow["rows"]
    assert np.all(rows["masked_bins"] == 1018) and np.all(rows["band_present"] == 1)
    assert np.all(np.isfinite(rows["spectral_target_error_before_db"]))
    # Half the amplitude is -6.0206 dB on every bin but for the 1e-12 inside the spectrum's 10 log10(psd + 1e-12): a bin at L dB
    # moves by another 4.343 * 3e-12 / 10^(L / 10) dB, 4.1e-4 dB at -75 dB.  The level-invariant error is an RMS of centred
    # differences, so it moves by at most twice the largest such deviation: 1e-3 dB while no masked bin lies below -75 dB.
    f = O.grid(NPERSEG)
    mask = (f >= 80.0) & (f <= 12_000.0)
    assert flow["after_db"][:, mask].min() >= -75.0
    moved = float(np.max(np.abs(rows["spectral_target_error_after_db"] - rows["spectral_target_error_before_db"])))
    print(f"largest |error after - error before| under a pure gain = {moved:.3e} dB")
    assert moved <= 1e-3
    gain = 20.0 * np.log10(0.5)
    assert np.max(np.abs(rows["rms_db"][:, 3] - rows["rms_db"][:, 2] - gain)) <= 1e-3  # (the 1e-9 inside _rms_db's log)
    assert np.max(np.abs(rows["rms_db"][:, 4] - rows["rms_db"][:, 0] - gain)) <= 1e-3
    assert np.all(rows["sum_squares"][:, 3] == rows["sum_squares"][:, 2] / 4.0)  # a power of two: exact
    assert not rows["non_finite"].any() and not rows["clipped_1"].any()


def test_rules_on_the_measured_records(flow):
    mi, rows, spectra = flow["mi"], flow["rows"], flow["spectra"]
    simulation = {"simulation_backend": "rust", "compressor_gain_reduction_p95_db": 3.0, "compressor_gain_reduction_db": 5.0,
                  "output_true_peak_db": -7.5, "limiter_effective_ceiling_db": -1.5, "true_peak_limited_events": 0}
    setup_result = {"compressor": {"target_p95_reduction_db": 3.5, "peak_reduction_cap_db": 8.0}, "deesser": {"max_reduction_db": 6.0}}
    for s in range(rows.size):
        kwargs = dict(verification_samples=flow["signals"][2].shape[1], before_snr_db=spectra[1][s].snr_db, after_snr_db=spectra[2][s].snr_db,
                      loudness_variation_before_db=5.0, loudness_variation_after_db=4.0)
        verdict = mi.decide_voice_setup_verification(rows[s], simulation, setup_result, **kwargs)
        assert verdict["decision"] == "accept" and verdict["reasons"] == ["repeatability and native-chain constraints passed"], (s, verdict)
        assert set(verdict["frequency_dependent_snr_db"]) == {"low", "body", "presence", "sibilance"}
        assert abs(verdict["relative_noise_floor_change_db"]) <= 1e-3  # (the 1e-9 inside _rms_db's log on both sides)
        assert verdict["snr_change_db"] == spectra[2][s].snr_db - spectra[1][s].snr_db
        assert verdict["clipped"] is False and verdict["limiter_activity_events"] == 0
        hot = dict(simulation, true_peak_limited_events=4)
        assert mi.decide_voice_setup_verification(rows[s], hot, setup_result, **kwargs)["decision"] == "reduce"
        assert mi.decide_voice_setup_verification(rows[s], hot, setup_result, **dict(kwargs, verification_samples=100_000)) == {
            "decision": "retry", "reasons": ["verification passage was too short"], "perceptual_validation": False}
