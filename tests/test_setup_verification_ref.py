"""The restatement of the second-passage measurements (csrc/af_setup_verification_math.h through tests/ref/setup_verification_ref.c)
against what the reference's own get_target_curve, _shape_error_db and _rms_db returned on the closed-form stimulus
(tests/golden/setup_verification.npz, tools/gen_golden_setup_verification.py), and against NumPy for the rules the reference
writes inline (np.median, np.interp, np.sum).  No GPU.

The restatement adds over bins in the kernels' order (256 lanes, then a halving tree), NumPy pairwise: the difference is rounding
of f64 sums of a few dB.  MEASURED is the largest difference seen, and four times it is allowed here; the GPU tests hold the
kernels to this restatement."""
import pathlib

import numpy as np
import pytest

import setup_verification_oracle as O
import setup_verification_stimulus as SV

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "setup_verification.npz"
MEASURED = {"shape_error_db": 3.6e-15, "target_curve_db": 2.0e-15, "rms_db": 1.8e-15}  # largest |restatement - reference| seen
RESTATEMENT_ERROR = 1e-9  # above this a difference is an error of the restatement, not rounding


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_shape_error_matches_the_reference(golden):
    worst = 0.0
    assert golden["errors"].shape == (len(SV.NPERSEGS), len(SV.SPECTRA), len(SV.PRESETS))
    for g, nperseg in enumerate(SV.NPERSEGS):
        f = SV.grid(nperseg)
        for i, name in enumerate(SV.SPECTRA):
            for j, preset in enumerate(SV.PRESETS):
                want = float(golden["errors"][g, i, j])
                got, _ = O.shape_error_db(f, SV.spectrum(name, nperseg), preset)
                if SV.MASKED_BINS[nperseg] < 8:
                    assert np.isposinf(want) and np.isposinf(got), (nperseg, name, preset)
                else:
                    worst = max(worst, abs(got - want))
    print(f"largest |shape error - reference| = {worst:.3e} dB")
    assert worst <= RESTATEMENT_ERROR
    assert worst <= 4 * MEASURED["shape_error_db"]


def test_restatement_counts_the_masked_bins_even_odd_and_too_few():
    for nperseg, count in SV.MASKED_BINS.items():
        f = SV.grid(nperseg)
        db = SV.spectrum("voice", nperseg)
        row = O.measure_row(f, db, db, db, None, "broadcast", [None] * 5)
        assert row["masked_bins"] == count == int(np.count_nonzero((f >= 80.0) & (f <= 12_000.0)))
        assert np.isposinf(row["spectral_target_error_before_db"]) == (count < 8)
        assert row["shape_delta_db"] == 0.0  # a passage against itself
    assert SV.MASKED_BINS[4096] % 2 == 0 and SV.MASKED_BINS[2048] % 2 == 1 and SV.MASKED_BINS[16] < 8 <= SV.MASKED_BINS[64]


def test_adaptive_target_curve_matches_the_reference(golden):
    worst, seen = 0.0, 0
    for key in golden.files:
        kind, *rest = key.split("/")
        if kind != "curve":
            continue
        nperseg, name, preset = int(rest[0]), rest[1], rest[2]
        f = SV.grid(nperseg)
        mask = (f >= 80.0) & (f <= 12_000.0)
        got, _ = O.target_curve(f[mask], preset, SV.spectrum(name, nperseg)[mask])
        worst = max(worst, float(np.max(np.abs(got - golden[key]))))
        seen += 1
    print(f"largest |target curve - reference| = {worst:.3e} dB over {seen} curves")
    assert seen >= 4 * (len(SV.SPECTRA) + len(SV.CLIP_CASES) + 1)
    assert worst <= RESTATEMENT_ERROR
    assert worst <= 4 * MEASURED["target_curve_db"]


def test_catalog_curve_is_exact_and_unknown_preset_is_the_reference_error(golden):
    for preset in SV.PRESETS:  # interpolation of ten catalog points with held ends: the same operations, so the same bits
        got, _ = O.target_curve(SV.grid(64), preset, None)
        assert np.array_equal(got, golden[f"static/{preset}"])
    with pytest.raises(ValueError) as error:
        O.target_curve(SV.grid(64), "warm", None)
    assert str(error.value) == str(golden["unknown_preset_message"])


def test_every_reachable_clip_is_driven_to_both_ends():
    f = SV.grid(2048)
    mask = (f >= 80.0) & (f <= 12_000.0)
    ends = set()
    for name, (which, sign) in SV.CLIP_CASES.items():
        _, s = O.target_curve(f[mask], "broadcast", SV.spectrum(name, 2048)[mask])
        if which == "tilt":
            assert sign * s["tilt_db_per_octave"] / 4.0 > 1.0
            assert s["presence_offset"] == pytest.approx(0.8 * s["low_mid_balance"] - 0.5 * sign, abs=1e-15)
            _, flat = O.target_curve(f[mask], "flat", SV.spectrum(name, 2048)[mask])
            assert flat["flat_scale"] == -0.6 * sign  # the flat branch at the end of tilt_norm
        elif which == "low_mid_balance":
            assert s["low_mid_balance"] == float(sign)
            assert s["warmth_offset"] == -0.9 * sign
        else:
            assert (s["sibilance_db"] - s["presence_db"]) / 7.0 > 1.0 and s["sibilance_offset"] == -1.2
        ends.add((which, sign))
    _, s = O.target_curve(f[mask], "broadcast", SV.spectrum("presence_heavy", 2048)[mask])
    assert (s["sibilance_db"] - s["presence_db"]) / 7.0 < -1.0 and s["sibilance_offset"] == 1.2  # sibilance_ratio -> -1
    assert ends == {("tilt", 1), ("tilt", -1), ("low_mid_balance", 1), ("low_mid_balance", -1), ("sibilance", 1)}


def test_flat_preset_takes_its_own_branch():
    f = SV.grid(2048)
    mask = (f >= 80.0) & (f <= 12_000.0)
    db = SV.spectrum("tilt_up", 2048)[mask]
    flat, s = O.target_curve(f[mask], "flat", db)
    ramp = np.interp(f[mask], [100.0, 1000.0, 8000.0], [-1.0, 0.0, 1.0])
    assert np.array_equal(flat, 0.0 + np.clip(s["flat_scale"] * ramp, -1.0, 1.0))  # catalog zeros plus target.py:48-51
    assert np.max(np.abs(flat)) <= 0.6


def test_levels_match_numpy_bit_for_bit_and_the_reference(golden):
    rng = np.random.default_rng(7)
    for n in (0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 4097, 8191, 8192, 8193, 32_768, 32_769, 201_600):
        x = rng.standard_normal(n).astype(np.float32)
        a = x.astype(np.float64)
        assert O.sum_squares(x) == float(np.sum(a * a)), n  # NumPy's own order: equal bits
    worst = 0.0
    for n in SV.LENGTHS:
        worst = max(worst, abs(O.rms_db(SV.signal(n, n % 7)) - float(golden[f"rms_db/{n}"])))
    print(f"largest |rms_db - reference| = {worst:.3e} dB")
    assert worst <= 4 * MEASURED["rms_db"]
    assert O.rms_db(np.zeros(0, dtype=np.float32)) == float(golden["rms_db/0"]) == -120.0


def test_repeatability_delta_is_interp_median_rms():
    f = SV.grid(2048)
    original, before, _, _, _ = SV.batch(2048, 3)
    mask = (f >= 80.0) & (f <= 12_000.0)
    worst = 0.0
    for f0, o in ((f, original[1]), (SV.grid(4096), SV.batch(4096, 3)[0][1])):  # the shared grid, and a finer original
        delta = before[1][mask] - np.interp(f, f0, o)[mask]
        delta -= float(np.median(delta))
        want = float(np.sqrt(np.mean(np.square(delta))))
        worst = max(worst, abs(O.repeatability_delta_db(f, before[1], f0, o) - want))
    print(f"largest |repeatability delta - NumPy| = {worst:.3e} dB")
    assert worst <= 1e-12


def test_snr_band_medians_follow_np_median():
    for nperseg in (4096, 2048, 64, 16):
        f = SV.grid(nperseg)
        _, _, _, snr, _ = SV.batch(nperseg, 3)
        for s in range(3):
            want = {}
            for name, low, high in (("low", 80.0, 250.0), ("body", 250.0, 1_000.0), ("presence", 1_000.0, 4_500.0),
                                    ("sibilance", 4_500.0, 10_000.0)):
                mask = (f >= low) & (f < high)
                if np.any(mask):
                    want[name] = float(np.median(snr[s][mask]))
            got = O.snr_band_medians(f, snr[s])
            assert got.keys() == want.keys(), (nperseg, s)
            for name in want:  # selections: equal bits, NaN where NumPy says NaN
                assert got[name] == want[name] or (np.isnan(got[name]) and np.isnan(want[name])), (nperseg, s, name)
        assert O.snr_band_medians(f, None) == {}
    assert set(O.snr_band_medians(SV.grid(64), SV.batch(64, 1)[3][0])) == {"body", "presence", "sibilance"}  # 750 Hz bins: no low band
    assert np.isnan(O.snr_band_medians(SV.grid(2048), SV.batch(2048, 3)[3][1])["body"])
