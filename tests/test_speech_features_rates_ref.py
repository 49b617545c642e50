"""tests/ref/speech_features_rates_ref.c (the device-rate kernels' arithmetic restated, with csrc/af_speech_features_math.h behind
it) against what the reference and scipy returned for the same stimuli (tests/golden/speech_features_rates.npz, written by
tools/gen_golden_speech_features_rates.py).

The resampler: lengths equal; values differ from scipy.signal.resample_poly's only through the filter, which the header designs
itself (firwin, Kaiser 5.0, i0 by its series) and which agrees with scipy's to a few ulp of its peak -- the sum behind it is
scipy's, in scipy's order, and is held bit for bit to a plain double loop in NumPy over the same table.  The features at 16,
32, 44.1 and 96 kHz: counts, masks, indices, durations and peak_hz equal, the continuous fields within four times the largest
difference measured here (MEASURED; the convention of tests/test_speech_features_ref.py).  The 48 kHz geometry through the
rate-taking forms of the header gives the 48 kHz forms' bits.  Every test prints what it measured before it asserts."""
import functools

import numpy as np
import pytest

import speech_features_oracle as SO
import speech_features_rates_oracle as RO
import speech_features_rates_stimulus as RS
import speech_features_stimulus as SS
from test_speech_features_ref import COUNTS, FAMILY, SCALARS

# the largest |restatement - reference| per family over every stream of every analysed batch, as measured by this file
MEASURED = {"exact": 0.0, "loudness": 1.9e-13, "level_db": 1.3e-13, "feature": 1.9e-13, "probability": 2.8e-14}
# the largest |restated resampler - scipy.signal.resample_poly| over the peak of scipy's output, over the seven rates
MEASURED_RESAMPLE = 4.0e-15  # at 22.05 kHz (6401 taps); 2.7e-16 .. 7.8e-16 at the other rates
FRAME_STREAMS = (1, 66)
RESAMPLED = tuple(fs for fs in RS.RATES if fs != 48_000)


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's results for every stream of a batch, computed once and shared."""
    b = RS.batch(name)
    return [RO.analyze(b["fs"], b["speech"][s], b["noise_rms_db"][s], None if b["vad"] is None else b["vad"][s],
                       None if b["noise"] is None else b["noise"][s]) for s in range(b["speech"].shape[0])]


def compare_with_fixture(name, rows, per_frame, worst):
    """rows[s]: field -> value of stream s; per_frame(s, field) -> array.  Equal fields are asserted, the others fill `worst`."""
    fx = RS.fixture()
    counts, scalars = fx[f"{name}/counts"], fx[f"{name}/scalars"]
    for s, got in enumerate(rows):
        where = (name, s)
        if counts[s, 0] < 0:
            assert got["non_finite"] == 1, where
            continue
        assert got["non_finite"] == 0, where
        for j, field in enumerate(COUNTS):
            assert int(got[field]) == int(counts[s, j]), where + (field,)
        for j, field in enumerate(SCALARS):
            want = scalars[s, j]
            if np.isnan(want):  # a key the reference's dict does not have without evidence
                continue
            family = FAMILY[field]
            worst[family] = max(worst[family], abs(float(got[field]) - float(want)))
        if name.startswith("main_") and s in FRAME_STREAMS:
            assert np.array_equal(per_frame(s, "active_frame_mask").astype(bool), fx[f"{name}/{s}/active_frame_mask"]), where
            assert np.array_equal(per_frame(s, "frame_indices"), fx[f"{name}/{s}/frame_indices"]), where
            for field in ("frame_db", "frame_probabilities", "frame_feature_rows"):
                d = np.abs(per_frame(s, field) - fx[f"{name}/{s}/{field}"])
                worst[FAMILY[field]] = max(worst[FAMILY[field]], float(d.max()) if d.size else 0.0)


def numpy_polyphase(fs, x):
    """resample_poly's sum as a plain double loop over the restatement's own table: the oldest input first, no fused step."""
    g, table = RO.geometry(fs), RO.phase_table(fs)
    n = x.size
    y = np.zeros(RO.resampled_length(fs, n))
    for o in range(y.size):
        t = (o + g["rem"]) * g["down"]
        phase, xi = t % g["up"], t // g["up"]
        acc = np.float64(0.0)
        for m in range(g["taps"] - 1, -1, -1):
            if 0 <= xi - m < n:
                acc = acc + np.float64(x[xi - m]) * table[phase, m]
        y[o] = acc
    return y


@pytest.mark.parametrize("fs", RESAMPLED)
def test_restated_resampler_matches_scipys_recorded_output(fs):
    fx = RS.fixture()
    x = RS.resample_input(fs)
    assert RS.fingerprint(x)["sha256"] == str(fx[f"resample/{fs}/input_sha256"])
    want = fx[f"resample/{fs}/output"]
    got, mask, counts = RO.resample(fs, x)
    g = RO.geometry(fs)
    assert got.size == want.size == -(-x.size * g["up"] // g["down"]) == RO.resampled_length(fs, x.size)
    assert counts.size == -(-want.size // 960) and not mask.any() and not counts.any()  # no frame is active: the mask is 0
    worst = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
    print(f"{fs} Hz: largest |restatement - resample_poly| / peak = {worst:.3e}")
    assert worst <= 4 * MEASURED_RESAMPLE


@pytest.mark.parametrize("fs", RESAMPLED)
def test_restated_resampler_is_the_plain_polyphase_sum_bit_for_bit(fs):
    x = RS.resample_input(fs)
    got, _, _ = RO.resample(fs, x)
    want = numpy_polyphase(fs, x)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_resampled_mask_and_counts_follow_the_frame_flags():
    """A mask of ones over whole frames: bytes set where the resampled mask is >= 0.5, counted per chunk of 960."""
    fs = 44_100
    x = RS.batch("one_window")["speech"][0]
    F = RO.frames(fs, x.size)
    flags = np.zeros(F, dtype=np.uint8)
    flags[3:9] = 1
    _, mask, counts = RO.resample(fs, x, flags)
    sample_mask = np.zeros(x.size)
    sample_mask[3 * RS.hop(fs): 8 * RS.hop(fs) + RS.frame(fs)] = 1.0
    g, table = RO.geometry(fs), RO.phase_table(fs)
    want = numpy_polyphase(fs, sample_mask) >= 0.5
    assert np.array_equal(mask.astype(bool), want) and g["up"] == 160 and table.shape == (160, 21)
    assert counts.tolist() == [int(want[c * 960:(c + 1) * 960].sum()) for c in range(counts.size)] and counts.sum() > 6000


@pytest.mark.parametrize("name", list(RS.ANALYZED))
def test_restatement_matches_the_reference_fixture(name):
    rows = restated(name)
    worst = dict.fromkeys(MEASURED, 0.0)
    compare_with_fixture(name, rows, lambda s, field: rows[s][field], worst)
    print(f"{name}: largest |restatement - reference|:", {k: f"{v:.3e}" for k, v in worst.items()})
    for family, value in worst.items():
        assert value <= 4 * MEASURED[family], (name, family, value)


def test_the_fixture_rests_on_the_conditions_its_generator_asserted():
    fx = RS.fixture()
    assert float(fx["nearest_decision"]) > RS.MARGIN and float(fx["mask_margin"]) > RS.MARGIN and float(fx["window_margin"]) > RS.MARGIN
    assert float(fx["runner_up"]) > 1e-9 and float(fx["chain/nearest_decision"]) > RS.MARGIN
    assert list(fx["batches"]) == list(RS.ANALYZED)
    for name in RS.ANALYZED:
        assert RS.fingerprint(RS.batch(name)["speech"])["sha256"] == str(fx[f"{name}/speech_sha256"]), name


@pytest.mark.parametrize("fs", RS.RATES)
def test_geometry_is_the_references(fs):
    g = RO.geometry(fs)
    divisor = int(np.gcd(fs, 48_000))
    assert (g["frame"], g["hop"]) == (max(256, int(fs * 40 / 1000.0)), max(128, int(fs * 20 / 1000.0))) and g["frame"] == 2 * g["hop"]
    assert g["vad_window"] == int(np.ceil(fs * 512 / 16_000)) and (g["up"], g["down"]) == (48_000 // divisor, fs // divisor)
    freqs = np.fft.rfftfreq(g["frame"], 1.0 / fs)
    band = freqs[(freqs >= 5000.0) & (freqs <= min(9500.0, fs * 0.45))]
    assert np.array_equal(RO.sibilance_freqs(fs), band) and band.size == (89 if fs == 16_000 else 181)
    for n in (g["frame"] - 1, g["frame"], 3 * g["hop"] - 1, 3 * g["hop"], 170 * g["hop"] + 123):
        assert RO.frames(fs, n) == (0 if n < g["frame"] else (n - g["frame"]) // g["hop"] + 1)
        n48 = -(-n * g["up"] // g["down"])
        assert RO.resampled_length(fs, n) == n48 and RO.chunks(fs, n) == -(-n48 // 960)
    with pytest.raises(ValueError):
        RO.geometry(11_025)


@pytest.mark.parametrize("name", ("tail", "one_window", "no_vad", "special"))
def test_rate_taking_forms_give_the_48_khz_forms_bits(name):
    """Masks and loudness through sfm_masks_at / sfm_loudness_at at 48 kHz against sfm_masks / sfm_loudness, and the whole
    restatement at 48 kHz against tests/ref/speech_features_ref.c, on batches of the 48 kHz stimulus."""
    b = SS.batch(name)
    for s in range(b["speech"].shape[0]):
        vad = None if b["vad"] is None else b["vad"][s]
        old = SO.analyze(b["speech"][s], b["noise_rms_db"][s], vad, None if b["noise"] is None else b["noise"][s])
        new = RO.analyze(48_000, b["speech"][s], b["noise_rms_db"][s], vad, None if b["noise"] is None else b["noise"][s])
        assert old["non_finite"] == new["non_finite"]
        if old["non_finite"]:
            continue
        for field, value in old.items():
            other = new[field]
            if isinstance(value, np.ndarray) and value.dtype.kind == "f":
                assert np.array_equal(value.view(np.uint64), other.view(np.uint64)), (name, s, field)
            elif isinstance(value, np.ndarray):
                assert np.array_equal(value, other), (name, s, field)
            else:
                assert np.float64(value).view(np.uint64) == np.float64(other).view(np.uint64), (name, s, field)
        assert RO.forms_agree_at_48k(old["frame_power"], old["chunk_energy"], b["speech"].shape[1], b["noise_rms_db"][s], vad), (name, s)


def test_a_capture_below_one_frame_is_refused():
    with pytest.raises(ValueError):
        RO.analyze(44_100, np.zeros(1763, dtype=np.float32), -60.0)
