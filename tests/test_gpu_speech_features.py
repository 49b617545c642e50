"""The speech-feature kernels (csrc/af_speech_features.hip) through the C ABI against tests/ref/speech_features_ref.c, which
tests/test_speech_features_ref.py holds to the reference's recorded outputs, on every batch of the stimulus: 67 streams of 209
frames (a tile edge, two short-term windows) and the small batches (one frame, a partial tail chunk, one momentary window, no
short-term window, no posteriors, the energy mask kept, no noise capture, a noise capture below one frame, an all-zero stream,
a stream without an active frame, a stream with a NaN).

Frame powers, chunk energies, the band sums with the sibilance maximum, the sibilance middles and rows and the weighted sums
are compared as bit patterns: they only sum or select in a fixed order that the restatement repeats, on the same tables, and
nothing is contracted.  Masks, counts, indices, both peak frequencies and the non-finite flag are equal.  Every dB, loudness,
feature and probability field is within 1e-12 (the host half is one text on both sides, so they are expected to be equal).
Against the reference's recorded values the bound is 1e-12 plus four times what tests/test_speech_features_ref.py measured.
Every test prints its largest difference before it asserts."""
import functools

import numpy as np
import pytest

import speech_features_oracle as SO
import speech_features_stimulus as SS
from test_speech_features_ref import MEASURED, compare_with_fixture, restated

pytestmark = pytest.mark.gpu

TOL = 1e-12
BATCHES = list(SS.BATCHES)
BIT_EQUAL_FRAMES = ("frame_power", "chunk_energy")                                     # whole rows
BIT_EQUAL_LISTED = ("band_sums", "sibilance_middles", "sibilance_rows")               # the first spectral_frames rows
EQUAL = ("non_finite", "frames", "active_frames", "spectral_frames", "noise_frames", "vad_probability_used", "short_term_window_count",
         "loudness_window_count", "evidence_available")
CLOSE = tuple(name for name in SO.LEVELS if name != "peak_hz")


@pytest.fixture(scope="module")
def core():
    from mic_eq_mi import mic_eq_core

    return mic_eq_core


def handle(core, b):
    return core.SpeechFeatures(SS.FS, b["speech"].shape[0], b["speech"].shape[1], 0 if b["noise"] is None else b["noise"].shape[1])


@functools.lru_cache(maxsize=None)
def computed(name):
    """The library's results for a batch (host entry point, with what the kernels left), computed once and shared."""
    from mic_eq_mi import mic_eq_core

    b = SS.batch(name)
    sf = handle(mic_eq_core, b)
    try:
        return sf.analyze(b["speech"], b["noise_rms_db"], b["vad"], b["noise"], internals=True)
    finally:
        sf.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_results(a, b, what):
    """Every field of two result dicts: floats as bit patterns, the rest as values (non-finite streams carry nothing else)."""
    assert np.array_equal(a["non_finite"], b["non_finite"]), what
    keep = a["non_finite"] == 0
    for field, value in a.items():
        x, y = value[keep], b[field][keep]
        assert np.array_equal(bits(x), bits(y)) if x.dtype.kind == "f" else np.array_equal(x, y), (what, field)


@pytest.mark.parametrize("name", BATCHES)
def test_c_abi_matches_the_restatement(name):
    got, want_rows = computed(name), restated(name)
    worst = dict.fromkeys(CLOSE + ("frame_db", "frame_probabilities", "frame_feature_rows"), 0.0)
    for s, want in enumerate(want_rows):
        where = (name, s)
        assert int(got["non_finite"][s]) == int(want["non_finite"]), where
        if want["non_finite"]:
            continue
        A = want["spectral_frames"]
        for field in EQUAL:
            assert int(got[field][s]) == int(want[field]), where + (field,)
        assert got["peak_hz"][s] == want["peak_hz"], where
        for field in BIT_EQUAL_FRAMES:
            assert np.array_equal(bits(got[field][s]), bits(want[field])), where + (field,)
        for field in BIT_EQUAL_LISTED:
            assert np.array_equal(bits(got[field][s, :A]), bits(want[field])), where + (field,)
        assert np.array_equal(bits(got["noise_band_sums"][s]), bits(want["noise_band_sums"])), where
        assert np.array_equal(got["sibilance_argmax"][s, :A], want["sibilance_argmax"]), where
        assert np.array_equal(got["active_frame_mask"][s], want["active_frame_mask"]), where
        assert np.array_equal(got["frame_indices"][s, :A], want["frame_indices"]), where
        if A:
            assert np.array_equal(bits(got["weighted_sums"][s]), bits(want["weighted_sums"])), where
            assert int(got["weighted_argmax"][s]) == want["weighted_argmax"], where
        for field in CLOSE:
            worst[field] = max(worst[field], abs(float(got[field][s]) - float(want[field])))
        worst["frame_db"] = max(worst["frame_db"], float(np.max(np.abs(got["frame_db"][s] - want["frame_db"]))))
        for field in ("frame_probabilities", "frame_feature_rows"):
            if A:
                worst[field] = max(worst[field], float(np.max(np.abs(got[field][s, :A] - want[field]))))
    print(f"{name}: largest |GPU - restatement|:", {k: f"{v:.3e}" for k, v in worst.items() if v} or 0.0)
    for field, value in worst.items():
        assert value <= TOL, (name, field, value)


@pytest.mark.parametrize("name", BATCHES)
def test_c_abi_matches_the_reference_fixture(name):
    got = computed(name)
    rows = [{field: got[field][s] for field in EQUAL + SO.LEVELS} for s in range(got["frames"].size)]
    worst = dict.fromkeys(MEASURED, 0.0)

    def per_frame(s, field):
        A = int(got["spectral_frames"][s])
        return got[field][s] if field in ("frame_db", "active_frame_mask") else got[field][s, :A]

    compare_with_fixture(name, rows, per_frame, worst)
    print(f"{name}: largest |GPU - reference|:", {k: f"{v:.3e}" for k, v in worst.items()})
    for family, value in worst.items():
        assert value <= (TOL if MEASURED[family] else 0.0) + 4 * MEASURED[family], (name, family, value)


@pytest.mark.parametrize("name", ("no_short_term", "short_noise", "no_noise"))
def test_host_and_device_entry_points_give_equal_bits(core, name):
    import torch

    b = SS.batch(name)
    speech, noise = b["speech"], b["noise"]
    pad = 11  # strides above the lengths
    d_speech = torch.zeros((speech.shape[0], speech.shape[1] + pad), dtype=torch.float32, device="cuda")
    d_speech[:, : speech.shape[1]] = torch.from_numpy(speech).cuda()
    d_noise = None
    if noise is not None:
        d_noise = torch.zeros((noise.shape[0], noise.shape[1] + pad), dtype=torch.float32, device="cuda")
        d_noise[:, : noise.shape[1]] = torch.from_numpy(noise).cuda()
    torch.cuda.synchronize()
    sf = handle(core, b)
    device = sf.analyze(None, b["noise_rms_db"], b["vad"], None, internals=True,
                        device_pointers=(d_speech.data_ptr(), speech.shape[1], speech.shape[0], d_speech.shape[1],
                                         None if d_noise is None else d_noise.data_ptr(), 0 if noise is None else noise.shape[1],
                                         0 if d_noise is None else d_noise.shape[1]))
    ms = sf.last_kernel_ms()
    sf.close()
    assert set(ms) == set(core.SPEECH_FEATURES_KERNELS) and all(v >= 0.0 for v in ms.values()) and sum(ms.values()) > 0.0
    assert_same_results(computed(name), device, name)


def test_a_handle_gives_the_same_bits_again_and_after_a_larger_batch(core):
    """Scratch is kept between calls and sized by the largest: the same batch twice, then a smaller one after it."""
    a, b = SS.batch("no_short_term"), SS.batch("special")
    sf = core.SpeechFeatures(SS.FS, 8, a["speech"].shape[1], a["noise"].shape[1])
    first = sf.analyze(a["speech"], a["noise_rms_db"], a["vad"], a["noise"], internals=True)
    again = sf.analyze(a["speech"], a["noise_rms_db"], a["vad"], a["noise"], internals=True)
    smaller = sf.analyze(b["speech"], b["noise_rms_db"], b["vad"], b["noise"], internals=True)
    sf.close()
    assert_same_results(first, again, "again")
    assert_same_results(first, computed("no_short_term"), "fresh handle")
    assert_same_results(smaller, computed("special"), "smaller after larger")


def test_a_nan_marks_its_stream_and_leaves_the_neighbours_alone(core):
    b = SS.batch("special")
    s = b["kinds"].index("nan")
    got = computed("special")
    assert got["non_finite"].tolist() == [int(k == "nan") for k in b["kinds"]]
    clean = b["speech"].copy()
    clean[s] = np.where(np.isfinite(clean[s]), clean[s], 0.0)
    sf = handle(core, b)
    other = sf.analyze(clean, b["noise_rms_db"], b["vad"], b["noise"], internals=True)
    noisy = b["noise"].copy()
    noisy[0, 5000] = np.inf  # a non-finite sample of the room tone marks its stream too
    third = sf.analyze(b["speech"], b["noise_rms_db"], b["vad"], noisy)
    sf.close()
    assert other["non_finite"].tolist() == [0] * len(b["kinds"])
    keep = np.arange(len(b["kinds"])) != s
    for field, value in got.items():
        x, y = value[keep], other[field][keep]
        assert np.array_equal(bits(x), bits(y)) if x.dtype.kind == "f" else np.array_equal(x, y), field
    assert third["non_finite"].tolist() == [1] + [int(k == "nan") for k in b["kinds"][1:]]
    assert third["momentary_lufs"][4] == got["momentary_lufs"][4] and third["peak_hz"][4] == got["peak_hz"][4]


def test_frame_model_parameters_reach_the_probabilities(core):
    b = SS.batch("one_window")
    model = np.array([-3.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    sf = handle(core, b)
    intercept, w = sf.frame_model()
    assert intercept == -14.745480728063148 and w[1] == 5.220098953258285
    sf.set_frame_model(model[0], model[1:])
    got = sf.analyze(b["speech"], b["noise_rms_db"], b["vad"], b["noise"])
    sf.close()
    for s in range(b["speech"].shape[0]):
        want = SO.analyze(b["speech"][s], b["noise_rms_db"][s], b["vad"][s], b["noise"][s], model=model)
        A = want["spectral_frames"]
        assert np.max(np.abs(got["frame_probabilities"][s, :A] - want["frame_probabilities"])) <= TOL
        assert got["peak_hz"][s] == want["peak_hz"] and abs(got["frame_probability_p90"][s] - want["frame_probability_p90"]) <= TOL


def test_python_operator_returns_the_references_dicts():
    import mic_eq_mi

    fx = SS.fixture()
    b = SS.batch("special")
    results = mic_eq_mi.measure_speech_features_batch(b["speech"], SS.FS, b["noise_rms_db"], vad_probabilities=b["vad"], noise_audio=b["noise"])
    raw = computed("special")
    assert results[b["kinds"].index("nan")] is None
    keys = {"frame_db", "active_frame_mask", "active_duration_s", "active_ratio", "vad_probability_used", "vad_active_frame_ratio",
            "short_term_lufs", "short_term_window_count", "momentary_lufs", "active_loudness_spread_db", "loudness_range_db",
            "loudness_window_count", "band_energy_db", "sibilance_excess_db", "deesser_frame_evidence"}
    for s, r in enumerate(results):
        if r is None:
            continue
        assert set(r) == keys and set(r["band_energy_db"]) == {"low", "body", "presence", "sibilance"}
        ev = r["deesser_frame_evidence"]
        assert ev["available"] == bool(fx["special/counts"][s, 6]) and ("frame_probability_p90" in ev) == ev["available"]
        assert r["momentary_lufs"] == raw["momentary_lufs"][s] and ev["peak_hz"] == raw["peak_hz"][s]
        assert ev["frame_feature_rows"].shape == (ev["frame_indices"].size, 6) and r["active_frame_mask"].dtype == bool
    with pytest.raises(NotImplementedError, match="44100"):
        mic_eq_mi.measure_speech_features_batch(b["speech"], 44_100, b["noise_rms_db"])
