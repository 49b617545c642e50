"""The speech features at device rates (af_device_rate_features_*, `device_rate=True`) against
tests/ref/speech_features_rates_ref.c, which tests/test_speech_features_rates_ref.py holds to the reference's and scipy's
recorded outputs: the main batch at 16, 32, 44.1 and 96 kHz (67 streams of 170 hops + 123 samples: one past the 64-stream tile,
one short-term window, a partial tail chunk, a resampled length that is no multiple of 64 or 960), the small batches at
44.1 kHz (one frame, twelve hops, one momentary window, no posteriors, no noise, a noise capture below one frame, an all-zero
stream, a stream with a NaN), and the resampling stage alone at 22.05, 24 and 88.2 kHz.

The resampled signal, its mask bytes and their counts per chunk are compared as bit patterns: the kernel and the restatement
sum the same products of the same table in the same order, unfused.  So are frame powers, chunk energies, band sums, sibilance
middles and rows and the weighted sums.  Masks, counts, indices, both peak frequencies and the non-finite flag are equal; every
dB, loudness, feature and probability field is within 1e-12.  Against the reference's recorded values the bound is 1e-12 plus
four times what tests/test_speech_features_rates_ref.py measured.  Every test prints its largest difference before it asserts."""
import functools

import numpy as np
import pytest

import signals as S
import speech_features_oracle as SO
import speech_features_rates_oracle as RO
import speech_features_rates_stimulus as RS
import speech_features_stimulus as SS
from test_gpu_speech_features import BIT_EQUAL_FRAMES, BIT_EQUAL_LISTED, CLOSE, EQUAL, TOL, assert_same_results, bits
from test_speech_features_rates_ref import MEASURED, compare_with_fixture, restated

pytestmark = pytest.mark.gpu

BATCHES = list(RS.ANALYZED)


@pytest.fixture(scope="module")
def core():
    from mic_eq_mi import mic_eq_core

    return mic_eq_core


def handle(core, b, streams=None):
    return core.SpeechFeatures(b["fs"], streams or b["speech"].shape[0], b["speech"].shape[1], 0 if b["noise"] is None else b["noise"].shape[1],
                               device_rate=True)


@functools.lru_cache(maxsize=None)
def computed(name):
    """The library's results for a batch (host entry point, with what the kernels left), computed once and shared."""
    from mic_eq_mi import mic_eq_core

    b = RS.batch(name)
    sf = handle(mic_eq_core, b)
    try:
        return sf.analyze(b["speech"], b["noise_rms_db"], b["vad"], b["noise"], internals=True)
    finally:
        sf.close()


def restated_flags(name):
    """Frame flags [B, F] for the resampling stage alone: the restatement's active masks (zeros for a non-finite stream)."""
    return np.stack([r["active_frame_mask"] for r in restated(name)])


@pytest.mark.parametrize("name", BATCHES)
def test_resampling_stage_matches_the_restatement_bit_for_bit(core, name):
    b = RS.batch(name)
    finite = np.where(np.isfinite(b["speech"]), b["speech"], 0.0).astype(np.float32)  # the stage itself has no flag: a NaN stays out
    flags = restated_flags(name)
    sf = handle(core, b)
    signal, mask, counts = sf.resample(finite, flags)
    sf.close()
    n48 = RO.resampled_length(b["fs"], finite.shape[1])
    assert signal.shape == mask.shape == (finite.shape[0], n48) and counts.shape == (finite.shape[0], -(-n48 // 960))
    for s, want in enumerate(restated(name)):
        if want["non_finite"]:
            continue
        assert np.array_equal(bits(signal[s]), bits(want["resampled"])), (name, s)
        assert np.array_equal(mask[s], want["resampled_mask"]) and np.array_equal(counts[s], want["chunk_counts"]), (name, s)


@pytest.mark.parametrize("fs", RS.TAP_RATES)
def test_resampling_stage_alone_at_the_other_rates(core, fs):
    b = RS.batch(f"tap_{fs}")
    rows = [RO.analyze(fs, b["speech"][s], b["noise_rms_db"][s], b["vad"][s]) for s in range(b["speech"].shape[0])]
    sf = handle(core, b)
    signal, mask, counts = sf.resample(b["speech"], np.stack([r["active_frame_mask"] for r in rows]))
    sf.close()
    for s, want in enumerate(rows):
        assert want["active_frames"] > 0 and 0 < want["chunk_counts"].sum() < want["resampled"].size, (fs, s)
        assert np.array_equal(bits(signal[s]), bits(want["resampled"])), (fs, s)
        assert np.array_equal(mask[s], want["resampled_mask"]) and np.array_equal(counts[s], want["chunk_counts"]), (fs, s)


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


@pytest.mark.parametrize("name", ("short", "short_noise", "no_noise"))
def test_host_and_device_entry_points_give_equal_bits(core, name):
    import torch

    b = RS.batch(name)
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
    assert set(ms) == set(core.SPEECH_FEATURES_KERNELS) | {"resampling"} and all(v >= 0.0 for v in ms.values())
    assert ms["resampling"] > 0.0 and ms["k_weighting"] > 0.0
    assert_same_results(computed(name), device, name)


def test_a_handle_gives_the_same_bits_again_and_after_a_larger_batch(core):
    """Scratch is kept between calls and sized by the largest: the same batch twice, then a smaller one after it."""
    a, b = RS.batch("no_vad"), RS.batch("special")
    sf = core.SpeechFeatures(RS.SMALL_RATE, 8, a["speech"].shape[1], a["noise"].shape[1], device_rate=True)
    first = sf.analyze(a["speech"], a["noise_rms_db"], a["vad"], a["noise"], internals=True)
    again = sf.analyze(a["speech"], a["noise_rms_db"], a["vad"], a["noise"], internals=True)
    smaller = sf.analyze(b["speech"], b["noise_rms_db"], b["vad"], b["noise"], internals=True)
    sf.close()
    assert_same_results(first, again, "again")
    assert_same_results(first, computed("no_vad"), "fresh handle")
    assert_same_results(smaller, computed("special"), "smaller after larger")


@pytest.mark.parametrize("name, n_bytes", (("main_44100", 4 << 20), ("short", 1), ("main_96000", 3 << 20)))
def test_results_do_not_depend_on_the_scratch_bound(core, name, n_bytes):
    """The resampled captures pass through scratch a segment of whole chunks of every stream at a time, the K-weighting's filter
    states carried across: 7 chunks a segment for the 67 streams under 4 MB, 5 under 3 MB, one chunk under a bound below one."""
    b = RS.batch(name)
    sf = handle(core, b)
    sf.set_scratch_bytes(n_bytes)
    got = sf.analyze(b["speech"], b["noise_rms_db"], b["vad"], b["noise"], internals=True)
    signal, mask, counts = sf.resample(b["speech"], restated_flags(name))
    sf.close()
    assert_same_results(computed(name), got, name)
    for s in (0, b["speech"].shape[0] - 1):
        want = restated(name)[s]
        assert np.array_equal(bits(signal[s]), bits(want["resampled"])) and np.array_equal(mask[s], want["resampled_mask"]), (name, s)
        assert np.array_equal(counts[s], want["chunk_counts"]), (name, s)


def test_a_nan_marks_its_stream_and_leaves_the_neighbours_alone(core):
    b = RS.batch("special")
    s = b["kinds"].index("nan")
    got = computed("special")
    assert got["non_finite"].tolist() == [int(k == "nan") for k in b["kinds"]]
    clean = b["speech"].copy()
    clean[s] = np.where(np.isfinite(clean[s]), clean[s], 0.0)
    sf = handle(core, b)
    other = sf.analyze(clean, b["noise_rms_db"], b["vad"], b["noise"], internals=True)
    sf.close()
    assert other["non_finite"].tolist() == [0] * len(b["kinds"])
    keep = np.arange(len(b["kinds"])) != s
    for field, value in got.items():
        x, y = value[keep], other[field][keep]
        assert np.array_equal(bits(x), bits(y)) if x.dtype.kind == "f" else np.array_equal(x, y), field
    # a NaN behind the last whole frame (the twelve hops end 57 samples past it): no frame power sees it, the K-weighting does
    c = RS.batch("short")
    tail = c["speech"].copy()
    tail[1, -3] = np.nan
    sf = handle(core, c)
    third = sf.analyze(tail, c["noise_rms_db"], c["vad"], c["noise"], internals=True)
    sf.close()
    assert third["non_finite"].tolist() == [0, 1, 0]
    for field, value in computed("short").items():
        x, y = value[[0, 2]], third[field][[0, 2]]
        assert np.array_equal(bits(x), bits(y)) if x.dtype.kind == "f" else np.array_equal(x, y), field


def test_the_new_family_at_48_khz_gives_the_old_familys_bits(core):
    b = SS.batch("tail")
    m = b["noise"].shape[1]
    old = core.SpeechFeatures(48_000, 2, b["speech"].shape[1], m)
    new = core.SpeechFeatures(48_000, 2, b["speech"].shape[1], m, device_rate=True)
    want = old.analyze(b["speech"], b["noise_rms_db"], b["vad"], b["noise"], internals=True)
    got = new.analyze(b["speech"], b["noise_rms_db"], b["vad"], b["noise"], internals=True)
    ms = new.last_kernel_ms()
    assert (new.frames(2879), new.chunks(2879), new.resampled_length(2879), new.sibilance_bins) == (old.frames(2879), old.chunks(2879), 2879, 181)
    old.close()
    new.close()
    assert ms["resampling"] == 0.0 and ms["k_weighting"] > 0.0
    assert want["non_finite"].tolist() == [0, 0]
    assert_same_results(want, got, "48 kHz")


def test_python_operator_returns_the_references_dicts_at_44100():
    import mic_eq_mi

    b = RS.batch("special")
    results = mic_eq_mi.measure_speech_features_batch(b["speech"], b["fs"], b["noise_rms_db"], vad_probabilities=b["vad"],
                                                      noise_audio=b["noise"], device_rate=True)
    raw = computed("special")
    assert results[b["kinds"].index("nan")] is None
    for s, r in enumerate(results):
        if r is None:
            continue
        ev = r["deesser_frame_evidence"]
        assert r["momentary_lufs"] == raw["momentary_lufs"][s] and ev["peak_hz"] == raw["peak_hz"][s]
        assert ev["frame_feature_rows"].shape == (ev["frame_indices"].size, 6) and r["frame_db"].size == RO.frames(b["fs"], b["speech"].shape[1])


# ---- end to end at 44.1 kHz: recommend_voice_chain_batch(..., device_rate=True) against the reference's analyze_voice_setup
PROFILES = ("gentle", "balanced", "dense", "custom")


@pytest.fixture(scope="module")
def recommendations():
    import mic_eq_mi

    c = RS.chain_batch()
    return mic_eq_mi.recommend_voice_chain_batch(c["noise"], c["speech"], c["fs"], vad_probabilities=c["vad"],
                                                 noise_vad_probabilities=c["noise_vad"], device_rate=True)


def test_recommendations_at_44100_match_the_references_analyze_voice_setup(recommendations):
    """The bound is the 48 kHz one (tests/test_gpu_voice_chain_recommendation.py: 1e-12, four times the rules' measured
    difference, what the spectrum's inputs are allowed) plus four times what the features measured at device rates for the
    loudness and the levels, which enter the settings with slopes of at most 1."""
    from test_gpu_voice_chain_recommendation import ALLOWED, numbers_and_flags

    allowed = ALLOWED + 4 * (MEASURED["loudness"] + MEASURED["level_db"])
    fx = RS.fixture()
    c = RS.chain_batch()
    for key in ("speech", "vad", "noise", "noise_vad"):
        assert str(fx[f"chain/{key}_sha256"]) == RS.fingerprint(c[key])["sha256"], key
    assert len(recommendations) == RS.CHAIN_PAIRS
    worst, where = 0.0, None
    for i, rec in enumerate(recommendations):
        numbers, flags = numbers_and_flags(rec)
        assert [int(v) for v in flags] == fx["chain/flags"][i].tolist(), i
        assert rec["compressor"]["dynamics_intensity"] == PROFILES[int(fx["chain/profiles"][i])], i
        assert rec["noise_reference_status"] == str(fx["chain/status"][i]), i
        assert rec["gate"]["gate_mode"] == 1 and rec["features"]["vad_probability_used"]
        d = np.abs(np.array(numbers) - fx["chain/numbers"][i])
        print(f"pair {i}: |GPU - reference| per number:", [f"{v:.1e}" for v in d])
        if d.max() > worst:
            worst, where = float(d.max()), (i, int(d.argmax()))
    print(f"largest |GPU - reference| over the recommended settings at 44.1 kHz: {worst:.3e} at {where} (allowed {allowed:.3e})")
    assert worst <= allowed


def test_an_engine_at_44100_takes_the_recommended_settings_and_runs(recommendations, core):
    n_streams, n = 3, 22_050  # 0.5 s
    x = RS.chain_batch()["speech"][:n_streams, 40_000:40_000 + n]
    rec = recommendations[0]
    eng = core.Engine(48_000.0, n_streams)
    core.configure_auto_eq_chain(eng, 48_000.0, S.LIMITER_BANDS, S.limiter_settings(2.0))
    eng.set_io_sample_rates(44_100, 44_100)
    core.configure_voice_chain(eng, rec)
    got = eng.stream(x)
    eng.close()
    assert got.shape[0] == n_streams and got.shape[1] > n // 2 and np.all(np.isfinite(got))
