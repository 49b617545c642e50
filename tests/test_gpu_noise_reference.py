"""The room-noise reference kernels (csrc/af_noise_reference.hip) through the C ABI against tests/ref/noise_reference_ref.c,
which tests/test_noise_reference_ref.py holds to the reference's recorded outputs, at every sample rate of the stimuli: frames
of 512 (radix 2 only), 600, 630, 882 and 9600 samples (the LDS path above 64 KB), 67 streams at 3000 Hz (a tile edge).

Sample statistics, chunk sums, frame powers, PSD rows, band sums and both middles of every median are compared as bit patterns:
they only sum or select in a fixed order that the restatement repeats, on the same tables, and nothing is contracted.  dB
fields and scores are within 1e-12 (the host half takes every logarithm, so they are expected to be equal too).  Status, bit
masks and counts are equal.  Against the reference's recorded values the bound is 1e-12 plus four times what
tests/test_noise_reference_ref.py measured between restatement and reference.  Every test prints its largest difference before
it asserts."""
import functools

import numpy as np
import pytest

import noise_reference_oracle as NO
import noise_reference_stimulus as NS
from test_noise_reference_ref import MEASURED

pytestmark = pytest.mark.gpu

DB_TOL = 1e-12
BATCHES = [b["name"] for b in NS.batches()]
BIT_EQUAL = ("noise_chunk_sums", "noise_frame_power", "speech_frame_power", "noise_psd", "band_power", "explicit_middles",
             "in_capture_middles")
EQUAL = ("status", "conservative", "reasons", "guidance", "finite_samples", "clipped_samples", "zero_samples",
         "in_capture_noise_frame_count", "noise_frames", "speech_frames", "n_bands", "has_in_capture_spectrum")
CLOSE = NO.METRICS + ("quality_score",)
ARRAYS = NO.SPECTRA + ("frame_rms_db", "band_levels_db")


@pytest.fixture(scope="module")
def core():
    from mic_eq_mi import mic_eq_core

    return mic_eq_core


def arguments(b):
    return dict(noise_vad_probabilities=b["noise_vad"], speech_vad_probabilities=b["speech_vad"], capture_age_s=b["age"],
                metadata_mismatch=b["mismatch"])


@functools.lru_cache(maxsize=None)
def restated(name):
    """The restatement's results for every stream of a batch, computed once and shared."""
    b = NS.batch(name)
    return [NO.analyze(b["noise"][s], None if b["speech"] is None else b["speech"][s], b["fs"],
                       None if b["noise_vad"] is None else b["noise_vad"][s], None if b["speech_vad"] is None else b["speech_vad"][s],
                       b["age"][s], int(b["mismatch"][s])) for s in range(b["noise"].shape[0])]


@functools.lru_cache(maxsize=None)
def computed(name):
    """The library's results for a batch (host entry point, with what the kernels left), computed once and shared."""
    from mic_eq_mi import mic_eq_core

    b = NS.batch(name)
    nr = mic_eq_core.NoiseReference(b["fs"])
    try:
        return nr.analyze(b["noise"], b["speech"], internals=True, **arguments(b))
    finally:
        nr.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def difference(got, want, where):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, where
    assert np.array_equal(np.isnan(got), np.isnan(want)), where
    finite = np.isfinite(want)
    return float(np.max(np.abs(got[finite] - want[finite]))) if finite.any() else 0.0


@pytest.mark.parametrize("name", BATCHES)
def test_c_abi_matches_the_restatement(name):
    got, want_rows = computed(name), restated(name)
    worst = dict.fromkeys(CLOSE + ARRAYS, 0.0)
    for s, want in enumerate(want_rows):
        where = (name, s)
        for field in EQUAL:
            assert int(got[field][s]) == int(want[field]), where + (field,)
        for field in ("noise_sum_squares", "noise_peak"):  # the sample statistics
            assert bits(got[field][s]) == bits(want[field]), where + (field,)
        for field in BIT_EQUAL:
            assert got[field][s].shape == want[field].shape, where + (field,)
            assert np.array_equal(bits(got[field][s]), bits(want[field])), where + (field,)
        for field in CLOSE:
            worst[field] = max(worst[field], difference(got[field][s], want[field], where + (field,)))
        for field in ARRAYS:
            worst[field] = max(worst[field], difference(got[field][s], want[field], where + (field,)))
        assert np.array_equal(got["frequencies"], want["frequencies"]), where
    print(f"{name}: largest |GPU - restatement|:", {k: f"{v:.3e}" for k, v in worst.items() if v})
    for field, value in worst.items():
        assert value <= DB_TOL, (name, field, value)


@pytest.mark.parametrize("name", BATCHES)
def test_c_abi_matches_the_reference_fixture(name):
    fx, got = NS.fixture(), computed(name)
    B = got["status"].size
    assert np.array_equal(got["status"], fx[f"{name}/status"])
    assert np.array_equal(got["reasons"], fx[f"{name}/masks"][:, 0]) and np.array_equal(got["guidance"], fx[f"{name}/masks"][:, 1])
    assert np.array_equal(got["conservative"], fx[f"{name}/flags"][:, 1])
    assert np.array_equal(got["in_capture_noise_frame_count"], fx[f"{name}/flags"][:, 3])
    chk = NS.checkpoint_bins(got["frequencies"].size)
    worst = dict.fromkeys(MEASURED, 0.0)
    worst["quality_score"] = difference(got["quality_score"], fx[f"{name}/quality"], name)
    for j, field in enumerate(NO.METRICS):
        worst[field] = difference(got[field], fx[f"{name}/metrics"][:, j], (name, field))
    for j, field in enumerate(NO.SPECTRA):
        worst[field] = difference(got[field][:, chk], fx[f"{name}/checkpoints"][:, j], (name, field))
    if f"{name}/full_spectra" in fx:
        full = fx[f"{name}/full_spectra"]
        for field, want in (("explicit_spectrum_db", full[0]), ("in_capture_spectrum_db", full[1]),
                            ("conservative_spectrum_db", np.fmax(full[0], full[1]))):
            worst[field] = max(worst[field], difference(got[field][0], want, (name, field, "full")))
    print(f"{name}: {B} streams, largest |GPU - reference|:", {k: f"{v:.3e}" for k, v in worst.items() if v})
    for field, value in worst.items():
        assert value <= DB_TOL + 4 * MEASURED[field], (name, field, value)


@pytest.mark.parametrize("name", ("main@3150", "vad@4410", "sub_frame@3150"))
def test_host_and_device_entry_points_give_equal_bits(core, name):
    import torch

    b = NS.batch(name)
    noise, speech = b["noise"], b["speech"]
    host = computed(name)
    pad = 11  # strides above the lengths
    d_noise = torch.zeros((noise.shape[0], noise.shape[1] + pad), dtype=torch.float32, device="cuda")
    d_noise[:, : noise.shape[1]] = torch.from_numpy(noise).cuda()
    d_speech = torch.zeros((speech.shape[0], speech.shape[1] + pad), dtype=torch.float32, device="cuda")
    d_speech[:, : speech.shape[1]] = torch.from_numpy(speech).cuda()
    torch.cuda.synchronize()
    nr = core.NoiseReference(b["fs"])
    device = nr.analyze(None, None, internals=True, **arguments(b),
                        device_pointers=(d_noise.data_ptr(), noise.shape[1], noise.shape[0], d_noise.shape[1], d_speech.data_ptr(),
                                         speech.shape[1], d_speech.shape[1]))
    ms = nr.last_kernel_ms()
    nr.close()
    assert set(ms) == set(core.NOISE_REFERENCE_KERNELS) and all(v >= 0.0 for v in ms.values()) and sum(ms.values()) > 0.0
    for field, value in host.items():
        assert np.array_equal(value, device[field], equal_nan=True) if value.dtype.kind != "f" else np.array_equal(
            bits(value), bits(device[field])), field


def test_a_handle_gives_the_same_bits_again_after_another_batch(core):
    """Scratch is kept between calls and sized by the largest: a smaller batch after a larger one, and the first one again."""
    a, b = NS.batch("main@3000"), NS.batch("no_voice@3000")
    nr = core.NoiseReference(3000)
    first = nr.analyze(a["noise"], a["speech"], **arguments(a))
    other = nr.analyze(b["noise"], None, **arguments(b))
    again = nr.analyze(a["noise"], a["speech"], **arguments(a))
    nr.close()
    for field in NO.SPECTRA + ("quality_score", "status", "reasons"):
        assert np.array_equal(first[field], again[field], equal_nan=True), field
        assert np.array_equal(other[field], computed("no_voice@3000")[field], equal_nan=True), field


def test_python_operators_return_the_references_results():
    import mic_eq_mi

    fx = NS.fixture()
    for name in ("main@2560", "vad@3150", "sub_frame@3150", "no_voice@3000"):
        b = NS.batch(name)
        results = mic_eq_mi.analyze_noise_reference_batch(b["noise"], b["speech"], b["fs"], noise_metadata=[m[0] for m in b["metadata"]],
                                                          speech_metadata=[m[1] for m in b["metadata"]],
                                                          noise_vad_probabilities=b["noise_vad"], speech_vad_probabilities=b["speech_vad"])
        raw = computed(name)
        for s, r in enumerate(results):
            where = (name, s)
            assert isinstance(r, mic_eq_mi.NoiseReferenceAnalysis)
            assert r.status == NO.STATUS[fx[f"{name}/status"][s]] and r.usable == bool(fx[f"{name}/flags"][s, 0]), where
            assert r.conservative == bool(fx[f"{name}/flags"][s, 1]), where
            assert r.reasons == NO.texts(int(fx[f"{name}/masks"][s, 0]), NO.REASONS), where
            assert r.guidance == NO.texts(int(fx[f"{name}/masks"][s, 1]), NO.GUIDANCE), where
            assert r.metrics["identity_metadata_available"] == bool(fx[f"{name}/flags"][s, 2]), where
            assert r.metrics["in_capture_noise_frame_count"] == fx[f"{name}/flags"][s, 3], where
            for j, field in enumerate(NO.METRICS):  # None exactly where the reference has None; values the C ABI's
                want = fx[f"{name}/metrics"][s, j]
                assert (r.metrics[field] is None) == bool(np.isnan(want)), where + (field,)
                assert r.metrics[field] is None or r.metrics[field] == raw[field][s], where + (field,)
            assert (r.in_capture_spectrum_db is None) == bool(np.isnan(fx[f"{name}/checkpoints"][s, 2, 0])), where
            assert np.array_equal(r.explicit_spectrum_db, raw["explicit_spectrum_db"][s]) and r.quality_score == raw["quality_score"][s]
            assert r.conservative_noise_rms_db == r.metrics["conservative_noise_rms_db"]
            assert r.diagnostics()["status"] == r.status and r.frequencies.shape == r.conservative_spectrum_db.shape
    b = NS.batch("main@3150")
    s = 15  # maybe_stale: metadata with timestamps
    one = mic_eq_mi.analyze_noise_reference(b["noise"][s], b["speech"][s], b["fs"], noise_metadata=b["metadata"][s][0],
                                            speech_metadata=mic_eq_mi.CaptureMetadata.coerce(b["metadata"][s][1]))
    raw = computed("main@3150")
    assert one.reasons == ["room-noise reference may be stale"] and one.status == "questionable" and one.metrics["capture_age_s"] == 200.0
    assert np.array_equal(one.conservative_spectrum_db, raw["conservative_spectrum_db"][s])
