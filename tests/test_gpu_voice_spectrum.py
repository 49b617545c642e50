"""The voice spectrum kernels (csrc/af_spectrum.hip) through the C ABI against tests/ref/voice_spectrum_ref.c, which
tests/test_voice_spectrum_ref.py holds to the reference's recorded outputs.

Linear quantities (frame energies, the Welch sums over segments, the PSD of every voiced window) are compared as bit patterns:
the restatement performs the kernels' operations in the kernels' order on the same tables, and nothing is contracted.  dB
fields are within 1e-12 dB (device log10 is within 2 ulp of glibc's, and an ulp at |dB| <= 120 is 1.4e-14; medians only
select).  Discrete fields are equal.  Every test prints its largest difference before it asserts."""
import functools

import numpy as np
import pytest

import voice_spectrum_oracle as VO
import voice_spectrum_stimulus as VS

pytestmark = pytest.mark.gpu

DB_TOL = 1e-12
SPECTRA = ("speech_db", "noise_db", "spectral_snr_db", "welch_db")
DISCRETE = ("frames", "voiced", "vad_probability_used", "noise_reference_source", "used_single_spectrum_fallback", "welch_segments")
# |GPU - reference| <= |GPU - restatement| + |restatement - reference|: DB_TOL plus four times the largest Welch difference
# tests/test_voice_spectrum_ref.py measured between restatement and reference (MEASURED_DB["welch_db"])
FIXTURE_WELCH_TOL = DB_TOL + 4 * 1.421e-13


@functools.lru_cache(maxsize=None)
def cases():
    return {c["name"]: c for c in VS.cases()}


@functools.lru_cache(maxsize=None)
def main_batch(nperseg, streams=VS.MAIN_STREAMS):
    return VS.main_batch(nperseg, streams)


@functools.lru_cache(maxsize=None)
def restated(name, nperseg, streams=None):
    """The restatement's results for every stream of a batch, computed once and shared."""
    if name.startswith("main"):
        audio, vad, noise = main_batch(nperseg, streams or VS.MAIN_STREAMS), None, None
    else:
        case = cases()[name]
        audio, vad, noise = case["audio"], case.get("vad"), case.get("noise")
    return [VO.analyze(audio[s], VS.FS, nperseg, None if vad is None else vad[s], None if noise is None else noise[s])
            for s in range(audio.shape[0])]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def db_difference(got, want, what):
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    return 0.0 if np.isnan(want).all() else float(np.nanmax(np.abs(got - want)))


def compare(got, want_rows, label, vs=None, window_streams=()):
    """One batch result against the restatement, stream by stream.  Returns the largest dB difference per field."""
    worst = dict.fromkeys(SPECTRA + ("frame_rms_db", "window_db", "window_smoothed_db"), 0.0)
    for s, want in enumerate(want_rows):
        where = (label, s)
        for name in DISCRETE:
            assert int(got[name][s]) == int(want[name]), where + (name,)
        assert got["voiced_window_ratio"][s] == want["voiced_window_ratio"], where
        assert got["vad_active_window_ratio"][s] == want["vad_active_window_ratio"], where
        assert np.array_equal(got["voiced_mask"][s], want["voiced_mask"]), where
        assert np.array_equal(bits(got["frame_power"][s]), bits(want["frame_power"])), where + ("frame energies",)
        assert np.array_equal(bits(got["welch_sum"][s]), bits(want["welch_sum"])), where + ("Welch sums",)
        worst["frame_rms_db"] = max(worst["frame_rms_db"], db_difference(got["frame_rms_db"][s], want["frame_rms_db"], where))
        for name in SPECTRA:
            worst[name] = max(worst[name], db_difference(got[name][s], want[name], where + (name,)))
    for s in window_streams:
        raw, smoothed, linear = vs.windows(s)
        want = want_rows[s]
        assert raw.shape == want["win_db"].shape, (label, s)
        assert np.array_equal(bits(linear), bits(want["win_linear"])), (label, s, "linear PSD rows")
        if raw.size:
            worst["window_db"] = max(worst["window_db"], float(np.max(np.abs(raw - want["win_db"]))))
            worst["window_smoothed_db"] = max(worst["window_smoothed_db"], float(np.max(np.abs(smoothed - want["win_smooth"]))))
    print(f"{label}: largest |GPU - restatement| in dB:", {k: f"{v:.3e}" for k, v in worst.items()})
    for field, value in worst.items():
        assert value <= DB_TOL, (label, field, value)
    return worst


@pytest.fixture(scope="module")
def core():
    from mic_eq_mi import mic_eq_core

    return mic_eq_core


@pytest.mark.parametrize("nperseg", [256, 512])
def test_main_batch_of_67_streams(core, nperseg):
    """More than one wave of chunks, an odd stream count, and a tile edge between streams 63 and 64."""
    vs = core.VoiceSpectrum(VS.FS, nperseg)
    got = vs.analyze(main_batch(nperseg), keep_windows=True)
    want = restated("main", nperseg)
    assert sum(r["used_single_spectrum_fallback"] for r in want) >= 3 and {r["noise_reference_source"] for r in want} == {0, 2}
    compare(got, want, f"main{nperseg}", vs, window_streams=(0, 33, 63, 64, 66))
    assert vs.last_kernel_ms() > 0.0
    vs.close()


def test_five_streams_at_4096(core):
    vs = core.VoiceSpectrum(VS.FS, 4096)
    got = vs.analyze(main_batch(4096, 5), keep_windows=True)
    compare(got, restated("main", 4096, 5), "main4096", vs, window_streams=(0, 2, 4))
    vs.close()


@pytest.mark.parametrize("index", [0, 1, 2])
def test_one_frame_and_three_frame_lengths(core, index):
    n = VS.SHORT_LENGTHS(256)[index]
    vs = core.VoiceSpectrum(VS.FS, 256)
    got = vs.analyze(VS.short_batch(256, n), keep_windows=True)
    assert int(got["frames"][0]) == (1, 1, 3)[index]
    compare(got, restated(f"short256_{n}", 256), f"short256_{n}", vs, window_streams=(0, 1))
    vs.close()


@pytest.mark.parametrize("name", ["noise256", "shortnoise256", "vad256"])
def test_explicit_noise_capture_and_vad_posteriors(core, name):
    case = cases()[name]
    vs = core.VoiceSpectrum(VS.FS, 256)
    got = vs.analyze(case["audio"], case.get("vad"), case.get("noise"), keep_windows=True)
    want = restated(name, 256)
    if name == "noise256":
        assert all(r["noise_reference_source"] == 1 for r in want)
    if name == "vad256":
        assert all(r["vad_probability_used"] for r in want)
    compare(got, want, name, vs, window_streams=range(len(want)))
    vs.close()


def test_host_and_device_entry_points_give_equal_bits(core):
    import torch

    case = cases()["noise256"]
    audio, noise = case["audio"], case["noise"]
    vs = core.VoiceSpectrum(VS.FS, 256)
    host = vs.analyze(audio, None, noise)
    pad = 11  # a stride above the length
    d_audio = torch.zeros((audio.shape[0], audio.shape[1] + pad), dtype=torch.float32, device="cuda")
    d_audio[:, : audio.shape[1]] = torch.from_numpy(audio).cuda()
    d_noise = torch.from_numpy(noise).cuda().contiguous()
    torch.cuda.synchronize()
    device = vs.analyze(None, None, None, device_pointers=(d_audio.data_ptr(), audio.shape[1], audio.shape[0], d_audio.shape[1],
                                                           d_noise.data_ptr(), noise.shape[1], noise.shape[1]))
    for name, value in host.items():
        assert np.array_equal(value, device[name], equal_nan=True) if value.dtype.kind != "f" else np.array_equal(
            bits(value), bits(device[name])), name
    vs.close()


def test_scratch_regrows_and_runs_repeat_bit_for_bit(core):
    """One handle: a small batch, the large one (every buffer grows), the small one again; then the large one twice."""
    vs = core.VoiceSpectrum(VS.FS, 256)
    big, small = main_batch(256), main_batch(256)[:3]
    first_small = vs.analyze(small, keep_windows=True)
    compare(first_small, restated("main", 256)[:3], "small", vs, window_streams=(0, 2))
    first_big = vs.analyze(big, keep_windows=True)
    windows = [vs.windows(s) for s in (0, 40, 66)]
    compare(first_big, restated("main", 256), "big after small", vs, window_streams=(66,))
    again_small = vs.analyze(small)
    again_big = vs.analyze(big, keep_windows=True)
    for first, again in ((first_small, again_small), (first_big, again_big)):
        for name, value in first.items():
            same = np.array_equal(bits(value), bits(again[name])) if value.dtype.kind == "f" else np.array_equal(value, again[name])
            assert same, name
    for s, kept in zip((0, 40, 66), windows):
        for a, b in zip(kept, vs.windows(s)):
            assert np.array_equal(bits(a), bits(b)), s
    with pytest.raises(RuntimeError):  # a call that kept nothing leaves nothing to read
        vs.analyze(small)
        vs.windows(0)
    vs.close()


def test_python_operators_against_the_reference_fixture():
    import mic_eq_mi

    case = cases()["main256"]
    fx = VS.fixture_case(case)
    full = list(fx["full_streams"])
    worst = 0.0
    for i, s in enumerate(full):
        freqs, spectrum = mic_eq_mi.compute_voice_spectrum(case["audio"][s], VS.FS, 256)
        assert np.array_equal(freqs, VS.fixture()["freqs256"])
        worst = max(worst, float(np.max(np.abs(spectrum - fx["full_spectra"][i, 3]))))
    freqs, spectra = mic_eq_mi.compute_voice_spectrum_batch(case["audio"], VS.FS, 256)
    chk = VS.checkpoint_bins(129)
    worst = max(worst, float(np.max(np.abs(spectra[:, chk] - fx["checkpoints"][:, 3]))))
    print(f"compute_voice_spectrum: largest |GPU - reference| {worst:.3e} dB (allowed {FIXTURE_WELCH_TOL:.3e})")
    assert worst <= FIXTURE_WELCH_TOL
    results = mic_eq_mi.measure_voice_spectra(case["audio"], VS.FS, 256, return_windows=True)
    assert len(results) == 67
    for s, r in enumerate(results):
        want = fx["scalars"][s]
        assert r["used_single_spectrum_fallback"] == bool(want[6]) and r["voiced_window_ratio"] == want[2], s
        assert r["noise_reference_source"] == VO.NOISE_SOURCES[int(want[5])] and r["vad_probability_used"] is False, s
        assert np.array_equal(r["voiced_mask"], fx["voiced_mask"][s].astype(bool)), s
        assert (r["noise_spectrum_db"] is None) == bool(np.isnan(fx["checkpoints"][s, 1, 0])), s
        if r["used_single_spectrum_fallback"]:
            assert r["window_spectra_db"].shape == (1, 129) and r["measurement_coverage"] == 0.45 and r["residual_confidence"] == 0.0
            assert np.all(np.isinf(r["measurement_uncertainty_db"])) and not r["spectral_repeatability"].any()
            assert np.array_equal(r["median_spectrum_db"], r["welch_spectrum_db"])
        else:
            assert r["window_spectra_db"].shape == (int(want[1]), 129) == r["smoothed_window_spectra_db"].shape
