"""The reliability kernels (csrc/af_spectrum_stats.hip) through the C ABI against tests/ref/voice_reliability_ref.c, which
tests/test_voice_reliability_ref.py holds to the reference's recorded outputs.

Two comparisons per batch.  (a) Restatement end to end (voice_spectrum_ref.c then voice_reliability_ref.c): discrete fields
equal; dB fields within DB_TOL = 1e-12 (the smoothed rows the statistics start from differ by a device log10 / pow, at most 2.8e-14
dB, and medians, differences and means of them do not amplify that); fields in [0, 1] within 1e-12 (their maps from dB are
Lipschitz with a constant below 1: |d/du exp(-(u / 2.5)^2)| <= 0.35); effective blocks within 1e-12 x block count; the per-bin
SNR and snr_db within 1e-12 (1 + P / max(P - N, 1e-6 N)), the amplification of the formula itself, from the restatement's powers.
(b) The restatement fed the GPU's own smoothed rows: its inputs are then bit-equal, and what only selects or sums in its order
-- distances, the robust median, the uncertainty, the effective block count -- is compared as bit patterns.
Every test prints its largest differences before it asserts."""
import functools

import numpy as np
import pytest

import voice_reliability_oracle as VR
import voice_reliability_stimulus as RS
import voice_spectrum_oracle as VO
import voice_spectrum_stimulus as VS

pytestmark = pytest.mark.gpu

DB_TOL = 1e-12
UNIT_TOL = 1e-12
UNIT_FIELDS = ("residual_confidence", "measurement_coverage", "outlier_rejection_ratio", "phonetic_coverage")
# |GPU - reference| <= |GPU - restatement| + |restatement - reference|: the second from tests/test_voice_reliability_ref.py's MEASURED
FIXTURE_TOL = {"median_spectrum_db": DB_TOL + 4 * 2.984e-13, "spectral_repeatability": UNIT_TOL + 4 * 9.059e-14,
               "measurement_uncertainty_db": DB_TOL + 4 * 2.645e-13, "residual_confidence": UNIT_TOL + 4 * 1.332e-14,
               "measurement_coverage": UNIT_TOL + 4 * 2.776e-15, "phonetic_coverage": UNIT_TOL + 4 * 4.774e-15,
               "spectral_tilt_db_per_octave": DB_TOL + 4 * 1.954e-14}


@functools.lru_cache(maxsize=None)
def cases():
    return {c["name"]: c for c in RS.cases()}


@functools.lru_cache(maxsize=None)
def batch(name, nperseg=256, streams=None):
    if name == "main":
        return VS.main_batch(nperseg, streams or VS.MAIN_STREAMS), None, None
    case = cases()[name]
    return case["audio"], case.get("vad"), case.get("noise")


@functools.lru_cache(maxsize=None)
def restated(name, nperseg=256, streams=None):
    """Both restatements for every stream of a batch, computed once and shared: [(first half, second half)]."""
    audio, vad, noise = batch(name, nperseg, streams)
    out = []
    for s in range(audio.shape[0]):
        first = VO.analyze(audio[s], VS.FS, nperseg, None if vad is None else vad[s], None if noise is None else noise[s])
        out.append((first, VR.from_first_half(first, VS.FS, nperseg)))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b)) if np.asarray(a).dtype.kind == "f" else np.array_equal(a, b)


def difference(got, want, where):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), where
    finite = np.isfinite(want)
    return np.abs(got[finite] - want[finite]) if finite.any() else np.zeros(1)


def snr_allowance(median_db, noise_db):
    """Per bin 1e-12 (1 + P / max(P - N, 1e-6 N)), and the same from the sums over 80 Hz .. 8 kHz for snr_db."""
    P, Nz = np.power(10.0, median_db / 10.0), np.maximum(np.power(10.0, noise_db / 10.0), 1e-18)
    return DB_TOL * (1.0 + P / np.maximum(P - Nz, 1e-6 * Nz))


def compare(vs, first_got, got, want_rows, label, nperseg=256):
    """One batch against the restatement, stream by stream; `vs` still holds the call's windows."""
    worst = {}

    def note(field, diff, allowed):
        ratio = float(np.max(diff / allowed))
        worst[field] = max(worst.get(field, (0.0, 0.0)), (ratio, float(np.max(diff))))

    freqs = VO.freqs(VS.FS, nperseg)
    band = (freqs >= 80.0) & (freqs <= 8000.0)
    for s, (first, want) in enumerate(want_rows):
        where = (label, s)
        for name in VR.COUNTS:
            assert int(got[name][s]) == int(want[name]), where + (name,)
        assert np.array_equal(got["inlier_mask"][s], want["inlier_mask"]), where
        for name in ("median_spectrum_db", "measurement_uncertainty_db", "window_distance"):
            note(name, difference(got[name][s], want[name], where + (name,)), DB_TOL)
        note("spectral_tilt_db_per_octave", difference(got["spectral_tilt_db_per_octave"][s], want["spectral_tilt_db_per_octave"], where), DB_TOL)
        note("spectral_repeatability", difference(got["spectral_repeatability"][s], want["spectral_repeatability"], where), UNIT_TOL)
        for name in UNIT_FIELDS:
            note(name, difference(got[name][s], want[name], where + (name,)), UNIT_TOL)
        note("effective_measurement_blocks", difference(got["effective_measurement_blocks"][s], want["effective_measurement_blocks"], where),
             DB_TOL * max(1, want["blocks"]))
        assert np.array_equal(np.isnan(got["spectral_snr_db"][s]), np.isnan(want["spectral_snr_db"])), where
        if not np.isnan(want["spectral_snr_db"][0]):
            base = first["speech_db"] if first["used_single_spectrum_fallback"] else want["median_spectrum_db"]
            allow = snr_allowance(base, first["noise_db"])
            note("spectral_snr_db", np.abs(got["spectral_snr_db"][s] - want["spectral_snr_db"]), allow)
            P, Nz = np.power(10.0, want["median_spectrum_db"][band] / 10.0).sum(), np.power(10.0, first["noise_db"][band] / 10.0).sum()
            note("snr_db", np.abs(got["snr_db"][s] - want["snr_db"]), DB_TOL * (1.0 + P / max(P - Nz, 1e-6 * Nz)))
        else:
            assert got["snr_db"][s] == 0.0 == want["snr_db"], where
        if first["used_single_spectrum_fallback"]:
            assert got["measurement_coverage"][s] == 0.45 and np.isinf(got["measurement_uncertainty_db"][s]).all(), where
            assert not got["spectral_repeatability"][s].any() and got["residual_confidence"][s] == 0.0, where
            continue
        # (b) the restatement on the GPU's own smoothed rows
        smoothed = vs.windows(s)[1]
        mask = first_got["voiced_mask"][s].astype(bool)
        noise = None if np.isnan(first_got["noise_db"][s, 0]) else first_got["noise_db"][s]
        own = VR.analyze(smoothed, np.flatnonzero(mask) * (nperseg // 2), noise, VS.FS, nperseg)
        assert same(got["window_distance"][s][mask], own["window_distance"]), where + ("distances",)
        assert same(got["median_spectrum_db"][s], own["median_spectrum_db"]), where + ("robust median",)
        assert same(got["measurement_uncertainty_db"][s], own["measurement_uncertainty_db"]), where + ("uncertainty",)
        assert same(got["effective_measurement_blocks"][s], own["effective_measurement_blocks"]), where + ("effective blocks",)
        assert same(got["phonetic_coverage"][s], own["phonetic_coverage"]), where + ("levels behind the coverage",)
    print(f"{label}: largest |GPU - restatement| (share of the allowance, absolute):", {k: f"{r:.3f} {a:.3e}" for k, (r, a) in worst.items()})
    for field, (ratio, value) in worst.items():
        assert ratio <= 1.0, (label, field, value)


@pytest.fixture(scope="module")
def core():
    from mic_eq_mi import mic_eq_core

    return mic_eq_core


def run(core, name, nperseg=256, streams=None):
    audio, vad, noise = batch(name, nperseg, streams)
    vs = core.VoiceSpectrum(VS.FS, nperseg)
    first = vs.analyze(audio, vad, noise, keep_windows=True, reliability=True)
    return vs, first, vs.reliability()


def test_main_batch_of_67_streams(core):
    """Fallback and main-branch streams interleaved, a tile edge between streams 63 and 64, 0 to 27 % of the windows rejected."""
    vs, first, got = run(core, "main")
    want = restated("main")
    assert sum(f["used_single_spectrum_fallback"] for f, _ in want) >= 3 and any(r["inliers"] < r["voiced"] for _, r in want)
    assert want[63][0]["used_single_spectrum_fallback"] and not want[62][0]["used_single_spectrum_fallback"]  # the tile's last streams
    assert not any(f["used_single_spectrum_fallback"] for f, _ in want[64:])  # ... and the next tile's
    compare(vs, first, got, want, "main256")
    shares = vs.last_reliability_kernel_ms()  # two tiles: every kernel ran, and the five spans are part of the call's total
    assert all(v > 0.0 for v in shares.values()) and sum(shares.values()) < vs.last_kernel_ms()
    vs.analyze(batch("main")[0][:3])
    assert not any(vs.last_reliability_kernel_ms().values())  # the option off: nothing of it ran
    vs.close()


@pytest.mark.parametrize("name", ["short256_512", "closest256", "noise256", "vad256", "long256"])
def test_three_windows_noise_capture_vad_and_long_captures(core, name):
    vs, first, got = run(core, name)
    want = restated(name)
    if name in ("short256_512", "closest256"):  # three windows, one block: infinite uncertainty, zero reliability
        assert all(r["voiced"] == 3 and r["blocks"] == 1 and np.isinf(r["measurement_uncertainty_db"]).all() for _, r in want)
        assert want[0][1]["used_closest_windows"] == 1 and got["used_closest_windows"][0] == 1
    if name == "noise256":
        assert any(np.any(r["spectral_snr_db"] == -60.0) for _, r in want)
    if name == "long256":
        assert all(r["effective_measurement_blocks"] >= 12.0 for _, r in want)
    compare(vs, first, got, want, name)
    vs.close()


@pytest.mark.parametrize("nperseg,streams", [(4096, 5), (1024, 2), (8192, 2)])
def test_other_transform_sizes(core, nperseg, streams):
    """The voice band's bin range and the band tables at other sizes (1349 bins in LDS at 8192)."""
    vs, first, got = run(core, "main", nperseg, streams)
    compare(vs, first, got, restated("main", nperseg, streams), f"main{nperseg}", nperseg)
    vs.close()


def test_host_and_device_entry_points_give_equal_bits(core):
    import torch

    audio, _, noise = batch("noise256")
    vs = core.VoiceSpectrum(VS.FS, 256)
    vs.analyze(audio, None, noise, reliability=True)
    host = vs.reliability()
    d_audio = torch.zeros((audio.shape[0], audio.shape[1] + 11), dtype=torch.float32, device="cuda")  # a stride above the length
    d_audio[:, : audio.shape[1]] = torch.from_numpy(audio).cuda()
    d_noise = torch.from_numpy(noise).cuda().contiguous()
    torch.cuda.synchronize()
    vs.analyze(None, None, None, reliability=True, device_pointers=(d_audio.data_ptr(), audio.shape[1], audio.shape[0], d_audio.shape[1],
                                                                    d_noise.data_ptr(), noise.shape[1], noise.shape[1]))
    device = vs.reliability()
    for name, value in host.items():
        assert same(value, device[name]), name
    vs.close()


def test_scratch_regrows_runs_repeat_and_the_first_half_is_untouched(core):
    """One handle: a small batch, the large one (every buffer grows), the small one again, with bits equal between repeats;
    every field of the existing outputs equals the call with the option off; keep_windows does not change the statistics;
    a call with the option off leaves nothing to read."""
    big, small = batch("main")[0], batch("main")[0][:3]
    vs = core.VoiceSpectrum(VS.FS, 256)
    off_small = vs.analyze(small)
    with pytest.raises(RuntimeError):
        vs.reliability()
    on_small = vs.analyze(small, reliability=True)
    rel_small = vs.reliability()
    on_big = vs.analyze(big, reliability=True)
    rel_big = vs.reliability()
    again_small = vs.analyze(small, reliability=True, keep_windows=True)
    rel_again_small = vs.reliability()
    again_big = vs.analyze(big, keep_windows=True, reliability=True)
    rel_again_big = vs.reliability()
    off_big = vs.analyze(big)
    with pytest.raises(RuntimeError):
        vs.reliability()
    for a, b in ((off_small, on_small), (on_small, again_small), (off_big, on_big), (on_big, again_big), (rel_small, rel_again_small),
                 (rel_big, rel_again_big)):
        assert a.keys() == b.keys()
        for name, value in a.items():
            assert same(value, b[name]), name
    for s in range(3):  # a stream's statistics do not depend on the batch around it
        for name, value in rel_small.items():
            assert same(value[s], rel_big[name][s]), (s, name)
    vs.close()


def test_python_operator_against_the_reference_fixture():
    import mic_eq_mi

    audio = batch("main256")[0]
    fx = RS.fixture_case("main256")
    results = mic_eq_mi.analyze_voice_spectrum_batch(audio, VS.FS, 256)
    assert len(results) == 67
    chk, full = VS.checkpoint_bins(129), list(fx["full_streams"])
    worst = dict.fromkeys(FIXTURE_TOL, 0.0)
    for s, r in enumerate(results):
        assert isinstance(r, mic_eq_mi.VoiceSpectrumResult)
        assert r.used_single_spectrum_fallback == bool(fx["flags"][s, 0]), s
        assert r.noise_reference_source == VO.NOISE_SOURCES[int(fx["flags"][s, 1])], s
        assert (r.spectral_snr_db is None) == (r.noise_spectrum_db is None) == bool(np.isnan(fx["checkpoints"][s, 3, 0])), s
        assert r.window_spectra_db.shape == ((1, 129) if r.used_single_spectrum_fallback else (int(fx["counts"][s, 0]), 129)), s
        assert r.outlier_rejection_ratio == fx["scalars"][s, RS.SCALARS.index("outlier_rejection_ratio")], s
        for j, name in enumerate(RS.SPECTRA[:3]):
            worst[name] = max(worst[name], float(np.max(difference(getattr(r, name)[chk], fx["checkpoints"][s, j], (s, name)))))
            if s in full:
                worst[name] = max(worst[name], float(np.max(difference(getattr(r, name), fx["full_spectra"][full.index(s), j], (s, name)))))
        for name in ("residual_confidence", "measurement_coverage", "phonetic_coverage", "spectral_tilt_db_per_octave"):
            worst[name] = max(worst[name], abs(getattr(r, name) - fx["scalars"][s, RS.SCALARS.index(name)]))
        blocks = max(1, int(fx["counts"][s, 2]))
        assert abs(r.effective_measurement_blocks - fx["scalars"][s, 6]) <= (DB_TOL + 4 * 6.928e-14) * blocks, s
    print("analyze_voice_spectrum_batch: largest |GPU - reference|:", {k: f"{v:.3e} (allowed {FIXTURE_TOL[k]:.3e})" for k, v in worst.items()})
    for name, value in worst.items():
        assert value <= FIXTURE_TOL[name], (name, value)
