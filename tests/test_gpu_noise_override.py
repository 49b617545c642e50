"""The noise-spectrum override of analyze_voice_spectrum (spectrum.py:554-569, 596-602) on the device path, at nperseg 256.

The expected noise reference is np.interp of the override onto the handle's grid, computed here; the per-bin SNR of the first
half is spectrum.py:333-342 written out below; both are put into the restatement's first-half result, from which
tests/voice_reliability_oracle.py restates the second half (it takes the noise reference as an argument).  Comparisons and
tolerances are those of tests/test_gpu_voice_reliability.py (its `compare`).  analyze_voice_capture_batch is held to what the
reference's own analyze_noise_reference and analyze_voice_spectrum returned for six capture pairs
(tests/golden/noise_reference.npz)."""
import functools

import numpy as np
import pytest

import noise_reference_oracle as NO
import noise_reference_stimulus as NS
import voice_reliability_oracle as VR
import voice_spectrum_oracle as VO
import voice_spectrum_stimulus as VS
from test_gpu_voice_reliability import DB_TOL, compare, same, snr_allowance
from test_noise_reference_ref import MEASURED

pytestmark = pytest.mark.gpu

NPERSEG = 256
OVERRIDE = 3  # AF_NOISE_REFERENCE_VALIDATED_CONSERVATIVE


@pytest.fixture(scope="module")
def core():
    from mic_eq_mi import mic_eq_core

    return mic_eq_core


def override_grid():
    """The grid of a 48 kHz noise reference analysis: 4801 points, 5 Hz apart -- not the handle's."""
    return np.fft.rfftfreq(9600, 1.0 / VS.FS)


def override_rows(streams: int) -> np.ndarray:
    """A smooth, stream-dependent noise spectrum around -75 dB with a ripple finer than the handle's 187.5 Hz bins."""
    f = override_grid()
    s = np.arange(streams)[:, None]
    return -75.0 - 6.0 * np.log2(1.0 + f / 1000.0) + 2.0 * np.sin(f / 310.0 + s) + 0.5 * s


def spectral_snr(speech_db, noise_db):
    """_spectral_snr_db, spectrum.py:333-342."""
    total = np.power(10.0, speech_db / 10.0)
    noise = np.maximum(np.power(10.0, noise_db / 10.0), 1e-18)
    return 10.0 * np.log10(np.maximum(total - noise, noise * 1e-6) / noise)


@functools.lru_cache(maxsize=None)
def stimulus(name):
    if name == "main":
        return VS.main_batch(NPERSEG, 16), None  # streams 7 and 15 take the single-spectrum fallback
    case = {c["name"]: c for c in VS.cases()}[name]
    return case["audio"], case.get("noise")


@functools.lru_cache(maxsize=None)
def first_halves(name, with_noise):
    audio, noise = stimulus(name)
    return [VO.analyze(audio[s], VS.FS, NPERSEG, None, noise[s] if with_noise and noise is not None else None) for s in range(audio.shape[0])]


def expected(name, rows, valid):
    """[(first half, second half)] per stream: the override where `valid`, the call without one elsewhere."""
    freqs = VO.freqs(VS.FS, NPERSEG)
    out = []
    for s, (with_noise, without) in enumerate(zip(first_halves(name, True), first_halves(name, False))):
        if not valid[s]:
            out.append((with_noise, VR.from_first_half(with_noise, VS.FS, NPERSEG)))
            continue
        first = dict(without, noise_reference_source=OVERRIDE)
        if first["voiced"] > 0:
            first["noise_db"] = np.interp(freqs, override_grid(), rows[s], left=float(rows[s][0]), right=float(rows[s][-1]))
            first["spectral_snr_db"] = spectral_snr(first["speech_db"], first["noise_db"])
        out.append((first, VR.from_first_half(first, VS.FS, NPERSEG)))
    return out


def check_first_half(got, want_rows, label):
    worst = 0.0
    for s, (first, _) in enumerate(want_rows):
        where = (label, s)
        assert int(got["noise_reference_source"][s]) == int(first["noise_reference_source"]), where
        assert int(got["used_single_spectrum_fallback"][s]) == int(first["used_single_spectrum_fallback"]), where
        assert np.array_equal(np.isnan(got["noise_db"][s]), np.isnan(first["noise_db"])), where
        if not np.isnan(first["noise_db"][0]):
            worst = max(worst, float(np.max(np.abs(got["noise_db"][s] - first["noise_db"]))))
            allow = snr_allowance(first["speech_db"], first["noise_db"])
            assert np.all(np.abs(got["spectral_snr_db"][s] - first["spectral_snr_db"]) <= allow), where
    print(f"{label}: largest |GPU - np.interp| of the noise reference: {worst:.3e} dB")
    assert worst <= DB_TOL, (label, worst)


def run(core, name, override, with_noise=True):
    audio, noise = stimulus(name)
    vs = core.VoiceSpectrum(VS.FS, NPERSEG)
    first = vs.analyze(audio, None, noise if with_noise else None, keep_windows=True, reliability=True, noise_override=override)
    return vs, first, vs.reliability()


def test_override_takes_precedence_over_noise_audio(core):
    audio, noise = stimulus("noise256")
    assert noise is not None
    rows = override_rows(audio.shape[0])
    vs, first, got = run(core, "noise256", (override_grid(), rows))
    want = expected("noise256", rows, [True] * audio.shape[0])
    assert all(int(v) == OVERRIDE for v in first["noise_reference_source"])
    check_first_half(first, want, "override over noise_audio")
    compare(vs, first, got, want, "override over noise_audio")
    vs.close()


def test_invalid_override_falls_through_per_stream(core):
    audio, _ = stimulus("noise256")
    B = audio.shape[0]
    rows = override_rows(B)
    rows[1, 2000] = np.nan  # stream 1 alone: back to its room-noise capture
    valid = [s != 1 for s in range(B)]
    vs, first, got = run(core, "noise256", (override_grid(), rows))
    assert [int(v) for v in first["noise_reference_source"]] == [OVERRIDE if v else 1 for v in valid]
    want = expected("noise256", rows, valid)
    check_first_half(first, want, "one invalid stream")
    compare(vs, first, got, want, "one invalid stream")
    plain_first = vs.analyze(audio, None, stimulus("noise256")[1], keep_windows=True, reliability=True)
    plain = vs.reliability()
    for field in ("noise_db", "spectral_snr_db"):
        assert same(first[field][1], plain_first[field][1]), field
    for field in ("median_spectrum_db", "spectral_snr_db", "snr_db", "residual_confidence"):
        assert same(got[field][1], plain[field][1]), field
    # a single point, or a non-finite frequency, is no override for any stream: every bit of the call without one
    for bad in ((override_grid()[:1], rows[0, :1]), (np.where(np.arange(4801) == 7, np.inf, override_grid()), rows[0])):
        bad_first = vs.analyze(audio, None, stimulus("noise256")[1], keep_windows=True, reliability=True, noise_override=bad)
        bad_rel = vs.reliability()
        for field, value in plain_first.items():
            assert same(value, bad_first[field]), field
        for field, value in plain.items():
            assert same(value, bad_rel[field]), field
    vs.close()


def test_shared_and_per_stream_forms_agree(core):
    audio, _ = stimulus("noise256")
    row = override_rows(1)[0]
    vs, shared_first, shared = run(core, "noise256", (override_grid(), row))
    tiled_first = vs.analyze(audio, None, stimulus("noise256")[1], keep_windows=True, reliability=True,
                             noise_override=(override_grid(), np.tile(row, (audio.shape[0], 1))))
    tiled = vs.reliability()
    for field, value in shared_first.items():
        assert same(value, tiled_first[field]), field
    for field, value in shared.items():
        assert same(value, tiled[field]), field
    assert all(int(v) == OVERRIDE for v in shared_first["noise_reference_source"])
    with pytest.raises(ValueError, match="streams"):  # a per-stream override for another stream count
        vs.analyze(audio, None, None, noise_override=(override_grid(), np.tile(row, (audio.shape[0] + 1, 1))))
    vs.close()


def test_fallback_branch_and_streams_without_voiced_frames(core):
    audio, _ = stimulus("main")
    rows = np.tile(override_rows(1)[0], (audio.shape[0], 1))
    vs, first, got = run(core, "main", (override_grid(), rows[0]), with_noise=False)
    want = expected("main", rows, [True] * audio.shape[0])
    assert sum(int(f["used_single_spectrum_fallback"]) for f, _ in want) >= 2
    check_first_half(first, want, "fallback branch")
    compare(vs, first, got, want, "fallback branch")
    vs.close()


def test_a_handle_gives_its_earlier_bits_back(core):
    audio, noise = stimulus("noise256")
    override = (override_grid(), override_rows(audio.shape[0]))
    vs = core.VoiceSpectrum(VS.FS, NPERSEG)
    runs = []
    for o in (None, override, None, override):
        first = vs.analyze(audio, None, noise, keep_windows=True, reliability=True, noise_override=o)
        runs.append((first, vs.reliability()))
    fresh = core.VoiceSpectrum(VS.FS, NPERSEG)  # a handle that never saw an override
    plain_first = fresh.analyze(audio, None, noise, keep_windows=True, reliability=True)
    plain = fresh.reliability()
    fresh.close()
    vs.close()
    for (a_first, a), (b_first, b) in ((runs[0], runs[2]), (runs[1], runs[3]), (runs[0], (plain_first, plain))):
        for field, value in a_first.items():
            assert same(value, b_first[field]), field
        for field, value in a.items():
            assert same(value, b[field]), field
    assert not same(runs[0][0]["noise_db"], runs[1][0]["noise_db"])


def test_voice_capture_batch_against_the_reference(core):
    """voice_setup.py:1122-1162 back to back for the six pairs the reference's two functions were run on.  Bounds: the noise
    reference is an interpolation of the conservative spectrum (a convex combination: its error is not amplified); the SNR
    fields are f(P, N) = 10 log10((P - N) / N) of the robust median and that noise reference, whose errors (1e-12 each for
    the device path plus four times what the restatements measured against the reference) the formula amplifies by at most
    1 + P / (P - N) = 2 + 10^(-snr / 10)."""
    import mic_eq_mi

    fx = NS.fixture()
    b = NS.batch("main@3000")
    streams = [int(s) for s in fx["override/streams"]]
    references, spectra = mic_eq_mi.analyze_voice_capture_batch(
        b["noise"][streams], b["speech"][streams], b["fs"], NPERSEG, noise_metadata=[b["metadata"][s][0] for s in streams],
        speech_metadata=[b["metadata"][s][1] for s in streams])
    chk = NS.checkpoint_bins(NPERSEG // 2 + 1)
    noise_tol = DB_TOL + 4 * MEASURED["conservative_spectrum_db"]
    input_tol = noise_tol + DB_TOL + 4 * 2.984e-13  # + the robust median's (tests/test_voice_reliability_ref.py MEASURED)
    worst = {"noise_spectrum_db": 0.0, "spectral_snr_db": 0.0, "snr_db": 0.0}
    for i, s in enumerate(streams):
        r, v = references[i], spectra[i]
        assert r.status == NO.STATUS[fx["main@3000/status"][s]] and r.reasons == NO.texts(int(fx["main@3000/masks"][s, 0]), NO.REASONS)
        assert v.noise_reference_source == str(fx["override/sources"][i]) == "validated_conservative"
        assert v.used_single_spectrum_fallback == bool(fx["override/scalars"][i, 1])
        want_noise, want_snr = fx["override/checkpoints"][i]
        d = float(np.max(np.abs(v.noise_spectrum_db[chk] - want_noise)))
        worst["noise_spectrum_db"] = max(worst["noise_spectrum_db"], d)
        assert d <= noise_tol, (s, d)
        d = np.abs(v.spectral_snr_db[chk] - want_snr)
        worst["spectral_snr_db"] = max(worst["spectral_snr_db"], float(np.max(d)))
        assert np.all(d <= input_tol * (2.0 + np.power(10.0, -want_snr / 10.0))), (s, d)
        want = fx["override/scalars"][i, 0]
        d = abs(v.snr_db - want)
        worst["snr_db"] = max(worst["snr_db"], d)
        assert d <= input_tol * (2.0 + 10.0 ** (-want / 10.0)), (s, d)
    print("voice capture batch: largest |GPU - reference|:", {k: f"{v:.3e}" for k, v in worst.items()})
