"""The two kernels of the second-passage measurements (csrc/af_setup_verification.hip) alone, through the C ABI, against the
restatement (tests/ref/setup_verification_ref.c over csrc/af_setup_verification_math.h, which tests/test_setup_verification_ref.py
holds to the reference).

Shape kernel: 1, 64, 65 and 70 streams; nperseg 4096 (1018 masked bins, even), 2048 (509, odd), 64 (16 bins, no low SNR band) and
16 (4 bins: the +inf path); all four presets and every clip-driving spectrum inside one batch; NaN in the SNR rows; no SNR rows.
Level kernel: 1, 64, 65 and 70 streams; lengths 1, 63, 64, 65, 4097 and 201 600 (and 8193 and 32 769, one past a buffer and past
a pass of four, and 8191 and 16 383, whose last buffer's right-hand nodes still hold more than 128 samples after six halvings),
unequal per signal and stream; a non-finite sample at the first and at the last index; peaks of exactly 0.999 and 1.0; and every
kind of short last buffer (tails of 7689..8191 samples) on random signals against np.sum.

Selections (medians), flags, counts, the band means and the sums of squares are bit-equal to the restatement: both run the same
operations in the same order.  The dB and RMS fields go through log10, log2, exp and sqrt of two libraries: within 1e-12, the
bound tests/test_gpu_voice_spectrum.py holds dB fields to.  A reused handle, and a smaller batch after a larger one, give equal
bytes."""
import numpy as np
import pytest

import setup_verification_oracle as O
import setup_verification_stimulus as SV

pytestmark = pytest.mark.gpu

DB_ALLOWED = 1e-12
STREAMS = 70
EXACT = ("masked_bins", "snr_available", "band_present", "band_snr_db", "reserved")
CLOSE = ("spectral_target_error_before_db", "spectral_target_error_after_db", "shape_delta_db")
LENGTHS = SV.LENGTHS + (8193, 32_769, 8191, 16_383)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.fixture(scope="module")
def sv():
    from mic_eq_mi import setup_verification

    return setup_verification


@pytest.fixture(scope="module")
def shape_cases():
    """Per nperseg: the 70-stream batch and the restatement's rows with and without the SNR rows, computed once."""
    cases = {}
    for nperseg in SV.NPERSEGS:
        original, before, after, snr, presets = SV.batch(nperseg, STREAMS)
        f = SV.grid(nperseg)
        rows = {use: np.array([O.measure_row(f, original[s], before[s], after[s], snr[s] if use else None, presets[s], [None] * 5)
                               for s in range(STREAMS)]) for use in (True, False)}
        cases[nperseg] = (original, before, after, snr, presets, rows)
    return cases


def _compare_shape(got, want, where):
    worst = 0.0
    for name in EXACT:
        assert _same(got[name], want[name]), (where, name)
    for side in ("offsets_before", "offsets_after"):  # means and their balance: the same sums; the tilt goes through log10
        assert _same(got[side][:, [0, 1, 2, 4]], want[side][:, [0, 1, 2, 4]]), (where, side)
        worst = max(worst, float(np.max(np.abs(got[side][:, 3] - want[side][:, 3]))))
    for name in CLOSE:
        assert _same(np.isfinite(got[name]), np.isfinite(want[name])) and _same(np.isnan(got[name]), np.isnan(want[name])), (where, name)
        finite = np.isfinite(want[name])
        if finite.any():
            worst = max(worst, float(np.max(np.abs(got[name][finite] - want[name][finite]))))
    return worst


@pytest.mark.parametrize("nperseg", SV.NPERSEGS)
def test_shape_kernel_matches_the_restatement(sv, shape_cases, nperseg):
    original, before, after, snr, presets, rows = shape_cases[nperseg]
    assert set(presets[:8]) == set(SV.PRESETS)
    handle = sv.SetupVerification(SV.FS, nperseg, STREAMS)
    worst, first = 0.0, None
    for n in (70, 1, 64, 65):
        for use in (True, False):
            got = handle.measure(original[:n], before[:n], after[:n], presets[:n], snr[:n] if use else None)
            worst = max(worst, _compare_shape(got, rows[use][:n], (nperseg, n, use)))
            if first is None:
                first = got
            elif use:  # a smaller batch after a larger one, on a reused handle: the bytes of the first call's rows
                assert got.tobytes() == first[:n].tobytes(), (nperseg, n)
    again = handle.measure(original, before, after, presets, snr)
    assert again.tobytes() == first.tobytes()
    handle.close()
    fresh = sv.SetupVerification(SV.FS, nperseg, 1)
    assert fresh.measure(original[:1], before[:1], after[:1], presets[:1], snr[:1]).tobytes() == first[:1].tobytes()
    fresh.close()
    print(f"nperseg {nperseg}: largest |kernel - restatement| over the dB fields = {worst:.3e}")
    want = rows[True]
    if SV.MASKED_BINS[nperseg] < 8:
        assert np.all(np.isposinf(want["spectral_target_error_before_db"])) and np.all(want["offsets_before"] == 0.0)
    else:
        assert np.all(np.isfinite(want["spectral_target_error_after_db"]))
    if nperseg >= 2048:  # the NaN rows: stream 1 in the body band only, stream 2 everywhere
        assert np.isnan(want["band_snr_db"][1]).tolist() == [False, True, False, False] and np.all(np.isnan(want["band_snr_db"][2]))
        assert np.all(np.isfinite(want["band_snr_db"][3]))
    assert worst <= DB_ALLOWED


def _level_batch(n_streams):
    """Five signals per stream with unequal lengths; the special samples the docstring lists."""
    signals = [[SV.signal(LENGTHS[(s + 3 * k) % len(LENGTHS)], s + k) for s in range(n_streams)] for k in range(5)]
    signals[0][0][0] = np.nan                      # a NaN at the first index
    signals[1][1][-1] = np.inf                     # an infinity at the last index
    big = max(range(n_streams), key=lambda s: signals[2][s].size)
    signals[2][big][-1] = -np.inf                  # ... and at the last index of the longest passage
    signals[2][(big + 1) % n_streams][0] = np.float32(0.999)                                   # clipped at :1490, not at :1677
    signals[3][2][signals[3][2].size // 2] = np.float32(-1.0)                                   # clipped at both
    signals[3][3][0] = np.nextafter(np.float32(0.999), np.float32(0.0))                         # the float below 0.999: neither
    signals[4][4][-1] = np.nextafter(np.float32(1.0), np.float32(0.0))                          # below 1.0: :1490 only
    return signals


@pytest.mark.parametrize("n_streams", (1, 64, 65, 70))
def test_level_kernel_matches_the_restatement_and_numpy(sv, n_streams):
    signals = _level_batch(max(n_streams, 8))
    signals = [rows[:n_streams] for rows in signals]
    spectra = np.zeros((n_streams, 9))  # nperseg 16: the shape side has nothing to do
    handle = sv.SetupVerification(SV.FS, 16, n_streams)
    got = handle.measure(spectra, spectra, spectra, "flat", noise=signals[0], original=signals[1], verification=signals[2],
                         rendered=signals[3], rendered_noise=signals[4])
    f = SV.grid(16)
    worst = 0.0
    for s in range(n_streams):
        want = O.measure_row(f, spectra[s], spectra[s], spectra[s], None, "flat", [signals[k][s] for k in range(5)])
        for name in ("sum_squares", "peak", "non_finite", "clipped_0999", "clipped_1"):
            assert _same(got[name][s], want[name]), (s, name, got[name][s], want[name])
        for k in range(5):
            x = signals[k][s].astype(np.float64)
            assert _same(got["sum_squares"][s][k], np.sum(x * x)), (s, k)  # NumPy's own order
            assert got["non_finite"][s][k] == (not np.isfinite(x).all())
            if np.isfinite(x).all():
                assert got["peak"][s][k] == np.max(np.abs(x))
                assert got["clipped_0999"][s][k] == (np.max(np.abs(x)) >= 0.999) and got["clipped_1"][s][k] == (np.max(np.abs(x)) >= 1.0)
        finite = np.isfinite(want["rms_db"])
        assert _same(np.isfinite(got["rms_db"][s]), finite)
        worst = max(worst, float(np.max(np.abs(got["rms_db"][s][finite] - want["rms_db"][finite]), initial=0.0)))
    if n_streams >= 10:  # every special sample of _level_batch lies within the first ten streams
        assert got["clipped_0999"].sum() >= 3 and got["clipped_1"].sum() >= 1 and got["non_finite"].sum() == 3
        assert got["clipped_0999"][3][3] == 0 and got["clipped_0999"][4][4] == 1 and got["clipped_1"][4][4] == 0
    again = handle.measure(spectra, spectra, spectra, "flat", noise=signals[0], original=signals[1], verification=signals[2],
                           rendered=signals[3], rendered_noise=signals[4])
    assert again.tobytes() == got.tobytes()
    handle.close()
    print(f"{n_streams} streams: largest |rms_db - restatement| = {worst:.3e} dB")
    assert worst <= DB_ALLOWED


def test_level_kernel_short_last_buffers_equal_numpy(sv):
    """NumPy cuts the halves of a pairwise sum at multiples of eight, so in a last buffer of 7689..8191 samples some node is still
    above 128 samples after six halvings and splits once more: every eighth such tail and both ends, alone and behind one, two
    and four whole buffers, on random signals (on smooth ones the two orders often round alike).  Summing such a node as one block
    instead differs from np.sum on 9 of these 1300 signals (worked out on the CPU), so this case tells the two apart."""
    rng = np.random.default_rng(20_261)
    tails = sorted(set(range(7689, 8192, 8)) | {8190, 8191})
    assert len(tails) == 65
    spectra = np.zeros((len(tails), 9))
    handle = sv.SetupVerification(SV.FS, 16, len(tails))
    for whole in (0, 1, 2, 4):  # all five signal slots: 1300 signals (the two orders round differently on about one in a hundred)
        signals = [[(0.25 * rng.standard_normal(whole * 8192 + tail)).astype(np.float32) for tail in tails] for _ in range(5)]
        got = handle.measure(spectra, spectra, spectra, "flat", noise=signals[0], original=signals[1], verification=signals[2],
                             rendered=signals[3], rendered_noise=signals[4])
        for k in range(5):
            for s, x in enumerate(signals[k]):
                a = x.astype(np.float64)
                assert got["sum_squares"][s][k] == float(np.sum(a * a)) == O.sum_squares(x), (whole, k, x.size)
                assert got["peak"][s][k] == float(np.max(np.abs(a)))
    handle.close()


def test_equal_lengths_absent_signals_and_the_device_entry_point(sv):
    import torch

    n_streams, nperseg, n = 6, 2048, 4097
    original, before, after, snr, presets = SV.batch(nperseg, n_streams)
    audio = np.stack([SV.signal(n, s) for s in range(n_streams)])
    rendered = np.stack([SV.signal(n + 40, s + 9) for s in range(n_streams)])
    handle = sv.SetupVerification(SV.FS, nperseg, n_streams)
    host = handle.measure(original, before, after, presets, snr, verification=audio, rendered=rendered)
    f = SV.grid(nperseg)
    for s in range(n_streams):
        want = O.measure_row(f, original[s], before[s], after[s], snr[s], presets[s], [None, None, audio[s], rendered[s], None])
        for name in ("sum_squares", "peak", "non_finite", "clipped_0999", "clipped_1", "band_snr_db", "band_present"):
            assert _same(host[name][s], want[name]), (s, name)
        assert np.all(host["rms_db"][s][[0, 1, 4]] == -120.0) and np.all(host["sum_squares"][s][[0, 1, 4]] == 0.0)
        assert np.max(np.abs(host["rms_db"][s] - want["rms_db"])) <= DB_ALLOWED
    # the same through device pointers, with strides wider than the rows and per-stream lengths for one signal
    dev = torch.device("cuda:0")
    pad = 7
    spectra = [torch.zeros((n_streams, f.size + pad), dtype=torch.float64, device=dev) for _ in range(4)]
    for t, a in zip(spectra, (original, before, after, snr)):
        t[:, :f.size] = torch.from_numpy(a).to(dev)
    d_audio, d_rendered = torch.from_numpy(audio).to(dev), torch.from_numpy(rendered).to(dev)
    d_rows = torch.zeros(n_streams * sv.ROW_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    lengths = np.full(n_streams, n + 40, dtype=np.int64)
    handle.measure_device(n_streams, spectra[0].data_ptr(), spectra[1].data_ptr(), spectra[2].data_ptr(), f.size + pad, presets,
                          spectra[3].data_ptr(), f.size + pad,
                          [None, None, (d_audio.data_ptr(), n, n, None), (d_rendered.data_ptr(), n + 40, n + 40, lengths), None],
                          d_rows.data_ptr())
    torch.cuda.synchronize()
    device_rows = np.frombuffer(d_rows.cpu().numpy().tobytes(), dtype=sv.ROW_DTYPE)
    assert device_rows.tobytes() == host.tobytes()
    handle.close()
