"""GPU parity of the batched product resampler with the CPU oracle (oracle/af_resampler.c), plus the
reference's published measurements (tests/golden/resampler_report_pins.json) through the HIP path.

The kernel and the oracle evaluate every sinc dot product as the same fused multiply-add chain and the same
cubic, on the same host-built coefficient table and positions: outputs must be BIT-EXACT (f64).
"""
import json
import pathlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import resampler_forms as F
import resampler_stimuli as R

pytestmark = pytest.mark.gpu

PINS = json.loads((pathlib.Path(__file__).parent / "golden" / "resampler_report_pins.json").read_text())


@pytest.fixture(scope="module")
def mi():
    import mic_eq_mi

    assert mic_eq_mi.CORE_AVAILABLE, "HIP library missing: GPU tests never fall back to the CPU"
    return mic_eq_mi


@pytest.mark.parametrize("fi,fo", [(44_100, 48_000), (48_000, 44_100), (32_000, 48_000), (96_000, 48_000), (48_000, 16_000)])
def test_bit_exact_against_oracle(mi, oracle, fi, fo):
    """Ragged batch (67 streams), length that is not a multiple of the chunk, five ratios at sinc length 128: the matrix-core
    kernel (three of them) and the vector kernel with segments of 64 and 32 outputs, six streams of stream groups 0 and 3
    compared.  Every form, every stream and the tails: test_every_form_is_bit_exact_on_every_stream below."""
    from mic_eq_mi import mic_eq_core as core

    rng = np.random.default_rng(fi ^ fo)
    n = 3 * 1024 + 517
    x = rng.standard_normal((67, n)) * 0.25
    x[3] = 0.0
    x[5, 1000] = 1.0
    out, delay, expected, blocks, _ = core.simulate_product_resampler_batch(x, fi, fo)
    for s in (0, 3, 5, 63, 64, 66):
        want, d, e, b = oracle.simulate_product_resampler(x[s], fi, fo)
        assert (delay, expected, blocks) == (d, e, b)
        assert out.shape[1] == want.size
        assert np.array_equal(out[s], want), (s, float(np.max(np.abs(out[s] - want))))


SILENT, IMPULSE_MID, IMPULSE_FIRST, IMPULSE_LAST, CONSTANT, SUBNORMAL, HUGE = 3, 5, 17, 34, 45, 51, 66


def _form_batch(n, seed):
    """67 streams of noise at 0.25, with the special rows spread over all four stream groups of a matrix-core workgroup
    (16 streams each) and the last, partly filled workgroup: silence, an impulse in the middle, at frame 0 and at the last
    frame, a constant 1.0, noise at 1e-308 (f64 subnormal samples and products) and at 1e300."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((F.N_STREAMS, n)) * 0.25
    x[SILENT] = 0.0
    x[CONSTANT] = 1.0
    x[SUBNORMAL] *= 4e-308
    x[HUGE] *= 4e300
    for s in (IMPULSE_MID, IMPULSE_FIRST, IMPULSE_LAST):
        x[s] = 0.0
    if n:
        x[IMPULSE_MID, min(1000, n - 1)] = 1.0
        x[IMPULSE_FIRST, 0] = 1.0
        x[IMPULSE_LAST, n - 1] = 1.0
    return x


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _oracle_batch(oracle, x, row):
    """[n_streams, n_out] f64 from the oracle, stream by stream on a thread pool, and its (delay, expected, blocks)"""
    oracle.simulate_product_resampler(x[0], row.fi, row.fo, row.chunk, row.sinc_len, row.window)  # binds the signature once
    with ThreadPoolExecutor(max_workers=16) as pool:
        per = list(pool.map(lambda s: oracle.simulate_product_resampler(x[s], row.fi, row.fo, row.chunk, row.sinc_len, row.window),
                            range(x.shape[0])))
    assert len({p[1:] for p in per}) == 1 and len({p[0].size for p in per}) == 1
    return np.stack([p[0] for p in per]), per[0][1:]


def _assert_all_streams_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    differ = _bits64(got) != _bits64(want)
    if differ.any():
        streams = np.flatnonzero(differ.any(axis=1))
        first = int(np.flatnonzero(differ.any(axis=0))[0])
        raise AssertionError(f"{what}: {streams.size} streams differ from the oracle: {streams.tolist()}, first differing output {first}")


@pytest.mark.parametrize("row", F.ROWS, ids=lambda r: r.id)
def test_every_form_is_bit_exact_on_every_stream(mi, oracle, row):
    """Every launch form of the one-shot kernels (tests/resampler_forms.py), 67 streams, all of them compared as bit patterns:
    the tile geometry edges, two or three input lengths per row for the tails (partial last tile, odd last output, a last
    segment of one output, a whole job shorter than a segment, a pure flush), impulses at both ends, a constant, subnormal
    and very large samples."""
    from mic_eq_mi import mic_eq_core as core

    r = F.make_resampler(core, row)
    assert r.launch_form == row.form
    for n in row.lengths:
        x = _form_batch(n, row.fi ^ row.fo ^ n)
        want, (delay, expected, blocks) = _oracle_batch(oracle, x, row)
        n_out, b = r.plan(n)
        assert (n_out, b, r.output_delay, r.expected_frames(n)) == (want.shape[1], blocks, delay, expected), (row.id, n)
        got = r.process(x)
        _assert_all_streams_equal(got, want, (row.id, n))
        if n > 1 and n_out > 2 * row.sinc_len:
            assert np.any(want[SUBNORMAL] != 0.0) and np.all(np.abs(want[SUBNORMAL]) < 1e-306)
            assert np.all(np.isfinite(want[HUGE])) and np.max(np.abs(want[HUGE])) > 1e299
    r.close()


@pytest.mark.parametrize("row_id", ["44100-48000-sinc128", "48000-40000-sinc128"])
def test_strided_device_entry_point(mi, oracle, row_id):
    """af_resampler_process_device with in_stride > n_in and out_stride > n_out, one matrix-core and one vector row: NaN behind
    every input row must not be read, the cells behind every output row must not be written."""
    import torch

    from mic_eq_mi import mic_eq_core as core

    row = next(r for r in F.ROWS if r.id == row_id)
    n = 1024
    x = _form_batch(n, 1234)
    want, _ = _oracle_batch(oracle, x, row)
    r = F.make_resampler(core, row)
    assert r.launch_form == row.form
    n_out, _ = r.plan(n)
    assert n_out == want.shape[1]
    padded = np.full((F.N_STREAMS, n + 3), np.nan)
    padded[:, :n] = x
    d_in = torch.from_numpy(padded).cuda()
    d_out = torch.full((F.N_STREAMS, n_out + 5), 7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    r.process_device(d_in.data_ptr(), d_out.data_ptr(), n, F.N_STREAMS, n + 3, n_out + 5)
    torch.cuda.synchronize()
    y = d_out.cpu().numpy()
    assert not np.isnan(y).any(), "a kernel read past n_in"
    assert (y[:, n_out:] == 7.0).all(), "the resampler wrote past a row's frames"
    _assert_all_streams_equal(y[:, :n_out], want, row_id)
    r.close()


def test_operator_surface_matches_reference(mi, oracle):
    """tests.rs:194-257: tuple shape, expected = 48000, delay, len >= delay + expected, timings non-empty,
    configuration tuple, and the ValueError contract."""
    out, delay, expected, timings = mi.simulate_product_resampler([0.0] * 44_100, 44_100, 48_000, 1024, None, None)
    assert expected == 48_000 and delay == 69 and len(out) >= delay + expected and len(timings) == 44
    assert isinstance(out, list) and isinstance(out[0], float) and all(isinstance(t, int) for t in timings)
    assert mi.product_resampler_configuration() == (128, "blackman", "cubic", 256, 1024)
    for args in (([0.0], 0, 48_000, 1024, None, None), ([float("nan")], 48_000, 44_100, 1024, None, None),
                 ([0.0], 48_000, 44_100, 0, None, None), ([0.0], 48_000, 44_100, 1025, None, None),
                 ([0.0], 48_000, 44_100, 1024, 96, None), ([0.0], 48_000, 44_100, 1024, None, "unknown")):
        with pytest.raises(ValueError):
            mi.simulate_product_resampler(*args)
    # other windows / a longer sinc run too and agree with the oracle
    x = np.sin(np.arange(5000) * 0.05)
    for sinc_len, window in ((256, "blackman_harris_squared"), (64, "hann"), (128, "blackman_squared")):
        got = np.asarray(mi.simulate_product_resampler(x.tolist(), 48_000, 44_100, 1024, sinc_len, window)[0])
        want = oracle.simulate_product_resampler(x, 48_000, 44_100, 1024, sinc_len, window)[0]
        assert np.array_equal(got, want), (sinc_len, window)


def test_published_measurements_through_the_gpu(mi):
    """evaluation/resampler-quality-report.json figures, computed from the HIP path's output."""
    pins = PINS["product"]

    def run(x, fi, fo):
        out, delay, expected, _ = mi.simulate_product_resampler(x, fi, fo)
        return np.asarray(out)[:expected], delay

    for fi, fo in ((44_100, 48_000), (48_000, 44_100)):
        x = np.zeros(fi)
        x[fi // 2] = 1.0
        y, delay = run(x, fi, fo)
        assert delay == pins["delays"][f"{fi}->{fo}"]
        assert int(np.argmax(np.abs(y))) == pins["impulse_peak_index"][f"{fi}->{fo}"]
    noise = R.stopband_noise()
    y, _ = run(noise, 48_000, 44_100)
    swept = R.db_ratio(R.rms(R.steady(y, 44_100)), R.rms(R.steady(noise, 48_000)))
    assert abs(swept - pins["swept_noise_attenuation_db"]) <= 1e-10
    src = R.roundtrip_noise()
    up, _ = run(src, 44_100, 48_000)
    back, _ = run(up, 48_000, 44_100)
    n = min(src.size, back.size)
    err = back[4096 : n - 4096] - src[4096 : n - 4096]
    assert abs(R.db_ratio(R.rms(src[4096 : n - 4096]), R.rms(err)) - pins["roundtrip_snr_db"]) <= 1e-10
    assert abs(float(np.max(np.abs(err))) - pins["roundtrip_max_absolute_error"]) <= 1e-14
    y, _ = run(R.sine(44_100, 21_000.0, 2.0), 44_100, 48_000)
    image = R.db_ratio(R.tone_amplitude(y, 48_000, 44_100.0 - 21_000.0), R.tone_amplitude(y, 48_000, 21_000.0))
    assert abs(image - pins["worst_image_db"]) <= 1e-9


def test_long_stream_properties(mi):
    """Size-independent properties at a BASELINE-sized stream (10 s): linearity and shift-by-a-period.
    44.1 -> 48 kHz repeats its sub-sample phase every 147 input / 160 output frames."""
    from mic_eq_mi import mic_eq_core as core

    rng = np.random.default_rng(7)
    n = 441_000
    a = rng.standard_normal(n) * 0.1
    b = rng.standard_normal(n) * 0.1
    shifted = np.concatenate([np.zeros(147 * 64), a])[:n]
    batch = np.stack([a, b, a + b, shifted])
    out, delay, expected, blocks, _ = core.simulate_product_resampler_batch(batch, 44_100, 48_000)
    assert expected == 480_000 and out.shape[1] >= expected + delay
    assert np.max(np.abs(out[2] - (out[0] + out[1]))) <= 1e-13
    # the shifted copy is the original delayed by 160*64 output frames (positions accumulate rounding: ~1e-9)
    k = 160 * 64
    tail = 256  # the shifted copy is cut at n: its last sinc_len/2 * ratio frames see zeros instead of the end of `a`
    assert np.max(np.abs(out[3][k : expected - tail] - out[0][: expected - k - tail])) <= 1e-8
