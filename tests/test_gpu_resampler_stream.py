"""GPU parity of the streaming product resampler, and of an engine with device-rate I/O, with the CPU oracle driven through
the realtime loop's protocol (tests/resampler_stream_oracle.py).

The device evaluates the oracle's fused multiply-add chains on the same table and the same positions; f32 -> f64 is exact and
f64 -> f32 rounds to nearest even on both sides: every audio comparison here is BIT-EXACT.  The one exception is the
suppressor case at the end, which checks counts and finiteness only and says why.
"""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import chain_oracle as CO
import resampler_forms as F
import resampler_stream_oracle as RS
import signals as S

pytestmark = pytest.mark.gpu

N_STREAMS = F.N_STREAMS
CALLS = F.CALLS  # zero-output calls and a 3000-frame call among them
OTHER_PARTITION = F.OTHER_PARTITION
GROWING_CALLS = [64, 99, 153, 237, 367, 569, 881, 1365, 2115, 3277, 5077, 8000]  # the first fills no 256-frame chunk
STEADY_CALLS = [700] * 10  # behind them: nothing grows any more, so the eight staging slots are reused in turn
RATIOS = [(44_100, 48_000), (48_000, 44_100), (32_000, 48_000), (96_000, 48_000), (48_000, 16_000)]  # test_bit_exact_against_oracle's


@pytest.fixture(scope="module")
def core():
    import mic_eq_mi
    from mic_eq_mi import mic_eq_core

    assert mic_eq_mi.CORE_AVAILABLE, "HIP library missing: GPU tests never fall back to the CPU"
    return mic_eq_core


def _batch(n_streams, n, seed):
    """one silent stream, one impulse, the rest noise at 0.25"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n_streams, n)) * 0.25).astype(np.float32)
    x[3] = 0.0
    x[5] = 0.0
    x[5, min(1000, n - 1)] = 1.0
    return x


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _oracle_calls(x, calls, fi, fo, streams=None, **kw):
    """per call: [len(streams), m] f32 from the helper, stream by stream on a thread pool"""
    RS._lib()
    streams = list(range(x.shape[0])) if streams is None else list(streams)
    with ThreadPoolExecutor(max_workers=16) as pool:
        per_stream = list(pool.map(lambda s: RS.run_calls(x[s], calls, fi, fo, **kw), streams))
    return [np.stack([per_stream[i][c] for i in range(len(streams))]) for c in range(len(calls))]


def _push_all(r, x, calls):
    outs, at = [], 0
    for n in calls:
        predicted = r.output_frames(n)
        y = r.push(x[:, at : at + n])
        assert y.shape == (x.shape[0], predicted), (n, y.shape, predicted)
        outs.append(y)
        at += n
    return outs


@pytest.mark.parametrize("fi,fo", RATIOS)
def test_every_call_is_bit_exact(core, fi, fo):
    x = _batch(N_STREAMS, sum(CALLS), fi ^ fo)
    want = _oracle_calls(x, CALLS, fi, fo)
    assert any(w.shape[1] == 0 for w in want) and any(w.shape[1] > 0 for w in want)
    r = core.StreamResampler(fi, fo, n_streams=N_STREAMS)
    o = RS.StreamOracle(fi, fo)
    at = 0
    got = []
    for n, w in zip(CALLS, want):
        assert r.output_frames(n) == w.shape[1], n  # the host replay predicts the call
        y = r.push(x[:, at : at + n])
        o.push(x[0, at : at + n])
        at += n
        assert y.shape == w.shape, (n, y.shape, w.shape)
        differ = np.flatnonzero((_bits(y) != _bits(w)).any(axis=1))
        assert differ.size == 0, (fi, fo, n, differ[:8].tolist())
        assert r.pending_input == o.pending_input
        got.append(y)
    assert r.frames_in == sum(CALLS) and r.frames_out == sum(w.shape[1] for w in want)
    # the same input under another partition: identical bytes
    r.reset()
    again = np.concatenate(_push_all(r, x, OTHER_PARTITION), axis=1)
    assert np.array_equal(_bits(again), _bits(np.concatenate(got, axis=1)))
    r.close()
    o.close()


@pytest.mark.parametrize("row", [r for r in F.ROWS if r.calls], ids=lambda r: r.id)
def test_every_form_streams_bit_exact(core, row):
    """The launch forms the ratios above do not reach (tests/resampler_forms.py): the 32-stream matrix-core kernel, the vector
    kernels with segments of 128 and 8 outputs, the geometry edges of both tiles, and chunks of 40 and 160 frames, where
    the split between the carried plane and the call's input moves through a tile from call to call.  Every call, all 67
    streams, bit for bit; then the same frames under a second partition."""
    calls, other = list(row.calls), list(row.other)
    kw = dict(chunk_size=row.chunk, sinc_len=row.sinc_len, window=row.window)
    x = _batch(N_STREAMS, sum(calls), row.fi ^ row.fo ^ row.sinc_len)
    want = _oracle_calls(x, calls, row.fi, row.fo, **kw)
    assert any(w.shape[1] == 0 for w in want) and any(w.shape[1] > 0 for w in want)
    r = F.make_stream_resampler(core, row, N_STREAMS)
    assert r.launch_form == row.form
    o = RS.StreamOracle(row.fi, row.fo, **kw)
    at = 0
    got = []
    for n, w in zip(calls, want):
        assert r.output_frames(n) == w.shape[1], n
        y = r.push(x[:, at : at + n])
        o.push(x[0, at : at + n])
        at += n
        assert y.shape == w.shape, (n, y.shape, w.shape)
        differ = _bits(y) != _bits(w)
        if differ.any():
            streams = np.flatnonzero(differ.any(axis=1)).tolist()
            raise AssertionError(f"{row.id}, call of {n} frames at {at - n}: streams {streams} differ, first differing output "
                                 f"{int(np.flatnonzero(differ.any(axis=0))[0])} of {w.shape[1]}")
        assert r.pending_input == o.pending_input
        got.append(y)
    assert r.frames_in == sum(calls) and r.frames_out == sum(w.shape[1] for w in want)
    r.reset()
    again = np.concatenate(_push_all(r, x, other), axis=1)
    assert np.array_equal(_bits(again), _bits(np.concatenate(got, axis=1)))
    r.close()
    o.close()


def test_long_run_positions(core):
    """310 chunks: the position is advanced by the crate's repeated addition, call after call."""
    fi, fo, chunks = 44_100, 48_000, 310
    n = chunks * 1024
    x = _batch(N_STREAMS, n, 99)
    calls = [10_007] * (n // 10_007) + [n % 10_007]
    check = (0, 3, 5, 63, 64, 66)
    want = np.concatenate(_oracle_calls(x, calls, fi, fo, streams=check), axis=1)
    r = core.StreamResampler(fi, fo, n_streams=N_STREAMS)
    got = np.concatenate(_push_all(r, x, calls), axis=1)
    assert r.pending_input == 0 and got.shape[1] == want.shape[1]
    assert np.array_equal(_bits(got[list(check)]), _bits(want))
    r.close()


def test_reset_and_clear_pending_mid_stream(core):
    fi, fo = 48_000, 44_100
    x = _batch(N_STREAMS, 9000, 5)
    r = core.StreamResampler(fi, fo, n_streams=N_STREAMS)
    oracles = [RS.StreamOracle(fi, fo) for _ in range(N_STREAMS)]

    def step(lo, hi):
        y = r.push(x[:, lo:hi])
        w = np.stack([o.push(x[s, lo:hi]) for s, o in enumerate(oracles)])
        assert y.shape == w.shape and np.array_equal(_bits(y), _bits(w)), (lo, hi)
        assert r.pending_input == oracles[0].pending_input

    step(0, 1500)
    r.clear_pending()
    for o in oracles:
        o.clear_pending()
    assert r.pending_input == 0
    step(1500, 2000)
    step(2000, 4100)
    r.reset()
    for o in oracles:
        o.reset()
    assert r.pending_input == 0 and r.frames_in == 0
    step(4100, 4300)
    step(4300, 9000)
    r.close()


def test_refused_calls_change_nothing(core):
    fi, fo = 44_100, 48_000
    x = _batch(N_STREAMS, 6000, 17)
    want = _oracle_calls(x, [700, 2500, 2800], fi, fo)
    r = core.StreamResampler(fi, fo, n_streams=N_STREAMS)
    assert np.array_equal(_bits(r.push(x[:, :700])), _bits(want[0]))
    need = r.output_frames(2500)
    with pytest.raises(ValueError, match="too small"):
        r.push(x[:, 700:3200], out_capacity=need - 1)
    bad = x[:, 700:3200].copy()
    bad[66, 2499] = np.nan
    with pytest.raises(ValueError, match="samples must be finite"):
        r.push(bad)
    assert r.pending_input == 700 and r.frames_in == 700
    assert np.array_equal(_bits(r.push(x[:, 700:3200])), _bits(want[1]))
    assert np.array_equal(_bits(r.push(x[:, 3200:])), _bits(want[2]))
    r.close()


def test_push_device_on_a_side_stream_matches_push_host(core):
    import torch

    fi, fo = 44_100, 48_000
    x = _batch(N_STREAMS, sum(CALLS), 23)
    host = core.StreamResampler(fi, fo, n_streams=N_STREAMS)
    dev = core.StreamResampler(fi, fo, n_streams=N_STREAMS)
    side = torch.cuda.Stream()
    xin = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    at = 0
    for n in CALLS:
        w = host.push(x[:, at : at + n])
        cap = dev.output_frames(n)
        stride = cap + 5
        out = torch.full((N_STREAMS, stride), 7.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        made = dev.push_device(xin.data_ptr() + 4 * at, n, x.shape[1], out.data_ptr(), cap, stride, side.cuda_stream)
        side.synchronize()
        assert made == w.shape[1]
        y = out.cpu().numpy()
        assert np.array_equal(_bits(y[:, :made]), _bits(w)), n
        assert (y[:, made:] == 7.0).all(), "the resampler wrote past a row's frames"
        at += n
    host.close()
    dev.close()
    # Twelve pushes queued on the side stream with no host wait between them, each about 1.5 times the one before: every
    # call's position records outgrow the pinned slots (which wait for the copies in flight and are reallocated) and their
    # device buffer (replaced, the old one retired behind an event).  Then ten equal pushes that fit: the eight slots are
    # reused in turn while earlier copies may still be in flight, each after a wait on its own event.  65 streams: one
    # full 64-stream workgroup and a tail.  The joined output against the oracle, bit for bit.
    kw = dict(chunk_size=256, sinc_len=64, window="hann")
    calls = GROWING_CALLS + STEADY_CALLS
    x = _batch(65, sum(calls), 29)
    want = np.concatenate(_oracle_calls(x, calls, fi, fo, **kw), axis=1)
    dev = core.StreamResampler(fi, fo, n_streams=65, **kw)
    made = []
    xin = torch.from_numpy(x).cuda()
    out = torch.full((65, want.shape[1] + 5), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    at = done = 0
    for n in calls:
        cap = dev.output_frames(n)
        made.append(dev.push_device(xin.data_ptr() + 4 * at, n, x.shape[1], out.data_ptr() + 4 * done, cap, out.shape[1], side.cuda_stream))
        assert made[-1] == cap
        at += n
        done += cap
    side.synchronize()
    assert done == want.shape[1] and made[0] == 0 and sum(m > 0 for m in made[:12]) >= 9 and min(made[12:]) > 0, made
    y = out.cpu().numpy()
    differ = np.flatnonzero((_bits(y[:, :done]) != _bits(want)).any(axis=1))
    assert differ.size == 0, differ[:8].tolist()
    assert (y[:, done:] == 7.0).all(), "the resampler wrote past a row's frames"
    dev.close()


@pytest.mark.parametrize("sinc_len,window", [(256, "blackman_harris_squared"), (64, "hann")])
def test_other_sinc_lengths_and_windows(core, sinc_len, window):
    fi, fo = 48_000, 44_100
    x = _batch(N_STREAMS, sum(CALLS), sinc_len)
    want = _oracle_calls(x, CALLS, fi, fo, sinc_len=sinc_len, window=window)
    r = core.StreamResampler(fi, fo, n_streams=N_STREAMS, sinc_len=sinc_len, window=window)
    got = _push_all(r, x, CALLS)
    for n, y, w in zip(CALLS, got, want):
        assert y.shape == w.shape and np.array_equal(_bits(y), _bits(w)), (n, sinc_len, window)
    r.close()


# --------------------------------------------------------------------------------------------------------- the engine
ENGINE_STREAMS = 131
ENGINE_CALLS = [441, 1500, 37, 1024, 2999, 1, 800, 2222, 441, 441]
LIMITER_ONLY = dict(S.limiter_settings(2.0), compressor_enabled=False)  # EQ + limiter + true-peak limiter: bit-exact


def _engine(core, rate_in, rate_out, suppressor=False):
    eng = core.Engine(48_000.0, ENGINE_STREAMS)
    core.configure_auto_eq_chain(eng, 48_000.0, S.LIMITER_BANDS, LIMITER_ONLY)
    if suppressor:
        eng.set_suppressor_enabled(1)
    eng.set_io_sample_rates(rate_in, rate_out)
    return eng


def _engine_oracle(x, calls, rate_in, rate_out):
    """helper(in) -> chain_oracle -> helper(out), per stream: the output of every call, and (m1, m3) per call"""
    RS._lib()

    def one(s):
        mids = RS.run_calls(x[s], calls, rate_in, 48_000) if rate_in != 48_000 else [x[s, a:b] for a, b in _spans(calls)]
        lengths = [m.size for m in mids]
        ran = [n for n in lengths if n > 0]  # the engine is not called when no chunk completed
        mid = np.concatenate(mids)
        y, _ = CO.run_calls(mid, 48_000, S.LIMITER_BANDS, LIMITER_ONLY, ran)
        if rate_out == 48_000:
            outs = [y[a:b] for a, b in _spans(lengths)]
        else:
            o = RS.StreamOracle(48_000, rate_out)
            outs = [o.push(y[a:b]) if b > a else np.zeros(0, np.float32) for a, b in _spans(lengths)]
            o.close()
        return outs, lengths

    CO._lib()
    with ThreadPoolExecutor(max_workers=16) as pool:
        res = list(pool.map(one, range(x.shape[0])))
    lengths = res[0][1]
    return [np.stack([r[0][c] for r in res]) for c in range(len(calls))], lengths


def _spans(lengths):
    at = 0
    for n in lengths:
        yield at, at + n
        at += n


@pytest.mark.parametrize("rate_in,rate_out", [(44_100, 44_100), (16_000, 48_000)])
def test_engine_with_device_rate_io_is_bit_exact(core, rate_in, rate_out):
    from mic_eq_mi import _lib

    x = _batch(ENGINE_STREAMS, sum(ENGINE_CALLS), rate_in + 1)
    want, mids = _engine_oracle(x, ENGINE_CALLS, rate_in, rate_out)
    eng = _engine(core, rate_in, rate_out)
    fp = C.POINTER(C.c_float)

    def run(refusals):
        outs, at = [], 0
        for k, n in enumerate(ENGINE_CALLS):
            blockx = np.ascontiguousarray(x[:, at : at + n])
            plan = eng.stream_plan(n)
            assert plan == (mids[k], mids[k], want[k].shape[1]), (k, plan)
            if refusals and plan[2] > 0 and k >= 3:
                # out_stride one frame short, then a NaN, then a one-shot entry point: each refused, nothing changes
                before = (eng.io_resampler_pending(), eng.samples_processed())
                small = np.zeros((ENGINE_STREAMS, plan[2] - 1), dtype=np.float32)
                n_out = C.c_int64(0)
                rc = eng._lib.af_engine_stream_host(eng._h, blockx.ctypes.data_as(fp), n, small.ctypes.data_as(fp), plan[2] - 1, C.byref(n_out))
                assert rc == _lib.AF_ERR_INVALID_ARGUMENT and n_out.value == 0
                bad = blockx.copy()
                bad[130, n - 1] = np.inf
                with pytest.raises(ValueError, match="samples must be finite"):
                    eng.stream(bad)
                with pytest.raises(NotImplementedError, match="af_engine_stream_host"):
                    eng.process(np.ascontiguousarray(blockx.T), layout=_lib.LAYOUT_TIME_MAJOR)
                with pytest.raises(NotImplementedError, match="af_engine_stream_host"):
                    eng.process_device(0, 0, 0, 1)
                assert (eng.io_resampler_pending(), eng.samples_processed()) == before and eng.stream_plan(n) == plan
            y = eng.stream(blockx)
            assert y.shape == want[k].shape, (k, y.shape, want[k].shape)
            assert eng.last_output_samples() == plan[1]
            outs.append(y)
            at += n
        return outs

    got = run(refusals=True)
    for k, (y, w) in enumerate(zip(got, want)):
        differ = np.flatnonzero((_bits(y) != _bits(w)).any(axis=1))
        assert differ.size == 0, (rate_in, rate_out, k, differ[:8].tolist())
    assert eng.samples_processed() == sum(mids)  # engine-rate samples
    eng.reset()  # restarts both sides (and the chain): the same calls give the same bytes
    assert eng.io_resampler_pending() == (0, 0)
    again = run(refusals=False)
    assert np.array_equal(_bits(np.concatenate(again, axis=1)), _bits(np.concatenate(got, axis=1)))
    with pytest.raises(RuntimeError):  # a configuration setter: AF_ERR_STATE after streaming has started
        eng.set_io_sample_rates(0, 0)
    eng.close()


def test_engine_counts_behind_the_suppressor(core):
    """Suppressor on: counts only.  The suppressor's own parity bound (tests/test_gpu_suppressor.py) is stated for its
    stimuli at 48 kHz; behind a resampler there is no derivable bound for its audio, so none is asserted: the frames per
    call, the three queues and finiteness are."""
    rate_in, rate_out = 44_100, 44_100
    x = _batch(ENGINE_STREAMS, sum(ENGINE_CALLS), 77)
    eng = _engine(core, rate_in, rate_out, suppressor=True)
    m1s = RS.plan_counts(ENGINE_CALLS, rate_in, 48_000)
    pend_frames = 0
    out_oracle = RS.StreamOracle(48_000, rate_out)
    in_pending = 0
    at = 0
    for n, m1 in zip(ENGINE_CALLS, m1s):
        in_pending = (in_pending + n) % 1024
        m2 = ((pend_frames + m1) // 480) * 480 if m1 > 0 else 0
        if m1 > 0:
            pend_frames = pend_frames + m1 - m2
        m3 = out_oracle.push(np.zeros(m2, np.float32)).size if m2 > 0 else 0
        assert eng.stream_plan(n) == (m1, m2, m3), n
        y = eng.stream(x[:, at : at + n])
        at += n
        assert y.shape == (ENGINE_STREAMS, m3) and np.isfinite(y).all()
        assert eng.pending_input() == pend_frames
        assert eng.io_resampler_pending() == (in_pending, out_oracle.pending_input)
    out_oracle.close()
    eng.close()
