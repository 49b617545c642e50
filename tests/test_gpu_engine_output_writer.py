"""The output writer behind the engine: 70 streams through the front end and the dynamics chain, at the engine rate and with
a 48 -> 44.1 kHz output side.  An engine with the writer on must equal, bit for bit, a second engine of the same
configuration whose rows go through the CPU restatement (tests/ref/output_writer_ref.c) with the same queue fills: everything
in front of the writer is the same device code on both sides.  With the writer off the engine is the engine it was."""
import ctypes as C

import numpy as np
import pytest

import output_writer_oracle as O
import signals as S

pytestmark = pytest.mark.gpu

STREAMS = 70
CALLS = (480, 960, 1440, 480, 720, 1000, 480, 1440, 960, 481, 1200, 480)
DB_TOL = 1e-4  # 20 log10f of bit-equal values, device log10f against glibc's: see tests/test_gpu_output_writer.py


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def core():
    from mic_eq_mi import mic_eq_core

    return mic_eq_core


@pytest.fixture(scope="module")
def audio():
    x = S.batch_signal(STREAMS, 22).astype(np.float32)
    assert x.shape[1] >= sum(CALLS)
    x[3::7] *= np.float32(6.0)  # streams that drive the chain's limiter hard: true peaks at the writer's ceiling
    return x


def _engine(core, output_rate):
    eng = core.Engine(48_000.0, STREAMS)
    core.configure_auto_eq_chain(eng, 48_000.0, S.LIMITER_BANDS, S.limiter_settings(2.0))  # the dynamics chain
    eng.set_limiter_enabled(1)
    eng.set_prefilter_enabled(1, 1)  # the front end: DC block + 80 Hz high-pass
    if output_rate:
        eng.set_io_sample_rates(0, output_rate)
    return eng


def _fills(k, lim):
    s = np.arange(STREAMS, dtype=np.int64)
    f = (lim["center"] - 900 + (k * 131 + s * 53) % (lim["hard"] + 600)).clip(0, lim["capacity"])  # drifts through every zone
    f[5::16] = lim["capacity"] - 100 - s[5::16]      # nearly full queues: short writes, then fades
    f[9::32] = lim["capacity"] if k % 3 == 0 else lim["center"]
    return f


@pytest.mark.parametrize("output_rate", (0, 44_100), ids=("engine-rate", "44k1-output"))
def test_engine_with_writer_equals_engine_plus_restatement(core, audio, output_rate):
    a, b = _engine(core, output_rate), _engine(core, output_rate)
    a.set_output_writer(True)
    rate = output_rate or 48_000
    lim = O.default_limits(rate)
    ref = O.Batch(STREAMS, rate=float(rate))
    powf = C.CDLL("libm.so.6").powf
    powf.restype, powf.argtypes = C.c_float, [C.c_float, C.c_float]
    ceiling = powf(10.0, float(np.float32(np.float32(a.limiter_ceiling_db()) / np.float32(20.0))))  # dsp_loop.rs:535
    ref.set_limiter(True, ceiling)
    at, seen = 0, set()
    for k, n in enumerate(CALLS):
        fill = _fills(k, lim)
        if k > 0:  # the first call runs on the default: the target centre
            a.set_output_queue_fill(fill)
        else:
            fill = np.full(STREAMS, lim["center"], dtype=np.int64)
        plan_a, plan_b = a.stream_plan(n), b.stream_plan(n)
        assert plan_a[:2] == plan_b[:2]
        got = a.stream(audio[:, at:at + n])
        plain = b.stream(audio[:, at:at + n])
        at += n
        assert plain.shape[1] == plan_b[2]
        if plain.shape[1] == 0:
            assert got.shape[1] == 0 and not a.output_written().any()
            continue
        assert plan_a[2] == max(max(O.retime(np.zeros(plain.shape[1], dtype=np.float32), 0.96, lim["capacity"]).size,
                                    plain.shape[1]), 1)
        want = ref.push(plain, fill)
        written = a.output_written()
        assert np.array_equal(written, [r.size for r in want]), k
        assert got.shape[1] == written.max()
        for s, r in enumerate(want):
            bad = np.flatnonzero(bits(got[s, :r.size]) != bits(r))
            assert bad.size == 0, (k, n, s, bad[:4].tolist())
            assert not got[s, r.size:].any(), (k, s)
        counters, meters = a.output_counters(), a.output_meters()
        wc, wm = ref.counters(), ref.meters()
        for key in O.COUNTERS:
            assert np.array_equal(counters[key], wc[key]), (k, key)
        for key in O.LINEAR + ("ratio", "ema"):
            assert np.array_equal(bits(meters[key]), bits(wm[key])), (k, key)
        for key in ("out_len", "fade_remaining", "fill_after"):
            assert np.array_equal(meters[key], wm[key]), (k, key)
        for key in O.DB:
            assert np.abs(meters[key].astype(np.float64) - wm[key].astype(np.float64)).max() <= DB_TOL, (k, key)
        seen |= set(np.sign(wm["out_len"] - plain.shape[1]).tolist())
    assert seen == {-1, 0, 1}  # expanded, passed through and compressed rows all occurred
    assert ref.counters()["recovery_events"].any() and (ref.meters()["fade_remaining"] >= 0).all()
    with pytest.raises(RuntimeError):  # a configuration setter: AF_ERR_STATE after streaming has started
        a.set_output_writer(False)
    with pytest.raises(NotImplementedError, match="af_engine_stream_host"):
        a.process(np.zeros((480, STREAMS), dtype=np.float32), layout=1)
    with pytest.raises(ValueError):  # more than the writer takes per block: refused, nothing touched
        a.stream(np.zeros((STREAMS, 9000), dtype=np.float32))
    before = a.output_counters()
    a.reset()  # a fresh writer, the fill evidence dropped
    assert not any(v.any() for v in a.output_counters().values()) and any(v.any() for v in before.values())
    a.close()
    b.close()


@pytest.mark.parametrize("output_rate", (0, 44_100), ids=("engine-rate", "44k1-output"))
def test_writer_off_is_the_route_it_was(core, audio, output_rate):
    a, b = _engine(core, output_rate), _engine(core, output_rate)
    a.set_output_writer(False)
    at = 0
    for n in CALLS[:5]:
        assert a.stream_plan(n) == b.stream_plan(n)
        got, want = a.stream(audio[:, at:at + n]), b.stream(audio[:, at:at + n])
        at += n
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    with pytest.raises(RuntimeError):
        a.output_written()
    a.close()
    b.close()
