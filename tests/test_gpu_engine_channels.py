"""Multichannel input of the engine: 70 streams of stereo phase-safe input through Engine.stream must equal, bit for bit, a
second engine of the same configuration fed the CPU restatement's mono (tests/ref/mixdown_ref.c) through the mono
Engine.stream.  Everything behind the mixdown is the same device code on both sides, so equality is exact."""
import numpy as np
import pytest

import mixdown_oracle as MO
import mixdown_stimulus as MS
import signals as S

pytestmark = pytest.mark.gpu

STREAMS = 70
CALLBACKS = (480, 3, 1000, 128, 2, 960, 4096)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def core():
    from mic_eq_mi import mic_eq_core

    return mic_eq_core


@pytest.fixture(scope="module")
def stereo():
    """[70, frames, 2]: the stimulus batch's 67 streams and three more of its streams with the channels swapped"""
    n = sum(CALLBACKS)
    x = MS.batch()[:, 1652:1652 + n]  # from inside the 8197-frame call: every family in steady state
    return np.ascontiguousarray(np.concatenate([x, x[[1, 9, 28]][:, :, ::-1]], axis=0))


@pytest.fixture(scope="module")
def restated(stereo):
    """the restatement's mono per callback and its diagnostics after the last one"""
    b = MO.Batch(2, MO.PHASE_SAFE_MONO, STREAMS)
    outs, at = [], 0
    for n in CALLBACKS:
        outs.append(b.push(stereo[:, at:at + n]))
        at += n
    return outs, b.diagnostics()


def _engine(core, input_rate):
    eng = core.Engine(48_000.0, STREAMS)
    core.configure_auto_eq_chain(eng, 48_000.0, S.LIMITER_BANDS, S.limiter_settings(2.0))  # the dynamics chain
    eng.set_prefilter_enabled(1, 1)  # the front end: DC block + 80 Hz high-pass
    if input_rate:
        eng.set_io_sample_rates(input_rate, 0)
    return eng


@pytest.mark.parametrize("input_rate", (0, 44_100), ids=("engine-rate", "44k1-input"))
def test_stereo_phase_safe_input_equals_mono_engine_on_the_restatement(core, stereo, restated, input_rate):
    mono_calls, want_diag = restated
    a, b = _engine(core, input_rate), _engine(core, input_rate)
    a.set_input_channels(2, "phase_safe_mono")
    at = 0
    for i, n in enumerate(CALLBACKS):
        assert a.stream_plan(n) == b.stream_plan(n)
        got = a.stream(stereo[:, at:at + n])
        want = b.stream(mono_calls[i])
        at += n
        assert got.shape == want.shape
        bad = np.argwhere(bits(got) != bits(want))
        assert bad.size == 0, (i, n, len(bad), sorted(set(bad[:, 0].tolist()))[:10])
    d = a.input_phase()
    for key in ("stereo_correlation", "estimated_delay"):
        assert np.array_equal(bits(d[key]), bits(want_diag[key])), key
    for key in ("strategy", "phase_warning_count", "polarity_flipped"):
        assert np.array_equal(np.asarray(d[key]).astype(np.int64), np.asarray(want_diag[key]).astype(np.int64)), key
    assert len(set(d["strategy"].tolist())) >= 3  # the batch exercises the rescue, not just the average
    with pytest.raises(RuntimeError):  # a configuration setter: AF_ERR_STATE after streaming has started
        a.set_input_channels(1, "average")
    a.set_input_channel_mode("average")  # live
    with pytest.raises(NotImplementedError, match="af_engine_stream_host"):
        a.process(np.zeros((stereo.shape[1], STREAMS), dtype=np.float32), layout=1)
    # reset: a fresh mixdown (and fresh everything else): the first callback again gives the first result again
    first = a.stream(stereo[:, :CALLBACKS[0]])
    a.reset()
    b.reset()
    a.set_input_channel_mode("phase_safe_mono")
    again = a.stream(stereo[:, :CALLBACKS[0]])
    want = b.stream(mono_calls[0])
    assert np.array_equal(bits(again), bits(want)) and first.shape == again.shape
    a.close()
    b.close()


def test_one_input_channel_is_an_engine_that_never_called_the_setter(core, restated):
    mono_calls, _ = restated
    a, b = _engine(core, 0), _engine(core, 0)
    a.set_input_channels(1, "phase_safe_mono")
    for x in mono_calls[:3]:
        assert np.array_equal(bits(a.stream(x)), bits(b.stream(x)))
    assert np.array_equal(bits(a.process(mono_calls[3])), bits(b.process(mono_calls[3])))  # process() stays available
    d = a.input_phase()
    assert np.isnan(d["stereo_correlation"]).all() and not d["strategy"].any()
    a.close()
    b.close()
