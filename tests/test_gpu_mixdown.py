"""The mixdown kernels against the CPU restatement (tests/ref/mixdown_ref.c), bit for bit: the 67-stream stimulus batch of
tests/mixdown_stimulus.py pushed callback by callback through Mixdown.push, in every mode, for 1, 2, 3 and 6 channels.
After every callback the mono output of all 67 streams and every diagnostic must equal the restatement's as bit patterns.
No tolerance: every quantity is one IEEE f32 operation in the reference's order on both sides."""
import numpy as np
import pytest

import mixdown_oracle as MO
import mixdown_stimulus as S

pytestmark = pytest.mark.gpu

MODES = (MO.AVERAGE, MO.LEFT, MO.RIGHT, MO.MAX_RMS, MO.PHASE_SAFE_MONO)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same_diagnostics(got, want, where):
    for key in ("stereo_correlation", "estimated_delay"):
        bad = np.flatnonzero(bits(got[key]) != bits(want[key]))
        assert bad.size == 0, (where, key, bad[:8], got[key][bad[:8]], want[key][bad[:8]])
    for key in ("strategy", "phase_warning_count", "polarity_flipped"):
        bad = np.flatnonzero(np.asarray(got[key]).astype(np.int64) != np.asarray(want[key]).astype(np.int64))
        assert bad.size == 0, (where, key, bad[:8], np.asarray(got[key])[bad[:8]], np.asarray(want[key])[bad[:8]])


def assert_same_output(got, want, where):
    assert got.shape == want.shape, (where, got.shape, want.shape)
    bad = np.argwhere(bits(got) != bits(want))
    assert bad.size == 0, (where, len(bad), "streams", sorted(set(bad[:, 0].tolist()))[:10], "first", bad[0].tolist(),
                           got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.fixture(scope="module")
def core():
    from mic_eq_mi import mic_eq_core

    return mic_eq_core


@pytest.mark.parametrize("mode", MODES, ids=MO.MODE_IDS)
@pytest.mark.parametrize("channels", (2, 1, 3, 6))
def test_every_callback_equals_the_restatement(core, channels, mode):
    outs, diags, _ = S.reference(channels, mode)
    m = core.Mixdown(channels, MO.MODE_IDS[mode], n_streams=S.N_STREAMS)
    for i, cb in enumerate(S.callbacks(S.material(channels))):
        where = f"channels {channels} mode {MO.MODE_IDS[mode]} callback {i} ({cb.shape[1]} frames)"
        assert_same_output(m.push(cb), outs[i], where)
        assert_same_diagnostics(m.diagnostics(), diags[i], where)
    m.close()


def test_mode_change_keeps_history_and_candidate_and_reset_clears_them(core):
    """phase-safe -> average -> phase-safe between callbacks: the state object outlives the mode (input.rs:780); then
    reset gives what a fresh object gives."""
    cbs = S.callbacks()
    plan = {5: MO.AVERAGE, 6: MO.PHASE_SAFE_MONO, 8: MO.MAX_RMS, 9: MO.PHASE_SAFE_MONO, 10: MO.AVERAGE, 11: MO.PHASE_SAFE_MONO}
    ref = MO.Batch(2, MO.PHASE_SAFE_MONO, S.N_STREAMS)
    m = core.Mixdown(2, "phase_safe_mono", n_streams=S.N_STREAMS)
    for i, cb in enumerate(cbs):
        if i in plan:
            ref.set_mode(plan[i])
            m.set_mode(MO.MODE_IDS[plan[i]])
        where = f"callback {i} mode {m.mode}"
        assert_same_output(m.push(cb), ref.push(cb), where)
        assert_same_diagnostics(m.diagnostics(), ref.diagnostics(), where)
    # the 2-frame callback right after a mode round trip reused stored candidates: the state survived
    assert sum(c["hysteresis_reused"] for c in ref.counters()) > 0
    m.reset()
    d = m.diagnostics()
    assert np.isnan(d["stereo_correlation"]).all() and not d["phase_warning_count"].any() and not d["strategy"].any()
    outs, diags, _ = S.reference(2, MO.PHASE_SAFE_MONO)
    for i, cb in enumerate(cbs[:7]):
        assert_same_output(m.push(cb), outs[i], f"after reset, callback {i}")
        assert_same_diagnostics(m.diagnostics(), diags[i], f"after reset, callback {i}")
    m.close()


def test_push_device_with_strides_equals_push(core):
    import torch

    outs, diags, _ = S.reference(2, MO.PHASE_SAFE_MONO)
    m = core.Mixdown(2, "phase_safe_mono", n_streams=S.N_STREAMS)
    for i, cb in enumerate(S.callbacks()[:9]):
        n = cb.shape[1]
        in_stride, out_stride = n + 3, n + 5
        x = torch.full((S.N_STREAMS, in_stride, 2), 7.0, dtype=torch.float32, device="cuda")
        x[:, :n] = torch.from_numpy(np.ascontiguousarray(cb)).cuda()
        y = torch.full((S.N_STREAMS, out_stride), -9.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        m.push_device(x.data_ptr(), n, in_stride, y.data_ptr(), out_stride)
        got = y.cpu().numpy()  # (waits for the default stream)
        assert_same_output(got[:, :n], outs[i], f"push_device callback {i}")
        assert (got[:, n:] == -9.0).all(), "frames past n_frames were written"
        assert_same_diagnostics(m.diagnostics(), diags[i], f"push_device callback {i}")
    dec_ms, mix_ms = m.last_kernel_ms()
    assert dec_ms > 0.0 and mix_ms > 0.0
    m.close()


def test_timing_read_outs_around_a_reset(core):
    outs, diags, _ = S.reference(2, MO.PHASE_SAFE_MONO)
    cb = S.callbacks()[0]
    m = core.Mixdown(2, "phase_safe_mono", n_streams=S.N_STREAMS)
    assert m.last_kernel_ms() == (0.0, 0.0)  # nothing pushed yet
    for label in ("first push", "after reset"):
        assert_same_output(m.push(cb), outs[0], label)
        assert_same_diagnostics(m.diagnostics(), diags[0], label)
        for ms in m.last_kernel_ms():
            assert np.isfinite(ms) and ms >= 0.0, (label, ms)
        m.reset()
    m.close()


def test_non_finite_host_sample_refuses_the_call_and_touches_nothing(core):
    outs, diags, _ = S.reference(2, MO.PHASE_SAFE_MONO)
    cbs = S.callbacks()
    m = core.Mixdown(2, "phase_safe_mono", n_streams=S.N_STREAMS)
    for i in range(7):
        m.push(cbs[i])
    bad = np.array(cbs[7])
    bad[66, 479, 1] = np.nan
    with pytest.raises(ValueError, match="samples must be finite"):
        m.push(bad)
    assert_same_diagnostics(m.diagnostics(), diags[6], "after the refused call")
    assert_same_output(m.push(cbs[7]), outs[7], "the callback after the refused call")
    assert_same_diagnostics(m.diagnostics(), diags[7], "the callback after the refused call")
    m.close()
