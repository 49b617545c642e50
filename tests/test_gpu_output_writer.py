"""The batched output writer (af_output_writer.hip) against the restatement of the reference's write_chunk
(tests/ref/output_writer_ref.c), push by push on the shared stimulus: audio rows, lengths, decisions, counters, linear
statistics and the limiter / detector state to the bit, the dB fields to 1e-4 dB (20 log10f of bit-equal values: the
device's log10f and glibc's differ by a few f32 ulp, and an ulp near 120 dB is 7.6e-6)."""
import ctypes as C

import numpy as np
import pytest

import output_writer_oracle as O
import output_writer_stimulus as stim

pytestmark = pytest.mark.gpu
DB_TOL = 1e-4
BIT_METERS = O.LINEAR + ("ratio", "ema", "out_len", "fade_remaining", "fill_after")
_REFERENCE = {}


def _writer(core, name):
    lim = stim.limits(name)
    return core.OutputWriter(lim["rate"], stim.N_STREAMS, 0, lim["capacity"], lim["center"], lim["hard"], lim["fade"])


def _reference(name):
    if name not in _REFERENCE:
        lim = stim.limits(name)
        _REFERENCE[name] = O.run_sequence(stim.sequence(name), stim.N_STREAMS, rate=float(lim["rate"]), capacity=lim["capacity"],
                                          center=lim["center"], hard=lim["hard"], fade=lim["fade"])
    return _REFERENCE[name]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _compare(w, rows, written, step, tag):
    want_written = np.asarray([r.size for r in step["rows"]], dtype=np.int64)
    _same_bits(written, want_written, (tag, "written"))
    for s, r in enumerate(step["rows"]):
        _same_bits(rows[s, :r.size], r, (tag, "audio", s))
        assert not rows[s, r.size:].any(), (tag, "row tail", s)
    counters, meters, state = w.counters(), w.meters(), w.state()
    for k in O.COUNTERS:
        _same_bits(counters[k], step["counters"][k], (tag, k))
    for k in BIT_METERS:
        _same_bits(meters[k], step["meters"][k], (tag, k))
    for k in O.DB:
        err = np.abs(meters[k].astype(np.float64) - step["meters"][k].astype(np.float64))
        assert err.max() <= DB_TOL, (tag, k, int(err.argmax()), float(err.max()))
    for k in ("gain", "delay", "write_idx", "histories"):
        _same_bits(state[k], step["state"][k], (tag, k))


@pytest.fixture(scope="module")
def core():
    from mic_eq_mi import mic_eq_core

    return mic_eq_core


@pytest.mark.parametrize("name", list(stim.CONFIGS))
def test_every_push_equals_the_restatement(core, name):
    w = _writer(core, name)
    for k, (push, step) in enumerate(zip(stim.sequence(name), _reference(name))):
        stim.apply_pre(w, push["pre"])
        rows, written = w.push(push["x"], push["fill"], push["clean_path"])
        _compare(w, rows, written, step, (name, k, push["x"].shape[1]))
    w.close()


def test_timing_read_outs_around_a_reset(core):
    name = "derived_48k"
    push, step = stim.sequence(name)[0], _reference(name)[0]
    w = _writer(core, name)
    assert w.last_kernel_ms() == 0.0 and list(w.last_pass_ms()) == [0.0] * 5  # nothing pushed yet
    for label in ("first push", "after reset"):
        stim.apply_pre(w, push["pre"])
        rows, written = w.push(push["x"], push["fill"], push["clean_path"])
        _compare(w, rows, written, step, (name, label))
        total, passes = w.last_kernel_ms(), list(w.last_pass_ms())
        assert len(passes) == 5 and all(np.isfinite(t) and t >= 0.0 for t in passes + [total]), (label, total, passes)
        w.reset()
    w.close()


def test_fresh_writer_reads_the_initial_fields(core):
    w = _writer(core, "derived_48k")
    m, c = w.meters(), w.counters()
    assert all((c[k] == 0).all() for k in O.COUNTERS)
    assert (m["clip_peak_db"] == -120).all() and (m["true_peak_db"] == -120).all() and (m["true_peak_input_db"] == -120).all()
    assert (m["headroom_db"] == 120).all() and (m["gain_reduction_db"] == 0).all() and (m["ratio"] == 1).all()
    assert (w.state()["gain"] == 1).all()
    w.close()


def test_push_device_with_strides_on_a_side_stream_equals_push_host(core):
    import torch

    name = "limits_128_256_4"
    pushes = stim.sequence(name)[6:10]
    host, dev = _writer(core, name), _writer(core, name)
    side = torch.cuda.Stream()
    B = stim.N_STREAMS
    for k, push in enumerate(pushes):
        stim.apply_pre(host, push["pre"])
        stim.apply_pre(dev, push["pre"])
        rows, written = host.push(push["x"], push["fill"], push["clean_path"])
        n = push["x"].shape[1]
        width = dev.max_output_frames(n)
        in_stride, out_stride = n + 5, width + 9
        x = torch.full((B, in_stride), 7.0, dtype=torch.float32, device="cuda")
        x[:, :n] = torch.from_numpy(push["x"]).cuda()
        fill = torch.from_numpy(push["fill"]).cuda()
        canary = np.float32(-12345.0)
        out = torch.full((B + 1, out_stride), float(canary), dtype=torch.float32, device="cuda")
        wr = torch.full((B + 1,), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            dev.push_device(x.data_ptr(), n, in_stride, fill.data_ptr(), push["clean_path"], out.data_ptr(), width, out_stride,
                            wr.data_ptr(), side.cuda_stream)
        side.synchronize()
        got, got_written = out.cpu().numpy(), wr.cpu().numpy()
        _same_bits(got_written[:B], written, (k, "written"))
        assert got_written[B] == -7
        for s in range(B):
            _same_bits(got[s, :written[s]], rows[s, :written[s]], (k, "audio", s))
            assert (got[s, written[s]:] == canary).all(), (k, "untouched tail", s)
        assert (got[B] == canary).all()
        hm, dm = host.meters(), dev.meters()
        for key in BIT_METERS + O.DB:
            _same_bits(dm[key], hm[key], (k, key))
        hs, ds = host.state(), dev.state()
        for key in hs:
            _same_bits(ds[key], hs[key], (k, key))
    host.close()
    dev.close()


def test_a_refused_call_changes_nothing(core):
    name = "limits_128_256_4"
    lim = stim.limits(name)
    w = _writer(core, name)
    push = stim.sequence(name)[0]
    w.push(push["x"], push["fill"])
    before = (w.counters(), w.meters(), w.state())
    lib, h, B = w._lib, w._h, stim.N_STREAMS
    fp, lp = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    x = np.full((B, 8193), 0.5, dtype=np.float32)
    out = np.full((B, 9000), 3.0, dtype=np.float32)
    written = np.full(B, -1, dtype=np.int64)
    fill = np.zeros(B, dtype=np.int64)

    def call(n, in_stride, f, cap, stride):
        return lib.af_output_writer_push_host(h, x.ctypes.data_as(fp), n, in_stride, f.ctypes.data_as(lp), 0, out.ctypes.data_as(fp),
                                              cap, stride, written.ctypes.data_as(lp))

    need = w.max_output_frames(480)
    bad_fill = fill.copy()
    bad_fill[B - 1] = lim["capacity"] + 1
    assert call(8193, 8193, fill, 9000, 9000) == -1            # too long a block
    assert call(480, 8193, fill, need - 1, 9000) == -1         # capacity one too small
    assert call(480, 8193, fill, 9000, need - 1) == -1         # stride one too small
    assert call(480, 8193, bad_fill, 9000, 9000) == -1         # a fill beyond the queue
    assert (out == 3.0).all() and (written == -1).all()
    after = (w.counters(), w.meters(), w.state())
    for b, a in zip(before, after):
        for key in b:
            _same_bits(a[key], b[key], key)
    # and the next push is what it would have been
    ref = O.Batch(B, rate=float(lim["rate"]), capacity=lim["capacity"], center=lim["center"], hard=lim["hard"], fade=lim["fade"])
    ref.push(push["x"], push["fill"])
    nxt = stim.sequence(name)[1]
    want = ref.push(nxt["x"], nxt["fill"])
    rows, wr = w.push(nxt["x"], nxt["fill"])
    for s, r in enumerate(want):
        assert wr[s] == r.size
        _same_bits(rows[s, :r.size], r, ("after refusal", s))
    w.close()
