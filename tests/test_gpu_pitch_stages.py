"""The suppressor's pitch path on the GPU -- supp_pitchsearch4_kernel and the remove_doubling half of supp_pitch_kernel --
per (frame, stream) cell against the float64 reference of tests/pitch_stage_ref.py.

Three taps feed it (host side only; the kernels are untouched): af_suppressor_debug_read_pitch (the whitened buffer of a cell
of the last window, and a stream's last_period / last_gain), af_suppressor_debug_pitch_search (the search kernel ALONE on
caller-supplied spans: its own pitch index, which the tracker overwrites in an engine run) and the existing record tap.
The stimulus (tests/pitch_stage_stimulus.py) is 69 streams x 43 frames in calls of 1, 1, 1, 2, 3, 4, 5, 1, 7, 16, 1, 1 frames,
31 streams read; the search alone also runs on five synthetic spans at 1, 3, 4 and 6 frames.  tests/test_pitch_stage_ref.py
proves on the CPU that the stimulus reaches every edge and that the reference agrees with the restatement.

Magnitudes (whitened buffer: max |d| / buffer peak; last_gain: absolute) are held to 4 x the restatement's own worst distance
from f64 on the same cells in evaluation order 0, never under 4 f32 epsilons.  Integer decisions must equal the f64 result
computed from the DEVICE's own whitened buffer, or be reachable by the tolerant replay (every comparison whose sides differ
by less than tau x max(|lhs|, |rhs|) may go either way; tau = 4 x the restatement's worst relative operand distance): an
excused cell.  Per stage at most 1 % of the cells may be excused -- a condition, not a measurement.  Every run prints the
figures (pytest -s); DESIGN.md 4.5 holds the table and what four mutated builds did.

Measured on an MI355X (device | restatement, order 0 | bound): whitened buffer 5.5e-4 | 5.5e-4 | 2.2e-3 of the buffer peak over
1333 engine cells and the stand-alone search's; last_gain 1.9e-7 | 1.9e-7 | 7.8e-7 over 372 call ends; tau 2.2e-6; excused 0 of
1403 search cells and 0 of 1333 tracker cells; the engine's whitened buffers bit for bit the stand-alone search's.  Mutated
builds (never committed): the decimation's first-sample case dropped fails the buffer test (0.70), one second_check entry
changed fails the tracker test through last_gain (0.054), `cont` against the undivided last period fails it through
unreachable indices, last_gain not stored fails it (0.999) and the window split.
"""
import ctypes as C
import os

import numpy as np
import pytest

import pitch_stage_ref as P
import pitch_stage_stimulus as T

pytestmark = pytest.mark.gpu

SCHEDULE_SWITCHES = ("AF_SUPP_WINDOW_FRAMES", "AF_SUPP_RAMP", "AF_SUPP_RAMP_LIST", "AF_SUPP_RAMP_END")
DEVICE_CAP = 0.01


def _engine(mi, n_streams: int):
    eng = mi.Engine(48_000.0, n_streams)
    eng.set_eq_enabled(0)
    eng.set_limiter_enabled(0)
    eng.set_suppressor_enabled(1)
    eng.set_control_block_samples(480)
    eng.suppressor_set_raw_protocol(1)
    eng.suppressor_set_trace_enabled(1)
    return eng


def _engine_run() -> dict:
    """The stimulus through an engine in the twelve one-window calls; every read stream's taps after every call."""
    import mic_eq_mi

    assert mic_eq_mi.CORE_AVAILABLE
    audio = T.batch()
    streams = list(T.READ_STREAMS)
    assert np.array_equal(audio[streams], T.read_audio())
    eng = _engine(mic_eq_mi, audio.shape[0])
    ds, final, silence, outs, traces, end_period, end_gain, f0 = [], [], [], [], [], [], [], 0
    try:
        for call, n in enumerate(T.CALLS):
            out = eng.process(audio[:, f0 * 480:(f0 + n) * 480])
            assert out.shape == (audio.shape[0], n * 480)
            trace = eng.suppressor_trace()
            assert trace.shape == (n, audio.shape[0], 2)
            for f in range(n):
                rec = [eng.suppressor_debug_read(f, s) for s in streams]
                for cell, s in zip(rec, streams):  # a stale cell (an earlier window's) would differ from the call's trace
                    assert (cell["silence"], cell["pitch_index"]) == tuple(trace[f, s]), ("stale tap cell", call, f, s)
                ds.append([eng.suppressor_debug_read_pitch(f, s)["whitened"] for s in streams])
                final.append([c["pitch_index"] for c in rec])
                silence.append([c["silence"] for c in rec])
            state = [eng.suppressor_debug_read_pitch(None, s) for s in streams]
            end_period.append([c["last_period"] for c in state])
            end_gain.append([c["last_gain"] for c in state])
            outs.append(out)
            traces.append(trace)
            f0 += n
    finally:
        eng.close()
    return {"ds": np.array(ds), "final": np.array(final, dtype=np.int64), "silence": np.array(silence), "end_period": np.array(end_period),
            "end_gain": np.array(end_gain, dtype=np.float32), "out": np.concatenate(outs, axis=1), "trace": np.concatenate(traces, axis=0),
            "audio": audio}


def _search_run() -> dict:
    """The search kernel alone: the synthetic spans at every frame count, and the read streams' model-input spans at once
    (43 frames: ten full four-frame workgroups and one with three live waves, per stream)."""
    import mic_eq_mi

    run = {}
    for key in (*T.SEARCH_FRAMES, "stimulus"):
        spans = T.model_spans() if key == "stimulus" else T.search_spans(key)
        ds, index = mic_eq_mi.Engine.suppressor_debug_pitch_search(spans)
        assert ds.shape == (T.N_FRAMES if key == "stimulus" else key, spans.shape[0], 864) and index.shape == ds.shape[:2]
        run[key] = {"spans": spans, "ds": ds, "index": index.astype(np.int64)}
    return run


_CACHE: dict = {}


@pytest.fixture(scope="module")
def device():
    saved = {k: os.environ.pop(k) for k in SCHEDULE_SWITCHES if k in os.environ}

    def get(kind: str) -> dict:
        if kind not in _CACHE:
            _CACHE[kind] = _engine_run() if kind == "engine" else _search_run()
        return _CACHE[kind]

    try:
        yield get
    finally:
        os.environ.update(saved)
        _CACHE.clear()


def _where(f: int, s: int) -> tuple:
    ends = np.cumsum(T.CALLS)
    call = int(np.searchsorted(ends, f, side="right"))
    return call, f - (int(ends[call - 1]) if call else 0), T.READ_STREAMS[s]


def _zero_columns() -> list:
    return [i for i, s in enumerate(T.READ_STREAMS) if T.ROLES.get(s) == "zeros"]


def test_whitened_buffer(device):
    """The device's whitened buffer against f64 pitch_downsample of the f32-restated model input with its carried history,
    in the engine (every read cell of the twelve calls) and in the stand-alone search; all-zero cells exactly zero."""
    ref = T.restatement(0)
    eng, alone = device("engine"), device("search")
    err = P.check_buffers(eng["ds"], T.model_spans())
    f, s = (int(v) for v in np.unravel_index(int(np.argmax(err)), err.shape))
    print(f"whitened buffer, engine: device {err.max():.3e} (call, frame, stream {_where(f, s)}) | restatement "
          f"{ref['engine']['buffer_err'].max():.3e} | bound {ref['buffer_bound']:.3e} | {err.size} cells")
    assert np.all(np.isfinite(eng["ds"])) and err.max() <= ref["buffer_bound"], (err.max(), _where(f, s))
    zero = _zero_columns()
    assert len(zero) == 2 and not np.any(eng["ds"][:, zero].view(np.uint32) & 0x7FFFFFFF)  # not even a negative zero
    assert all(np.any(eng["ds"][5, i] != 0) for i in range(len(T.READ_STREAMS)) if i not in zero)
    worst = 0.0
    for key, part in alone.items():
        e = P.check_buffers(part["ds"], part["spans"])
        worst = max(worst, float(e.max()))
        assert np.all(np.isfinite(part["ds"])) and e.max() <= ref["buffer_bound"], (key, e.max(), np.unravel_index(int(np.argmax(e)), e.shape))
        if key != "stimulus":
            assert not np.any(part["ds"][:, 0].view(np.uint32) & 0x7FFFFFFF)
    print(f"whitened buffer, search alone: device {worst:.3e} | restatement {ref['buffer_worst']:.3e} | bound {ref['buffer_bound']:.3e}")
    # the engine's search is the stand-alone one: same kernel, same launcher, same input -> the same bits
    assert np.array_equal(eng["ds"].view(np.uint32), alone["stimulus"]["ds"].view(np.uint32))


def test_search_alone(device):
    """The search's own index against the f64 search of the device's own whitened buffer: equal, or excused by the replay."""
    ref = T.restatement(0)
    alone = device("search")
    status = []
    for key, part in alone.items():
        check = P.check_search(part["ds"], part["index"], ref["tau"])
        bad = np.argwhere(check["status"] == 2)
        assert bad.size == 0, (key, [(int(f), int(s), int(part["index"][f, s]), P.pitch_search(part["ds"][f, s])[0]) for f, s in bad[:8]])
        status.append(check["status"].ravel())
        if key != "stimulus":  # the edges the spans were built for, as the device saw them
            assert np.all(part["index"][:, :2] == 768)
            assert np.all(part["index"][:, T.SEARCH_STREAMS.index("lag146")] == 182)
    status = np.concatenate(status)
    print(f"search alone: {int(np.sum(status == 1))} excused of {status.size} cells (cap {DEVICE_CAP:.0%}), tau {ref['tau']:.3e}")
    assert status.size == sum(T.SEARCH_FRAMES) * len(T.SEARCH_STREAMS) + T.N_FRAMES * len(T.READ_STREAMS)
    assert P.excused_share(status) <= DEVICE_CAP


def test_tracker_in_the_engine(device):
    """remove_doubling in f64 from the device's whitened buffer, the f64 search of it, the device's previous final index and
    a gain carried in f64 and re-synchronised to the device's last_gain at every call end: the final index equal or
    excused, last_gain within its bound and last_period the last frame's index at all twelve call ends."""
    ref = T.restatement(0)
    eng = device("engine")
    check = P.check_tracker(eng["ds"], eng["final"], T.CALLS, eng["end_period"], eng["end_gain"], ref["tau"])
    status = check["status"]
    bad = np.argwhere(status == 2)
    assert bad.size == 0, [(_where(int(f), int(s)), int(eng["final"][f, s]), check["info"][(int(f), int(s))]["T"]) for f, s in bad[:8]]
    gain = check["gain_error"]
    c, s = (int(v) for v in np.unravel_index(int(np.argmax(gain)), gain.shape))
    print(f"tracker: {int(np.sum(status == 1))} excused of {status.size} cells (cap {DEVICE_CAP:.0%}) | last_gain: device "
          f"{gain.max():.3e} (call {c}, stream {T.READ_STREAMS[s]}) | restatement {ref['gain_worst']:.3e} | bound {ref['gain_bound']:.3e} "
          f"| {gain.size} call ends")
    assert status.shape == (T.N_FRAMES, len(T.READ_STREAMS)) and P.excused_share(status) <= DEVICE_CAP
    assert np.all((eng["end_gain"] >= 0.0) & (eng["end_gain"] <= 1.0))
    assert gain.max() <= ref["gain_bound"], (gain.max(), c, T.READ_STREAMS[s])
    assert check["period_wrong"] == []
    assert np.array_equal(eng["end_period"], eng["final"][np.cumsum(T.CALLS) - 1])
    # the edges, as the device saw them: both clamps and a removed doubling
    assert int(eng["final"].min()) == 60 and int(eng["final"].max()) >= 760
    assert np.all(eng["silence"][:, _zero_columns()] != 0) and not np.all(eng["silence"] != 0)  # silent cells are compared like any other


def test_window_split(device):
    """The same audio through a second engine in calls of several windows (43 frames at once: windows of 16, 16 and 11; and
    20 + 23 frames): the (silence, pitch) trace and the audio bit for bit those of the one-window calls.  The whitened
    buffers are a single set that only stream order protects from the next window's search."""
    import mic_eq_mi

    eng = device("engine")
    audio = eng["audio"]
    for calls in ((T.N_FRAMES,), (20, 23)):
        other = _engine(mic_eq_mi, audio.shape[0])
        try:
            outs, traces, f0 = [], [], 0
            for n in calls:
                outs.append(other.process(audio[:, f0 * 480:(f0 + n) * 480]))
                traces.append(other.suppressor_trace())
                f0 += n
        finally:
            other.close()
        assert np.array_equal(np.concatenate(traces, axis=0), eng["trace"]), calls
        assert np.array_equal(np.concatenate(outs, axis=1).view(np.uint32), eng["out"].view(np.uint32)), calls


def test_refusals(device):
    """A refused or out-of-range tap call returns the existing error codes and writes nothing."""
    import mic_eq_mi
    from mic_eq_mi import _lib

    lib = _lib.load()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    sentinel = np.float32(-7.25)
    buf = np.full(864, sentinel, dtype=np.float32)
    period, gain = C.c_int32(-5), C.c_float(-7.25)

    def untouched() -> bool:
        return bool(np.all(buf == sentinel)) and period.value == -5 and gain.value == -7.25

    eng = _engine(mic_eq_mi, 3)
    try:
        h = eng._h
        assert lib.af_suppressor_debug_read_pitch(h, 0, 0, buf.ctypes.data_as(fp), C.byref(period), C.byref(gain)) == _lib.AF_ERR_STATE
        assert lib.af_suppressor_debug_read_pitch(None, 0, 0, buf.ctypes.data_as(fp), C.byref(period), C.byref(gain)) == _lib.AF_ERR_STATE
        assert untouched()
        with pytest.raises(RuntimeError):
            eng.suppressor_debug_read_pitch(0, 0)
        audio = T.read_audio()[:3, :2 * 480]
        eng.process(audio)
        before = [eng.suppressor_debug_read_pitch(1, s) for s in range(3)]
        for frame, stream in ((-1, 0), (2, 0), (0, -1), (0, 3), (1 << 20, 0), (0, 1 << 20)):
            rc = lib.af_suppressor_debug_read_pitch(h, frame, stream, buf.ctypes.data_as(fp), C.byref(period), C.byref(gain))
            assert rc == _lib.AF_ERR_INVALID_ARGUMENT and untouched(), (frame, stream)
        with pytest.raises(ValueError):
            eng.suppressor_debug_read_pitch(0, 3)
        # without a buffer the frame is not looked at; the state read alone works
        assert lib.af_suppressor_debug_read_pitch(h, -1, 2, None, C.byref(period), None) == _lib.AF_OK
        assert period.value == before[2]["last_period"] and gain.value == -7.25
        after = [eng.suppressor_debug_read_pitch(1, s) for s in range(3)]
        for a, b in zip(before, after):
            assert np.array_equal(a["whitened"], b["whitened"]) and (a["last_period"], a["last_gain"]) == (b["last_period"], b["last_gain"])
        out2 = eng.process(audio)  # and the engine goes on as if nothing had been asked
        assert out2.shape == audio.shape and np.all(np.isfinite(out2))
    finally:
        eng.close()
    spans = T.search_spans(1)
    ds = np.full((1, 5, 864), sentinel, dtype=np.float32)
    idx = np.full((1, 5), -5, dtype=np.int32)
    args = (spans.ctypes.data_as(fp), 5, 1, ds.ctypes.data_as(fp), idx.ctypes.data_as(ip), 0)
    for bad in ((None, 5, 1, args[3], args[4], 0), (args[0], 5, 1, None, args[4], 0), (args[0], 5, 1, args[3], None, 0),
                (args[0], 0, 1, args[3], args[4], 0), (args[0], 4097, 1, args[3], args[4], 0), (args[0], 5, 0, args[3], args[4], 0),
                (args[0], 5, 65, args[3], args[4], 0), (args[0], -1, -1, args[3], args[4], 0)):
        assert lib.af_suppressor_debug_pitch_search(*bad) == _lib.AF_ERR_INVALID_ARGUMENT
        assert np.all(ds == sentinel) and np.all(idx == -5)
    with pytest.raises(ValueError):
        mic_eq_mi.Engine.suppressor_debug_pitch_search(np.zeros((2, 1728 + 100), dtype=np.float32))
    assert lib.af_suppressor_debug_pitch_search(*args) == _lib.AF_OK
    assert np.array_equal(ds, device("search")[1]["ds"]) and np.array_equal(idx, device("search")[1]["index"])
