"""CPU checks of the output writer's boundary: the derived configuration, creation refusals, and push / Python argument
checks that happen before any device work.  No GPU compute is touched here."""
import ctypes as C

import numpy as np
import pytest

import output_writer_oracle as O


@pytest.fixture(scope="module")
def core():
    import mic_eq_mi
    from mic_eq_mi import mic_eq_core

    assert mic_eq_mi.CORE_AVAILABLE
    return mic_eq_core


@pytest.mark.parametrize("rate", [8_000, 44_100, 48_000, 96_000])
def test_default_config_is_the_reference_derivation(core, rate):
    """dsp_loop.rs:781-795, :204; tests.rs:9-13 for 44.1 kHz"""
    cfg = core.output_writer_default_config(rate)
    want = O.default_limits(rate)
    assert cfg == dict(output_rate=rate, queue_capacity=want["capacity"], target_center=want["center"],
                       hard_backlog=want["hard"], fade_frames=want["fade"])
    if rate == 44_100:
        assert (cfg["target_center"], cfg["hard_backlog"]) == ((1323 + 1764 + 1) // 2, 2646)
    with pytest.raises(ValueError, match="output_rate"):
        core.output_writer_default_config(0)


def test_creation_refusals(core):
    for kw in (dict(n_streams=0), dict(n_streams=65_536), dict(device=-1), dict(queue_capacity=0), dict(queue_capacity=2**31),
               dict(target_center=-1), dict(hard_backlog=-1), dict(fade_frames=0), dict(output_rate=0), dict(output_rate=-5)):
        args = dict(output_rate=48_000, n_streams=4, device=0)
        args.update(kw)
        with pytest.raises(ValueError):
            core.OutputWriter(**args)
    lib = core._lib.load()
    assert lib.af_output_writer_create(None, 1, 0, C.byref(C.c_void_p())) == -1
    cfg = core.OutputWriterConfig()
    lib.af_output_writer_default_config(48_000, C.byref(cfg))
    assert lib.af_output_writer_create(C.byref(cfg), 1, 0, None) == -1


def test_max_output_frames(core):
    w = core.OutputWriter(48_000, 3)
    for n in (1, 2, 12, 480, 8191, 8192):
        longest = max(O.retime(np.zeros(n, dtype=np.float32), r, w.config["queue_capacity"]).size for r in (0.96, 1.0, 1.06))
        assert w.max_output_frames(n) == max(longest, n)
    assert w.max_output_frames(0) == 0 and w.max_output_frames(-3) == 0
    small = core.OutputWriter(48_000, 3, queue_capacity=8, target_center=4, hard_backlog=8, fade_frames=4)
    assert small.max_output_frames(480) == 480 and small.max_output_frames(4) == 4  # the clean path yields n_in
    w.close()
    small.close()


def test_push_argument_checks_come_before_any_device_work(core):
    w = core.OutputWriter(48_000, 2)
    lib, h = w._lib, w._h
    fp, lp = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    x = np.zeros((2, 8200), dtype=np.float32)
    out = np.full((2, 9000), 2.0, dtype=np.float32)
    fill, written = np.zeros(2, dtype=np.int64), np.full(2, -1, dtype=np.int64)

    def call(n, in_stride, f, cap, stride, wr=written, src=x, dst=out):
        return lib.af_output_writer_push_host(h, src.ctypes.data_as(fp) if src is not None else None, n, in_stride,
                                              f.ctypes.data_as(lp) if f is not None else None, 0,
                                              dst.ctypes.data_as(fp) if dst is not None else None, cap, stride,
                                              wr.ctypes.data_as(lp) if wr is not None else None)

    need = w.max_output_frames(480)
    assert need == 500
    def refused(message, *args, **kw):
        assert call(*args, **kw) == -1
        assert message in lib.af_last_error(), lib.af_last_error()

    refused(b"at most 8192", 8193, 8200, fill, 9000, 9000)
    refused(b"n_in must be >= 0", -1, 8200, fill, 9000, 9000)
    refused(b"in_stride", 480, 479, fill, 9000, 9000)
    refused(b"out_capacity and out_stride", 480, 8200, fill, need - 1, 9000)
    refused(b"out_capacity and out_stride", 480, 8200, fill, 9000, need - 1)
    refused(b"fill[1] = 96001", 480, 8200, np.asarray([0, 96_001], dtype=np.int64), 9000, 9000)
    refused(b"fill[0] = -1", 480, 8200, np.asarray([-1, 0], dtype=np.int64), 9000, 9000)
    refused(b"null buffer", 480, 8200, None, 9000, 9000)
    refused(b"null buffer", 480, 8200, fill, 9000, 9000, src=None)
    refused(b"null buffer", 480, 8200, fill, 9000, 9000, dst=None)
    refused(b"written is null", 480, 8200, fill, 9000, 9000, wr=None)
    assert (out == 2.0).all() and (written == -1).all()
    assert call(0, 8200, fill, 0, 0) == 0 and (written == 0).all()  # an empty block is a no-op (output_writer.rs:63-65)
    assert lib.af_output_writer_push_host(None, None, 0, 0, None, 0, None, 0, 0, None) == -1
    # nothing ran: the fields are the fresh ones
    assert (w.meters()["headroom_db"] == 120).all() and (w.counters()["recovery_events"] == 0).all()
    w.close()


def test_python_argument_checks(core):
    w = core.OutputWriter(48_000, 2)
    with pytest.raises(ValueError, match="expected"):
        w.push(np.zeros((3, 8), dtype=np.float32), [0, 0])
    with pytest.raises(ValueError, match="fill"):
        w.push(np.zeros((2, 8), dtype=np.float32), [0, 0, 0])
    with pytest.raises(ValueError, match="fill"):
        w.push(np.zeros((2, 8), dtype=np.float32), [0.5, 1.0])
    with pytest.raises(ValueError, match="finite"):
        w.set_limiter(True, float("nan"))
    w.set_limiter(False, 0.5)
    w.reset()
    w.close()


def test_engine_setters_before_start(core):
    """host only: the setter, the plan and the fill's argument checks need no device.  The after-start half (AF_ERR_STATE
    from the setter once streaming has started) is in tests/test_gpu_engine_output_writer.py: starting needs a device."""
    e = core.Engine(48_000.0, 3)
    with pytest.raises(RuntimeError, match="output writer is off"):
        e.set_output_queue_fill([0, 0, 0])
    with pytest.raises(RuntimeError, match="output writer is off"):
        e.output_written()
    with pytest.raises(RuntimeError, match="output writer is off"):
        e.output_counters()
    plain = e.stream_plan(480)
    e.set_output_writer(True)
    assert e.stream_plan(480) == (480, 480, 500) and plain == (480, 480, 480)  # af_output_writer_max_output_frames(480)
    assert e.stream_plan(0)[2] == 0
    e.set_output_queue_fill([0, 96_000, 1680])
    with pytest.raises(ValueError, match="outside the queue"):
        e.set_output_queue_fill([0, 96_001, 0])
    with pytest.raises(ValueError, match="outside the queue"):
        e.set_output_queue_fill([-1, 0, 0])
    with pytest.raises(ValueError, match="fill must be"):
        e.set_output_queue_fill([0, 0])
    with pytest.raises(ValueError, match="fill must be"):
        e.set_output_queue_fill([0.5, 0.0, 1.0])
    assert not e.output_written().any()
    assert not any(v.any() for v in e.output_counters().values()) and (e.output_meters()["headroom_db"] == 120).all()
    with pytest.raises(NotImplementedError, match="af_engine_stream_host"):  # AF_ERR_UNSUPPORTED, before any device work
        e.process(np.zeros((480, 3), dtype=np.float32), layout=1)
    lib = e._lib
    assert lib.af_engine_process_device(e._h, None, None, 480, 480, 0, None) == -5
    # the writer follows the output side's rate (dsp_loop.rs:781-795 at 44.1 kHz: capacity 88200)
    e.set_io_sample_rates(0, 44_100)
    e.set_output_queue_fill([88_200, 0, 0])
    with pytest.raises(ValueError, match="outside the queue"):
        e.set_output_queue_fill([88_201, 0, 0])
    e.set_output_writer(False)  # off again: the plan is the plain one
    e.set_io_sample_rates(0, 0)
    assert e.stream_plan(480) == plain
    e.reset()
    e.close()
    assert lib.af_engine_set_output_writer(None, 1) == -1 and lib.af_engine_read_output_written(None, None, 0) == -1
