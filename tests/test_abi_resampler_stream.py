"""CPU checks of the streaming resampler's boundary: the symbols exist, the argument contract is the reference's and is
enforced without a device, and the engine's stream plan is the host replay the helper predicts.  No GPU is touched."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import resampler_stream_oracle as RS

ROOT = pathlib.Path(__file__).resolve().parents[1]

NEW_SYMBOLS = (
    "af_stream_resampler_create", "af_stream_resampler_destroy", "af_stream_resampler_push_host",
    "af_stream_resampler_push_device", "af_stream_resampler_output_frames", "af_stream_resampler_pending_input",
    "af_stream_resampler_output_delay", "af_stream_resampler_frames_in", "af_stream_resampler_frames_out",
    "af_stream_resampler_reset", "af_stream_resampler_clear_pending", "af_stream_resampler_last_kernel_ms",
    "af_engine_set_io_sample_rates", "af_engine_stream_plan", "af_engine_io_resampler_delay",
    "af_engine_io_resampler_pending",
)


@pytest.fixture(scope="module")
def lib():
    from mic_eq_mi import _lib

    return _lib.load()


def test_new_symbols_are_declared_and_exported(lib):
    from mic_eq_mi import _lib

    header = (ROOT / "include" / "audioforge_mi.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(af_[a-z0-9_]+)\s*\(", header))
    raw = C.CDLL(str(_lib.LIB_PATH))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name


def _create(lib, fi, fo, chunk, sinc_len, window, n_streams):
    from mic_eq_mi import _lib

    h = C.c_void_p()
    rc = lib.af_stream_resampler_create(fi, fo, chunk, sinc_len, window, n_streams, 0, C.byref(h))
    return rc, _lib.last_error(), h


@pytest.mark.parametrize("args,message", [
    ((0, 48_000, 1024, 128, 2, 1), "sample rates must be positive"),
    ((48_000, 0, 1024, 128, 2, 1), "sample rates must be positive"),
    ((48_000, 44_100, 0, 128, 2, 1), "chunk_size must be between 1 and 1024"),
    ((48_000, 44_100, 1025, 128, 2, 1), "chunk_size must be between 1 and 1024"),
    ((48_000, 44_100, 1024, 96, 2, 1), "sinc_len must be a power of two between 32 and 2048"),
    ((48_000, 44_100, 1024, 128, 17, 1), "unsupported resampler window"),
    ((48_000, 44_100, 1024, 128, 2, 0), "n_streams must be positive"),
])
def test_create_refuses_bad_arguments_without_a_device(lib, args, message):
    from mic_eq_mi import _lib

    rc, err, h = _create(lib, *args)
    assert rc == _lib.AF_ERR_INVALID_ARGUMENT and not h.value
    assert message in err


def test_create_limits_and_host_only_values(lib):
    from mic_eq_mi import _lib

    rc, err, h = _create(lib, 48_000, 44_100, 1024, 512, 2, 1)
    assert rc == _lib.AF_ERR_UNSUPPORTED and not h.value
    rc, err, h = _create(lib, 48_000, 8_000, 1024, 128, 2, 1)  # ratio below 0.2
    assert rc == _lib.AF_ERR_UNSUPPORTED and not h.value
    # a good one is built, and its value functions replay the loop, on a machine with no GPU
    rc, err, h = _create(lib, 44_100, 48_000, 1024, 128, 2, 67)
    assert rc == 0 and h.value
    assert lib.af_stream_resampler_output_delay(h) == 69  # resampling.rs:216 at 44.1 -> 48 kHz
    assert lib.af_stream_resampler_pending_input(h) == 0
    for n in (0, 1, 441, 1023, 1024, 1025, 3000, 44_100):
        want = RS.plan_counts([n], 44_100, 48_000)[0] if n else 0
        assert lib.af_stream_resampler_output_frames(h, n) == want, n
    assert lib.af_stream_resampler_frames_in(h) == 0 and lib.af_stream_resampler_frames_out(h) == 0
    assert lib.af_stream_resampler_reset(h) == 0 and lib.af_stream_resampler_clear_pending(h) == 0
    lib.af_stream_resampler_destroy(h)


def test_python_class_is_exported_and_validates():
    import mic_eq_mi
    from mic_eq_mi import mic_eq_core as core

    assert mic_eq_mi.StreamResampler is core.StreamResampler and "StreamResampler" in mic_eq_mi.__all__
    for bad in (dict(input_rate=0, output_rate=48_000), dict(input_rate=48_000, output_rate=44_100, chunk_size=0),
                dict(input_rate=48_000, output_rate=44_100, chunk_size=1025), dict(input_rate=48_000, output_rate=44_100, sinc_len=96),
                dict(input_rate=48_000, output_rate=44_100, window="unknown"), dict(input_rate=48_000, output_rate=44_100, n_streams=0)):
        with pytest.raises(ValueError):
            core.StreamResampler(**bad)
    r = core.StreamResampler(16_000, 48_000, n_streams=3)
    assert r.output_frames(1024) == RS.plan_counts([1024], 16_000, 48_000)[0] and r.pending_input == 0
    r.close()


@pytest.mark.parametrize("rate_in,rate_out", [(44_100, 44_100), (16_000, 48_000), (48_000, 44_100), (0, 0)])
def test_engine_stream_plan_is_host_arithmetic(rate_in, rate_out):
    """On an engine that has not started: the plan of a call is what a fresh helper does with it."""
    import mic_eq_mi

    for suppressor in (0, 1):
        e = mic_eq_mi.Engine(48_000.0, 5)
        e.set_suppressor_enabled(suppressor)
        e.set_io_sample_rates(rate_in, rate_out)  # accepted before start
        for n in (0, 1, 441, 479, 1023, 1024, 1025, 3000, 10_000):
            m1 = n if rate_in in (0, 48_000) else (RS.plan_counts([n], rate_in, 48_000)[0] if n else 0)
            m2 = (m1 // 480) * 480 if suppressor else m1
            m3 = m2 if rate_out in (0, 48_000) else (RS.plan_counts([m2], 48_000, rate_out)[0] if m2 else 0)
            assert e.stream_plan(n) == (m1, m2, m3), (n, suppressor)
        want_delay = (0 if rate_in in (0, 48_000) else int(np.float32(64) * np.float32(48_000 / rate_in)),
                      0 if rate_out in (0, 48_000) else int(np.float32(64) * np.float32(rate_out / 48_000)))
        assert e.io_resampler_delay() == want_delay
        e.set_io_sample_rates(0, 48_000)  # both sides off again: still configuration
        assert e.stream_plan(777) == ((777, 777 // 480 * 480, 777 // 480 * 480) if suppressor else (777, 777, 777))
        e.close()
