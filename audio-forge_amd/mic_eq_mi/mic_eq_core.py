"""Drop-in for the offline operator surface of ``mic_eq.mic_eq_core`` on the MI355X engine.

Function names, argument meaning, returned dict keys and error behaviour follow the PyO3
module of the reference (rust-core/src/lib.rs:99-350, audio/processor/python_api.rs:118-714,
typed in python/mic_eq/mic_eq_core.pyi:202-258).  The audio path is the HIP engine behind
``libaudioforge_mi.so``; this file only (a) replays the reference's setter sequence on an
engine and (b) folds the per-block rows the kernels emit into the dict statistics
(python_api.rs:578-713).  There is no CPU audio path here.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import time
from typing import Any, Mapping, Sequence

import numpy as np

from . import _lib
from ._lib import BlockStats, EqBandConfig

NUM_BANDS = 10
EQ_TYPE_IDS = {"low_shelf": 0, "bell": 1, "high_shelf": 2, "notch": 3, "high_pass": 4, "low_pass": 5}
CAREFUL_OUTPUT_CEILING_DB = -1.5  # audio/processor/control.rs:772
STATS_DTYPE = np.dtype(
    [
        ("input_sample_peak", "<f4"),
        ("output_sample_peak", "<f4"),
        ("true_peak_limiter_input_peak", "<f4"),
        ("output_true_peak", "<f4"),
        ("limiter_peak_gain_reduction_db", "<f4"),
        ("true_peak_limiter_gain_reduction_db", "<f4"),
        ("compressor_gain_reduction_db", "<f4"),
        ("deesser_gain_reduction_db", "<f4"),
        ("input_square_sum", "<f8"),
        ("output_square_sum", "<f8"),
        ("true_peak_limited_events", "<u4"),
        ("non_finite_output", "<u4"),
        ("compressor_makeup_gain_db", "<f4"),
        ("auto_makeup_activity", "<f4"),
        ("auto_makeup_reliability", "<f4"),
        ("reserved", "<f4"),
    ]
)
assert STATS_DTYPE.itemsize == C.sizeof(BlockStats)

f32 = np.float32


# ------------------------------------------------------------------------------- engine
class Engine:
    """N independent reference chains (OfflineDspBlockProcessor) resident on one GPU.

    Setter methods are the C ABI entry points with the ``af_`` prefix dropped, e.g.
    ``engine.compressor_set_threshold(-20.0)`` or ``engine.eq_set_band_gain(2, 3.0)``.
    """

    def __init__(self, sample_rate: float = 48_000.0, n_streams: int = 1, device: int = 0):
        self._lib = _lib.load()
        handle = C.c_void_p()
        _lib.check(self._lib.af_engine_create(float(sample_rate), int(n_streams), int(device), C.byref(handle)))
        self._h = handle
        self._apply_variant_override()
        self.sample_rate = float(sample_rate)
        self.n_streams = int(n_streams)
        self.device = int(device)

    def _apply_variant_override(self) -> None:
        """AF_KERNEL_VARIANT=lane | quad | staged | roles | ring-<waves>x<chunk> pins the kernel (tests and tuning runs)."""
        import os

        variant = os.environ.get("AF_KERNEL_VARIANT", "")
        if variant == "lane":
            _lib.check(self._lib.af_engine_set_kernel(self._h, _lib.KERNEL_LANE_PER_STREAM))
        elif variant == "staged":
            _lib.check(self._lib.af_engine_set_kernel(self._h, _lib.KERNEL_STAGED))
        elif variant == "roles":
            _lib.check(self._lib.af_engine_set_kernel(self._h, _lib.KERNEL_ROLES))
        elif variant.startswith("quad"):  # quad | quad-<waves>
            _lib.check(self._lib.af_engine_set_kernel(self._h, _lib.KERNEL_QUAD))
            if "-" in variant:
                _lib.check(self._lib.af_engine_set_ring_variant(self._h, int(variant.split("-")[1]), 4))
        elif variant.startswith("ring-"):
            waves, chunk = (int(v) for v in variant[5:].split("x"))
            _lib.check(self._lib.af_engine_set_kernel(self._h, _lib.KERNEL_PHASED))
            _lib.check(self._lib.af_engine_set_ring_variant(self._h, waves, chunk))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __getattr__(self, name: str):
        # engine.<x>(...) -> af_<x>(handle, ...) / af_engine_<x>(handle, ...)
        for symbol in (f"af_{name}", f"af_engine_{name}"):
            if symbol in _lib.SIGNATURES:
                fn = getattr(self._lib, symbol)
                is_status = symbol not in _lib.VALUE_FUNCTIONS

                def call(*args, _fn=fn, _is_status=is_status):
                    rc = _fn(self._h, *args)
                    if _is_status:
                        _lib.check(rc)
                        return None
                    return rc

                return call
        raise AttributeError(name)

    def eq_set_band_config_tuple(self, band: int, cfg: tuple) -> None:
        name, freq, gain, q, slope, enabled = cfg
        c = EqBandConfig(EQ_TYPE_IDS[name], float(freq), float(gain), float(q), int(slope), int(bool(enabled)))
        _lib.check(self._lib.af_eq_set_band_config(self._h, band, C.byref(c)))

    def set_live_control(self, enabled: bool) -> None:
        """Accept the chain setters (``eq_set_band_*``, ``compressor_set_*``, ``limiter_set_ceiling`` / ``_release_time``,
        ``true_peak_limiter_set_release_ms``, ``deesser_set_*``) after ``process`` / ``stream`` has started: they then act on
        the running streams, like the reference's realtime control plane, from the first sample of the next call.  A
        configuration setter (RuntimeError after the first call); off by default."""
        _lib.check(self._lib.af_engine_set_live_control(self._h, int(bool(enabled))))

    def live_control_pending(self) -> int:
        """State edits recorded by live setters that the next call will apply."""
        ops = C.c_int32(0)
        _lib.check(self._lib.af_engine_live_control_pending(self._h, C.byref(ops)))
        return ops.value

    def last_retune_ms(self) -> float:
        """Device time of the last call's state-retune launch (timing enabled), 0.0 when it launched none."""
        ms = C.c_double(0.0)
        _lib.check(self._lib.af_engine_last_retune_ms(self._h, C.byref(ms)))
        return ms.value

    # -- per-stream lifecycle -----------------------------------------------------
    def set_stream_lifecycle(self, enabled: bool) -> None:
        """Accept ``restart_streams`` / ``export_stream_state`` / ``import_stream_state`` between calls once streaming has
        started.  A configuration setter (RuntimeError after the first call); off by default.  With it on the engine never
        runs the stage pipeline."""
        _lib.check(self._lib.af_engine_set_stream_lifecycle(self._h, int(bool(enabled))))

    @staticmethod
    def _stream_list(indices):
        idx = [int(i) for i in indices]
        return (C.c_int32 * max(len(idx), 1))(*idx), len(idx)

    def stream_state_size(self) -> int:
        """Bytes of one stream-state blob of this engine."""
        size = C.c_size_t(0)
        _lib.check(self._lib.af_engine_stream_state_size(self._h, C.byref(size)))
        return size.value

    def restart_streams(self, indices) -> None:
        """The listed streams continue from a fresh engine's state (a caller left, another takes the slot); every other
        stream is untouched.  One launch, no wait.  ValueError: duplicate or out-of-range index; NotImplementedError: the
        engine is not at a point where single streams can be cut out (pending samples, a crossfade in flight, ...)."""
        arr, n = self._stream_list(indices)
        _lib.check(self._lib.af_engine_restart_streams(self._h, arr, n))

    def export_stream_state(self, indices) -> list:
        """One canonical state blob (``bytes``) per listed stream: a checkpoint, or what ``import_stream_state`` of another
        engine of the same shape continues from bit for bit."""
        arr, n = self._stream_list(indices)
        size = self.stream_state_size()
        buf = (C.c_ubyte * max(size * n, 1))()
        _lib.check(self._lib.af_engine_export_stream_state(self._h, arr, n, C.cast(buf, C.c_void_p)))
        raw = bytes(buf)
        return [raw[i * size:(i + 1) * size] for i in range(n)]

    def import_stream_state(self, indices, blobs) -> None:
        """Put exported blobs into the listed slots.  ValueError, nothing touched: a blob that is not one (magic, version)
        or whose shape record differs from the slot's; the message names the field."""
        arr, n = self._stream_list(indices)
        blobs = [bytes(b) for b in blobs]
        size = self.stream_state_size()
        if len(blobs) != n:
            raise ValueError(f"expected {n} blobs, got {len(blobs)}")
        for i, b in enumerate(blobs):
            if len(b) != size:
                raise ValueError(f"blob {i} has {len(b)} bytes, a stream state blob of this engine has {size}")
        raw = b"".join(blobs)
        buf = (C.c_ubyte * max(len(raw), 1)).from_buffer_copy(raw or b"\0")
        _lib.check(self._lib.af_engine_import_stream_state(self._h, arr, n, C.cast(buf, C.c_void_p)))

    def stream_samples_processed(self, stream: int) -> int:
        """Samples the stream has run since its own (re)start; an import carries the count over."""
        out = C.c_int64(0)
        _lib.check(self._lib.af_engine_stream_samples_processed(self._h, int(stream), C.byref(out)))
        return out.value

    # -- processing ---------------------------------------------------------------
    def process(self, audio: np.ndarray, layout: int = _lib.LAYOUT_STREAM_MAJOR) -> np.ndarray:
        """Host arrays: [n_streams, n] (stream-major) or [n, n_streams] (time-major) float32."""
        a = np.ascontiguousarray(audio, dtype=np.float32)
        if a.ndim == 1:
            a = a.reshape(1, -1) if layout == _lib.LAYOUT_STREAM_MAJOR else a.reshape(-1, 1)
        n_streams, n = (a.shape if layout == _lib.LAYOUT_STREAM_MAJOR else a.shape[::-1])
        if n_streams != self.n_streams:
            raise ValueError(f"expected {self.n_streams} streams, got {n_streams}")
        fp = C.POINTER(C.c_float)
        if layout == _lib.LAYOUT_STREAM_MAJOR:
            # with the suppressor on a call returns the whole 480-sample frames that are complete (rnnoise.rs:114-164):
            # floor((pending + n) / 480) * 480 samples per stream, the rest waits in the engine
            stride = int(n) + 480
            out = np.empty((n_streams, stride), dtype=np.float32)
            n_out = C.c_int64(0)
            _lib.check(self._lib.af_engine_stream_host(self._h, a.ctypes.data_as(fp), int(n), out.ctypes.data_as(fp), stride,
                                                       C.byref(n_out)))
            return np.ascontiguousarray(out[:, : n_out.value])
        out = np.empty_like(a)
        _lib.check(self._lib.af_engine_process_host(self._h, a.ctypes.data_as(fp), out.ctypes.data_as(fp), int(n), layout))
        return out

    def stream_plan(self, n_in: int) -> tuple[int, int, int]:
        """What the next ``stream`` call of n_in frames per stream will do, from the host alone: (frames the input resampler
        hands the chain, frames the chain returns, frames that come out).  Size VAD / activity evidence from the first two."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.af_engine_stream_plan(self._h, int(n_in), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def stream(self, x: np.ndarray) -> np.ndarray:
        """One wake-up over af_engine_stream_host: float32 [n_streams, n] at the input rate -> [n_streams, m] at the output
        rate (``set_io_sample_rates``; without it the engine's own rate on both sides)."""
        a = np.ascontiguousarray(x, dtype=np.float32)
        channels = getattr(self, "_input_channels", 1)
        if channels > 1:  # set_input_channels: interleaved frames, [n_streams, n, channels]
            if a.ndim == 2 and self.n_streams == 1:
                a = a.reshape(1, *a.shape)
            if a.ndim != 3 or a.shape[2] != channels:
                raise ValueError(f"expected [streams, frames, {channels}] interleaved frames, got shape {a.shape}")
        elif a.ndim == 3:
            raise ValueError("3-D input needs set_input_channels(n_channels > 1, mode) first")
        if a.ndim == 1:
            a = a.reshape(1, -1)
        if a.shape[0] != self.n_streams:
            raise ValueError(f"expected {self.n_streams} streams, got {a.shape[0]}")
        n = a.shape[1]
        stride = max(self.stream_plan(n)[2], 1)
        out = np.empty((self.n_streams, stride), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        n_out = C.c_int64(0)
        _lib.check(self._lib.af_engine_stream_host(self._h, a.ctypes.data_as(fp), n, out.ctypes.data_as(fp), stride, C.byref(n_out)))
        return np.ascontiguousarray(out[:, : n_out.value])

    def set_input_channels(self, n_channels: int, mode="average") -> None:
        """Multichannel input (a configuration setter): ``stream`` then takes [n_streams, n, n_channels] and the capture
        callback's mixdown (input.rs:785-843) runs first on the device.  One channel: off.  ``mode``: an id of
        input.rs:158-180 ("average", "left", "right", "max_rms", "phase_safe_mono") or its number."""
        _lib.check(self._lib.af_engine_set_input_channels(self._h, int(n_channels), input_channel_mode(mode)))
        self._input_channels = int(n_channels)

    def set_input_channel_mode(self, mode) -> None:
        """Live: takes effect with the next ``stream`` call and keeps the phase-safe history."""
        _lib.check(self._lib.af_engine_set_input_channel_mode(self._h, input_channel_mode(mode)))

    def input_phase(self) -> dict:
        """The capture callback's phase diagnostics, arrays per stream: as ``Mixdown.diagnostics``."""
        return _read_phase(self._lib.af_engine_read_input_phase, self._h, self.n_streams)

    def set_output_writer(self, enabled: bool) -> None:
        """The output writer behind the chain / output resampler (a configuration setter): every ``stream`` call then ends
        with one write_chunk per stream (output_writer.rs:62-110) and returns ragged rows, zero beyond ``output_written()``."""
        _lib.check(self._lib.af_engine_set_output_writer(self._h, int(bool(enabled))))

    def set_output_queue_fill(self, fill) -> None:
        """Frames in each stream's playback queue, used from the next ``stream`` call on (until then: the target centre)."""
        f = np.asarray(fill)
        if f.shape != (self.n_streams,) or not np.issubdtype(f.dtype, np.integer):
            raise ValueError(f"fill must be {self.n_streams} integers (frames in each stream's queue)")
        f = np.ascontiguousarray(f, dtype=np.int64)
        _lib.check(self._lib.af_engine_set_output_queue_fill(self._h, f.ctypes.data_as(C.POINTER(C.c_int64)), self.n_streams))

    def output_written(self) -> np.ndarray:
        """Frames of each row of the last ``stream`` call that reached the queue."""
        w = np.zeros(self.n_streams, dtype=np.int64)
        _lib.check(self._lib.af_engine_read_output_written(self._h, w.ctypes.data_as(C.POINTER(C.c_int64)), self.n_streams))
        return w

    def output_counters(self) -> dict:
        """As ``OutputWriter.counters``."""
        return _read_writer_counters(self._lib.af_engine_read_output_counters, self._h, self.n_streams)

    def output_meters(self) -> dict:
        """As ``OutputWriter.meters``."""
        return _read_writer_meters(self._lib.af_engine_read_output_meters, self._h, self.n_streams)

    def io_resampler_delay(self) -> tuple[int, int]:
        """(input side, output side) ``output_delay()`` in frames, 0 for a side that does not resample."""
        a, b = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.af_engine_io_resampler_delay(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def io_resampler_pending(self) -> tuple[int, int]:
        """(input side, output side) frames queued in the I/O resamplers, 0 for a side that does not resample."""
        a, b = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.af_engine_io_resampler_pending(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def suppressor_trace(self) -> np.ndarray:
        """[frames, n_streams, 2] int32: (silence flag, pitch index) of every frame of the last process call
        (needs ``suppressor_set_trace_enabled(1)`` before the call)."""
        frames = int(self._lib.af_suppressor_trace_frames(self._h))
        out = np.zeros((frames, self.n_streams, 2), dtype=np.int32)
        if frames:
            _lib.check(self._lib.af_suppressor_read_trace(self._h, out.ctypes.data_as(C.POINTER(C.c_int32)), frames))
        return out

    def suppressor_debug_read(self, frame: int, stream: int) -> dict:
        """The suppressor's test tap for one (frame, stream) cell of the LAST window of the last call (cells of earlier
        windows, and frames beyond that window's, are stale): Ex Ep Exp [22], feat [44] (42 features + the two pad words the
        network's K padding reads), gains_raw gains [22], silence, pitch_index, and the spectra X P [481] complex64."""
        rec = np.zeros(160, dtype=np.float32)  # af::SuppFrameRec
        X = np.zeros(481, dtype=np.complex64)
        P = np.zeros(481, dtype=np.complex64)
        fp = C.POINTER(C.c_float)
        _lib.check(self._lib.af_suppressor_debug_read(self._h, int(frame), int(stream), rec.ctypes.data_as(fp),
                                                      X.ctypes.data_as(fp), P.ctypes.data_as(fp)))
        silence, pitch = (int(v) for v in rec[154:156].view(np.int32))
        return {"Ex": rec[0:22].copy(), "Ep": rec[22:44].copy(), "Exp": rec[44:66].copy(), "feat": rec[66:110].copy(),
                "gains_raw": rec[110:132].copy(), "gains": rec[132:154].copy(), "silence": silence, "pitch_index": pitch,
                "X": X, "P": P}

    def suppressor_debug_read_pitch(self, frame: int | None, stream: int) -> dict:
        """The pitch path's test tap: ``whitened`` [864] float32, the LPC-whitened 2x-decimated pitch buffer of one
        (frame, stream) cell of the LAST window (``frame`` None: left out), and the stream's tracker state as the last call
        left it, ``last_period`` (int) and ``last_gain`` (float32)."""
        ds = None if frame is None else np.zeros(864, dtype=np.float32)
        period, gain = C.c_int32(0), C.c_float(0.0)
        fp = C.POINTER(C.c_float)
        _lib.check(self._lib.af_suppressor_debug_read_pitch(self._h, 0 if frame is None else int(frame), int(stream),
                                                            None if ds is None else ds.ctypes.data_as(fp), C.byref(period),
                                                            C.byref(gain)))
        return {"whitened": ds, "last_period": int(period.value), "last_gain": np.float32(gain.value)}

    def suppressor_debug_read_model_input(self, stream: int) -> np.ndarray:
        """The pre-pass's test tap: ``stream``'s row of the LAST window's model-input buffer, float32
        [1728 + 480 x that window's frames]: the history samples the pre-pass put in front, then the window's."""
        n = C.c_int64(0)
        _lib.check(self._lib.af_suppressor_debug_read_model_input(self._h, int(stream), None, 0, C.byref(n)))
        row = np.zeros(n.value, dtype=np.float32)
        _lib.check(self._lib.af_suppressor_debug_read_model_input(self._h, int(stream), row.ctypes.data_as(C.POINTER(C.c_float)),
                                                                  row.size, C.byref(n)))
        assert n.value == row.size
        return row

    @staticmethod
    def suppressor_debug_pitch_search(spans, device: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """The pitch search kernel alone (no engine state), launched as the engine launches it, on model-input ``spans``
        [streams, 1728 + 480 n_frames] float32: (whitened buffers [n_frames, streams, 864] float32, the search's own pitch
        index [n_frames, streams] int32 -- the one the tracker overwrites in an engine run)."""
        x = np.ascontiguousarray(spans, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] <= 1728 or (x.shape[1] - 1728) % 480:
            raise ValueError("spans must be [streams, 1728 + 480 n_frames]")
        n_streams, n_frames = x.shape[0], (x.shape[1] - 1728) // 480
        ds = np.zeros((n_frames, n_streams, 864), dtype=np.float32)
        pitch = np.zeros((n_frames, n_streams), dtype=np.int32)
        fp = C.POINTER(C.c_float)
        _lib.check(_lib.load().af_suppressor_debug_pitch_search(x.ctypes.data_as(fp), n_streams, n_frames, ds.ctypes.data_as(fp),
                                                                pitch.ctypes.data_as(C.POINTER(C.c_int32)), int(device)))
        return ds, pitch

    def process_device(self, in_ptr: int, out_ptr: int, n_samples: int, stream_stride: int,
                       layout: int = _lib.LAYOUT_STREAM_MAJOR, hip_stream: int = 0) -> None:
        """Device pointers (e.g. ``tensor.data_ptr()``); asynchronous on ``hip_stream``."""
        _lib.check(self._lib.af_engine_process_device(self._h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), int(n_samples),
                                                      int(stream_stride), int(layout), C.c_void_p(hip_stream)))

    def gate_state(self) -> dict:
        """Each stream's noise gate as of the end of the last call: ``current_gain`` (float32), ``chatter_events``
        (uint64, since reset), ``is_open`` and ``auto_relax_active`` (bool)."""
        gain = np.zeros(self.n_streams, dtype=np.float32)
        events = np.zeros(self.n_streams, dtype=np.uint64)
        flags = np.zeros(self.n_streams, dtype=np.int32)
        _lib.check(self._lib.af_engine_read_gate_state(self._h, gain.ctypes.data_as(C.POINTER(C.c_float)),
                                                        events.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                        flags.ctypes.data_as(C.POINTER(C.c_int32)), self.n_streams))
        return {"current_gain": gain, "chatter_events": events, "is_open": (flags & 1) != 0,
                "auto_relax_active": (flags & 2) != 0}

    def gate_set_vad_evidence(self, probabilities=None, available=None) -> None:
        """Speech probability and availability per control block of the NEXT call's gate pass: [blocks] (shared by all
        streams) or [blocks, n_streams].  ``None`` clears it (every block then runs with probability 0, not available)."""
        if probabilities is None:
            _lib.check(self._lib.af_gate_set_vad_evidence(self._h, None, None, 0, 0))
            return
        p = np.ascontiguousarray(probabilities, dtype=np.float32)
        a = np.ascontiguousarray(np.ones(p.shape, bool) if available is None else available).astype(np.uint8)
        if a.shape != p.shape or p.ndim not in (1, 2) or (p.ndim == 2 and p.shape[1] != self.n_streams):
            raise ValueError("evidence must be [blocks] or [blocks, n_streams], probabilities and flags alike")
        _lib.check(self._lib.af_gate_set_vad_evidence(self._h, p.ctypes.data_as(C.POINTER(C.c_float)),
                                                       a.ctypes.data_as(C.POINTER(C.c_uint8)), p.shape[0], int(p.ndim == 2)))

    def gate_vad_controls(self) -> dict:
        """The VAD controller's settings: ``vad_threshold``, ``hold_ms``, ``margin_db``, ``auto_threshold``, ``attached``."""
        thr, hold, margin = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
        auto, attached = C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.af_gate_read_vad_controls(self._h, C.byref(thr), C.byref(hold), C.byref(margin), C.byref(auto),
                                                        C.byref(attached)))
        return {"vad_threshold": thr.value, "hold_ms": hold.value, "margin_db": margin.value,
                "auto_threshold": bool(auto.value), "attached": bool(attached.value)}

    def gate_vad_decisions(self, n_blocks: int) -> dict:
        """The per-block decisions of the last fused call, [n_blocks, n_streams]: ``probability`` (clamped), ``noise_floor_db``
        after the block, ``held_open`` and ``available``."""
        prob = np.zeros((n_blocks, self.n_streams), dtype=np.float32)
        floor = np.zeros((n_blocks, self.n_streams), dtype=np.float32)
        flags = np.zeros((n_blocks, self.n_streams), dtype=np.int32)
        fp = C.POINTER(C.c_float)
        _lib.check(self._lib.af_engine_read_gate_vad_decisions(self._h, prob.ctypes.data_as(fp), floor.ctypes.data_as(fp),
                                                                flags.ctypes.data_as(C.POINTER(C.c_int32)), int(n_blocks)))
        return {"probability": prob, "noise_floor_db": floor, "held_open": (flags & 1) != 0, "available": (flags & 4) != 0}

    def gate_vad_state(self) -> dict:
        """Each stream's VAD-fused gate as of the end of the last call: ``noise_floor_db``, ``noise_floor_reliability``,
        ``fused_score``, ``probability`` (the smoothed posterior) (float32), ``gate_state`` (0 Closed, 1 Opening, 2 Open,
        3 Uncertain, 4 Releasing), ``held_open`` / ``available`` (the last block's decision) and ``fused_open`` (bool)."""
        f = [np.zeros(self.n_streams, dtype=np.float32) for _ in range(4)]
        state = np.zeros(self.n_streams, dtype=np.int32)
        flags = np.zeros(self.n_streams, dtype=np.int32)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        _lib.check(self._lib.af_engine_read_gate_vad_state(self._h, *(x.ctypes.data_as(fp) for x in f), state.ctypes.data_as(ip),
                                                            flags.ctypes.data_as(ip), self.n_streams))
        return {"noise_floor_db": f[0], "noise_floor_reliability": f[1], "fused_score": f[2], "probability": f[3],
                "gate_state": state, "held_open": (flags & 1) != 0, "fused_open": (flags & 2) != 0, "available": (flags & 4) != 0}

    def block_stats(self) -> np.ndarray:
        """Structured array [blocks, n_streams] of the last process call."""
        blocks = int(self._lib.af_engine_last_block_count(self._h))
        rows = np.zeros((blocks, self.n_streams), dtype=STATS_DTYPE)
        if blocks:
            _lib.check(self._lib.af_engine_read_block_stats(self._h, rows.ctypes.data_as(C.POINTER(BlockStats)), rows.size))
        return rows

    def debug_detector_reuse_chunks(self) -> int:
        """Test tap: chunks (summed over 64-stream groups and token-ring launches so far) whose output true-peak detector took
        the input observer's maxima instead of running its own FIR."""
        n = C.c_uint64(0)
        _lib.check(self._lib.af_engine_debug_detector_reuse_chunks(self._h, C.byref(n)))
        return int(n.value)

    def last_kernel_ms(self) -> tuple[float, int]:
        ms, launches = C.c_double(0.0), C.c_int32(0)
        _lib.check(self._lib.af_engine_last_kernel_ms(self._h, C.byref(ms), C.byref(launches)))
        return ms.value, launches.value

    def last_chain_launch_ms(self) -> tuple[float, float, int]:
        """(summed ms of the chain launches of the last call, 0.0, number of launches)."""
        first, tail, segments = C.c_double(0.0), C.c_double(0.0), C.c_int32(0)
        _lib.check(self._lib.af_engine_last_chain_launch_ms(self._h, C.byref(first), C.byref(tail), C.byref(segments)))
        return first.value, tail.value, segments.value


# ---------------------------------------------------------------------- argument checks
def _audio_1d(audio) -> np.ndarray:
    if not isinstance(audio, np.ndarray) or audio.dtype != np.float32 or audio.ndim != 1:
        raise TypeError("audio must be a 1-D numpy.float32 array")
    if not audio.flags.c_contiguous:
        raise ValueError("audio must be a contiguous float32 array")
    return audio


def _bands_v2(bands, sample_rate: float):
    """parse_eq_v2_bands, lib.rs:154-189."""
    if not np.isfinite(sample_rate) or sample_rate <= 0.0:
        raise ValueError("sample_rate must be finite and positive")
    if len(bands) != NUM_BANDS:
        raise ValueError(f"expected {NUM_BANDS} EQ bands, got {len(bands)}")
    arr = (EqBandConfig * NUM_BANDS)()
    lib = _lib.load()
    for index, (name, freq, gain, q, slope, enabled) in enumerate(bands):
        if name not in EQ_TYPE_IDS:
            raise ValueError(f"band {index} has unsupported EQ filter type: {name}")
        arr[index] = EqBandConfig(EQ_TYPE_IDS[name], float(freq), float(gain), float(q), int(slope), int(bool(enabled)))
        _lib.check(lib.af_eq_band_config_validate(C.byref(arr[index]), index, float(sample_rate)))
    return arr


def _get(settings: Mapping[str, object] | None, key: str, default):
    if settings is not None and key in settings and settings[key] is not None:
        value = settings[key]
        if isinstance(default, bool):
            if not isinstance(value, (bool, np.bool_)):
                raise TypeError(f"settings[{key!r}] must be a bool")
            return bool(value)
        return float(value)
    return default


# ---------------------------------------------------- python_api.rs:54-111 statistics
def _linear_to_db(value) -> np.float32:
    return f32(20.0) * np.log10(np.maximum(f32(value), f32(1.0e-12)), dtype=np.float32)


def _percentile(values: np.ndarray, percentile: float) -> np.float32:
    values = np.sort(np.asarray(values, dtype=np.float32))
    if values.size == 0:
        return f32(0.0)
    position = f32(values.size - 1) * f32(min(max(percentile, 0.0), 1.0))
    lower = int(np.floor(position))
    upper = int(np.ceil(position))
    if lower == upper:
        return values[lower]
    fraction = position - f32(lower)
    return values[lower] + fraction * (values[upper] - values[lower])


def _pumping_score(trace: np.ndarray, cadence_hz: float) -> np.float32:
    trace = np.asarray(trace, dtype=np.float32)
    if trace.size < 3 or not np.isfinite(cadence_hz) or cadence_hz <= 0.0:
        return f32(0.0)
    pi = f32(np.pi)
    dt = f32(1.0) / f32(cadence_hz)
    highpass_rc = f32(1.0) / (f32(2.0) * pi * f32(2.0))
    lowpass_rc = f32(1.0) / (f32(2.0) * pi * f32(8.0))
    highpass_alpha = highpass_rc / (highpass_rc + dt)
    lowpass_alpha = dt / (lowpass_rc + dt)
    previous = trace[0]
    highpass = f32(0.0)
    bandpass = f32(0.0)
    bandpass_abs = np.empty(trace.size - 1, dtype=np.float32)
    deltas = np.empty(trace.size - 1, dtype=np.float32)
    for i in range(1, trace.size):
        value = trace[i]
        if not np.isfinite(value):
            return f32(np.inf)
        highpass = highpass_alpha * (highpass + value - previous)
        bandpass = bandpass + lowpass_alpha * (highpass - bandpass)
        bandpass_abs[i - 1] = abs(bandpass)
        deltas[i - 1] = abs(value - previous)
        previous = value
    robust_limit = _percentile(bandpass_abs, 0.95)
    total = f32(0.0)
    for v in np.minimum(bandpass_abs, robust_limit):
        total = total + v * v
    robust_rms = np.sqrt(total / f32(bandpass_abs.size))
    return f32(robust_rms + _percentile(deltas, 0.95))


def chain_diagnostics(rows: np.ndarray, block_lengths: np.ndarray, effective_ceiling_db: float) -> dict[str, Any]:
    """Fold one stream's per-block rows into the dict of python_api.rs:578-713."""
    n_rows = rows.shape[0]
    in_sq_total = 0.0
    out_sq_total = 0.0
    for k in range(n_rows):  # sequential f64 accumulation order of python_api.rs:519-571
        in_sq_total += float(rows["input_square_sum"][k])
        out_sq_total += float(rows["output_square_sum"][k])
    samples = int(block_lengths.sum())
    input_rms = f32(np.sqrt(in_sq_total / samples)) if samples > 0 else f32(0.0)
    output_rms = f32(np.sqrt(out_sq_total / samples)) if samples > 0 else f32(0.0)
    lengths = block_lengths.astype(np.float64)
    block_in_rms = np.sqrt(rows["input_square_sum"] / lengths).astype(np.float32)
    block_out_rms = np.sqrt(rows["output_square_sum"] / lengths).astype(np.float32)
    in_db = _linear_to_db(block_in_rms)
    out_db = _linear_to_db(block_out_rms)
    comp = rows["compressor_gain_reduction_db"].astype(np.float32)
    dees = rows["deesser_gain_reduction_db"].astype(np.float32)

    def fmax(field):
        return f32(rows[field].max()) if n_rows else f32(0.0)

    input_sample_peak = max(f32(0.0), fmax("input_sample_peak"))
    output_sample_peak = max(f32(0.0), fmax("output_sample_peak"))
    pre_limiter_true_peak = max(f32(0.0), fmax("true_peak_limiter_input_peak"))
    output_true_peak = max(f32(0.0), fmax("output_true_peak"))
    output_sample_peak_db = _linear_to_db(output_sample_peak)
    pre_limiter_true_peak_db = _linear_to_db(pre_limiter_true_peak)
    output_true_peak_db = _linear_to_db(output_true_peak)
    ceiling = f32(effective_ceiling_db)

    input_floor_db = _percentile(in_db, 0.20)
    input_p90_db = _percentile(in_db, 0.90)
    active_threshold_db = max(max(input_floor_db + f32(6.0), input_p90_db - f32(24.0)), f32(-60.0))
    active = in_db >= active_threshold_db
    active_comp = np.maximum(comp[active], f32(0.0))
    active_dees = np.maximum(dees[active], f32(0.0))
    if active_comp.size < 3:
        active_comp = np.maximum(comp, f32(0.0))
        active_dees = np.maximum(dees, f32(0.0))
    active_block_count = int(active_comp.size)
    active_ratio = f32(np.count_nonzero(active_comp >= f32(0.10))) / f32(active_block_count) if active_block_count else f32(0.0)
    audible = in_db > f32(-100.0)
    active_output_gain = _percentile((out_db - in_db)[active & audible], 0.50)
    silence_level_delta = _percentile((out_db - in_db)[(~active) & audible], 0.50)
    silence_output_gain = _percentile(-np.maximum(comp[~active], f32(0.0)), 0.50)
    pumping = _pumping_score(np.maximum(comp, f32(0.0)), 50.0)
    return {
        "input_sample_peak_db": float(_linear_to_db(input_sample_peak)),
        "input_rms_db": float(_linear_to_db(input_rms)),
        "output_sample_peak_db": float(output_sample_peak_db),
        "pre_limiter_true_peak_db": float(pre_limiter_true_peak_db),
        "output_true_peak_db": float(output_true_peak_db),
        "output_rms_db": float(_linear_to_db(output_rms)),
        "limiter_effective_ceiling_db": float(ceiling),
        "sample_headroom_db": float(ceiling - output_sample_peak_db),
        "pre_limiter_true_peak_headroom_db": float(ceiling - pre_limiter_true_peak_db),
        "true_peak_headroom_db": float(ceiling - output_true_peak_db),
        "limiter_gain_reduction_db": float(max(f32(0.0), fmax("limiter_peak_gain_reduction_db"))),
        "true_peak_limiter_gain_reduction_db": float(max(f32(0.0), fmax("true_peak_limiter_gain_reduction_db"))),
        "true_peak_limited_events": int(rows["true_peak_limited_events"].sum()),
        "compressor_gain_reduction_db": float(max(f32(0.0), fmax("compressor_gain_reduction_db"))),
        "deesser_gain_reduction_db": float(max(f32(0.0), fmax("deesser_gain_reduction_db"))),
        "compressor_gain_reduction_median_db": float(_percentile(active_comp, 0.50)),
        "compressor_gain_reduction_p95_db": float(_percentile(active_comp, 0.95)),
        "compressor_gain_reduction_active_ratio": float(active_ratio),
        "active_output_gain_db": float(active_output_gain),
        "silence_output_gain_db": float(silence_output_gain),
        "silence_level_delta_db": float(silence_level_delta),
        "compressor_pumping_score_db": float(pumping),
        "non_finite_output": bool(rows["non_finite_output"].any()),
        "deesser_gain_reduction_median_db": float(_percentile(active_dees, 0.50)),
        "deesser_gain_reduction_p95_db": float(_percentile(active_dees, 0.95)),
        "analysis_block_ms": 20.0,
        "active_analysis_threshold_db": float(active_threshold_db),
        "active_analysis_block_count": active_block_count,
        "processed_samples": samples,
    }


# ------------------------------------------------------------ simulate_auto_eq_chain
def configure_auto_eq_chain(engine: Engine, sample_rate: float, bands, settings: Mapping[str, object] | None) -> float:
    """Replay python_api.rs:400-487 on `engine`; returns the effective limiter ceiling (dB, f32)."""
    engine.set_eq_enabled(1)
    if settings is not None and settings.get("eq_bands_v2") is not None:
        arr = _bands_v2(list(settings["eq_bands_v2"]), sample_rate)
        lib = _lib.load()
        for index in range(NUM_BANDS):
            _lib.check(lib.af_eq_set_band_config(engine._h, index, C.byref(arr[index])))
        engine.eq_reset()
    else:
        for index, (frequency, gain_db, q) in enumerate(bands):
            engine.eq_set_band_frequency(index, float(frequency))
            engine.eq_set_band_gain(index, float(gain_db))
            engine.eq_set_band_q(index, float(q))
    deesser_enabled = _get(settings, "deesser_enabled", False)
    engine.set_eq_before_deesser(int(_get(settings, "eq_before_deesser", False)))
    engine.set_deesser_enabled(int(deesser_enabled))
    if deesser_enabled:
        engine.deesser_set_auto_enabled(int(_get(settings, "deesser_auto_enabled", True)))
        engine.deesser_set_auto_amount(_get(settings, "deesser_auto_amount", 0.5))
        engine.deesser_set_low_cut_hz(_get(settings, "deesser_low_cut_hz", 4000.0))
        engine.deesser_set_high_cut_hz(_get(settings, "deesser_high_cut_hz", 11_000.0))
        engine.deesser_set_threshold_db(_get(settings, "deesser_threshold_db", -28.0))
        engine.deesser_set_ratio(_get(settings, "deesser_ratio", 4.0))
        engine.deesser_set_attack_ms(_get(settings, "deesser_attack_ms", 2.0))
        engine.deesser_set_release_ms(_get(settings, "deesser_release_ms", 80.0))
        engine.deesser_set_max_reduction_db(_get(settings, "deesser_max_reduction_db", 6.0))
    compressor_enabled = _get(settings, "compressor_enabled", True)
    engine.set_compressor_enabled(int(compressor_enabled))
    if compressor_enabled:
        engine.compressor_set_threshold(_get(settings, "compressor_threshold_db", -20.0))
        engine.compressor_set_ratio(_get(settings, "compressor_ratio", 4.0))
        engine.compressor_set_attack_time(_get(settings, "compressor_attack_ms", 10.0))
        engine.compressor_set_release_time(_get(settings, "compressor_release_ms", 200.0))
        engine.compressor_set_makeup_gain(_get(settings, "compressor_makeup_gain_db", 0.0))
        engine.compressor_set_adaptive_release(int(_get(settings, "compressor_adaptive_release", False)))
        engine.compressor_set_base_release_time(_get(settings, "compressor_base_release_ms", 50.0))
        engine.compressor_set_auto_makeup_enabled(int(_get(settings, "compressor_auto_makeup_enabled", False)))
        engine.compressor_set_target_lufs(_get(settings, "compressor_target_lufs", -18.0))
        engine.compressor_set_sidechain_highpass_enabled(int(_get(settings, "compressor_sidechain_highpass_enabled", True)))
    limiter_enabled = _get(settings, "limiter_enabled", True)
    engine.set_limiter_enabled(int(limiter_enabled))
    ceiling_db = _get(settings, "limiter_ceiling_db", -0.5)
    careful = _get(settings, "limiter_careful_output_enabled", True)
    # effective_limiter_ceiling_db, audio/processor/control.rs:904-910, then `as f32`
    effective = float(f32(min(ceiling_db, CAREFUL_OUTPUT_CEILING_DB) if careful else ceiling_db))
    if limiter_enabled:
        release_ms = _get(settings, "limiter_release_ms", 50.0)
        engine.limiter_set_lookahead_ms(_get(settings, "limiter_lookahead_ms", 2.0))
        engine.limiter_set_ceiling(effective)
        engine.limiter_set_release_time(release_ms)
        engine.true_peak_limiter_set_release_ms(float(f32(release_ms)))
    block = int(min(max(round(sample_rate * 0.020), 1), 8192))  # python_api.rs:512-514
    engine.set_control_block_samples(block)
    return effective


def _block_lengths(n: int, block: int) -> np.ndarray:
    full, rest = divmod(n, block)
    return np.asarray([block] * full + ([rest] if rest else []), dtype=np.int64)


GROUP_STREAMS = 64  # streams of one chain workgroup = the granularity of a preset


def _is_preset_list(bands, settings) -> bool:
    return isinstance(settings, (list, tuple)) or (len(bands) > 0 and isinstance(bands[0], (list, tuple)) and len(bands[0]) > 0
                                                    and isinstance(bands[0][0], (list, tuple)))


def simulate_auto_eq_chain_batch(audio: np.ndarray, sample_rate: float, bands, settings=None, device: int = 0,
                                 diagnostics: bool = True, route: str = "groups") -> tuple[np.ndarray, list[dict[str, Any]]]:
    """Batched form: ``audio`` is [n_streams, n] float32.

    ``bands`` / ``settings`` are either one preset for every stream (the reference's arguments), or one entry per
    stream (a list of 10-band lists / a list of settings dicts): the reference configures one processor per stream
    (python/mic_eq/config_parts/settings.py:543-593).  Streams that share a preset are packed into groups of 64 (the unit
    a preset applies to on the GPU; partial groups are padded with silent streams) and handed back in the caller's order.

    ``route="groups"`` (the default) is that path.  ``route="lanes"`` runs the same call on a ``LaneChain`` (lane_chain.py): one
    lane per stream, no packing and no padding, the right choice when most streams have a preset of their own (DESIGN 4.25
    has the measured crossover).  It returns the same values and raises NotImplementedError, naming the setting, for what a
    lane does not run: the de-esser, auto-makeup, typed bands, and limiter lookaheads that differ between streams.

    Returns (output [n_streams, n] float32, one reference-shaped dict per stream).
    """
    started = time.perf_counter()
    if route not in ("groups", "lanes"):
        raise ValueError(f"route must be 'groups' or 'lanes', got {route!r}")
    if not np.isfinite(sample_rate) or sample_rate <= 0.0:
        raise ValueError("sample_rate must be positive and finite")
    audio = np.ascontiguousarray(audio, dtype=np.float32)
    if audio.ndim != 2:
        raise TypeError("audio must be [n_streams, n_samples]")
    n_streams, n = audio.shape
    if route == "lanes":
        from . import lane_chain

        if not _is_preset_list(bands, settings) and len(bands) != NUM_BANDS:
            raise ValueError(f"expected {NUM_BANDS} EQ bands, got {len(bands)}")
        output, rows, effective = lane_chain.simulate_lanes(audio, float(sample_rate), bands, settings, device)
        results = []
        if diagnostics:
            lengths = _block_lengths(n, int(min(max(round(sample_rate * 0.020), 1), 8192)))
            runtime_ms = (time.perf_counter() - started) * 1000.0
            for s_i in range(n_streams):
                d = chain_diagnostics(rows[:, s_i], lengths, effective[s_i])
                d["candidate_runtime_ms"] = runtime_ms
                results.append(d)
        return output, results
    if not _is_preset_list(bands, settings):
        if len(bands) != NUM_BANDS:
            raise ValueError(f"expected {NUM_BANDS} EQ bands, got {len(bands)}")
        presets = [(bands, settings)]
        stream_preset = np.zeros(n_streams, dtype=np.int64)
    else:
        per_bands = list(bands) if (len(bands) and isinstance(bands[0][0], (list, tuple))) else [bands] * n_streams
        per_settings = list(settings) if isinstance(settings, (list, tuple)) else [settings] * n_streams
        if len(per_bands) != n_streams or len(per_settings) != n_streams:
            raise ValueError(f"expected one preset per stream ({n_streams}), got {len(per_bands)} band lists and {len(per_settings)} settings")
        presets, index, stream_preset = [], {}, np.zeros(n_streams, dtype=np.int64)
        for s_i, (b, st) in enumerate(zip(per_bands, per_settings)):
            if len(b) != NUM_BANDS:
                raise ValueError(f"expected {NUM_BANDS} EQ bands, got {len(b)}")
            key = (repr([tuple(x) for x in b]), repr(sorted((st or {}).items(), key=lambda kv: kv[0])))
            if key not in index:
                index[key] = len(presets)
                presets.append((b, st))
            stream_preset[s_i] = index[key]
    # pack: streams of preset k -> whole groups of 64
    order, group_preset = [], []
    for k in range(len(presets)):
        members = np.flatnonzero(stream_preset == k)
        padded = -(-members.size // GROUP_STREAMS) * GROUP_STREAMS if len(presets) > 1 else members.size
        order.extend(members.tolist() + [-1] * (padded - members.size))
        group_preset.extend([k] * (-(-padded // GROUP_STREAMS)))
    order = np.asarray(order, dtype=np.int64)
    packed = np.zeros((order.size, n), dtype=np.float32)
    packed[order >= 0] = audio[order[order >= 0]]
    engine = Engine(sample_rate, int(order.size), device)
    try:
        effective = []
        if len(presets) > 1:
            engine.set_preset_count(len(presets))
        for k, (b, st) in enumerate(presets):
            if len(presets) > 1:
                engine.select_preset(k)
            effective.append(configure_auto_eq_chain(engine, float(sample_rate), b, st))
        if len(presets) > 1:
            gp = np.asarray(group_preset, dtype=np.int32)
            _lib.check(engine._lib.af_engine_assign_presets(engine._h, gp.ctypes.data_as(C.POINTER(C.c_int32)), int(gp.size)))
        packed_out = engine.process(packed) if n else packed.copy()
        rows = engine.block_stats()
    finally:
        engine.close()
    output = np.empty_like(audio)
    position = np.empty(n_streams, dtype=np.int64)
    position[order[order >= 0]] = np.flatnonzero(order >= 0)
    output[:] = packed_out[position]
    results: list[dict[str, Any]] = []
    if diagnostics:
        block = int(min(max(round(sample_rate * 0.020), 1), 8192))
        lengths = _block_lengths(n, block)
        runtime_ms = (time.perf_counter() - started) * 1000.0
        for s_i in range(n_streams):
            d = chain_diagnostics(rows[:, position[s_i]], lengths, effective[int(stream_preset[s_i])])
            d["candidate_runtime_ms"] = runtime_ms
            results.append(d)
    return output, results


def simulate_auto_eq_chain(audio, sample_rate: float, bands: Sequence[tuple[float, float, float]],
                           settings: Mapping[str, object] | None = None) -> dict[str, Any]:
    """python_api.rs:378-714 -- de-esser -> EQ -> compressor -> limiter -> true-peak limiter."""
    started = time.perf_counter()
    if not np.isfinite(sample_rate) or sample_rate <= 0.0:
        raise ValueError("sample_rate must be positive and finite")
    if len(bands) != NUM_BANDS:
        raise ValueError(f"expected {NUM_BANDS} EQ bands, got {len(bands)}")
    audio = _audio_1d(audio)
    output, results = simulate_auto_eq_chain_batch(audio.reshape(1, -1), sample_rate, bands, settings)
    d = results[0]
    d["candidate_runtime_ms"] = (time.perf_counter() - started) * 1000.0
    if _get(settings, "return_output_audio", False):
        d["output_audio"] = output[0].tolist()  # the reference returns a Python list of floats
    return d


# ----------------------------------------------------------------------- suppressor
TIMING_REPETITIONS = 7  # python/tools/evaluate_limiter_lookahead.py:28 (1 warm-up + 7 timed runs)


def _percentile_f64(values, q: float) -> float:
    v = np.sort(np.asarray(values, dtype=np.float64))
    if v.size == 0:
        return 0.0
    pos = (v.size - 1) * min(max(q, 0.0), 1.0)
    lo, hi = int(np.floor(pos)), int(np.ceil(pos))
    return float(v[lo] + (pos - lo) * (v[hi] - v[lo]))


def suppress(audio: np.ndarray, strength: float = 1.0, weight_seed: int | None = None, raw_protocol: bool = False,
             device: int = 0, kernel_ms: list | None = None) -> np.ndarray:
    """RNNoiseProcessor::process_frames (rust-core/src/dsp/rnnoise.rs:122-164) over [n_streams, n] or [n] audio.

    Only whole 480-sample frames are produced (a shorter tail stays "buffered", as in the reference).
    `raw_protocol=True` is the scaling of bin/rnnoise_benchmark.rs (clamp(+-1)*32768, no wet/dry mix).
    `kernel_ms` (optional list) receives the HIP-event time of the call's kernels.
    """
    a = np.ascontiguousarray(audio, dtype=np.float32)
    squeeze = a.ndim == 1
    if squeeze:
        a = a.reshape(1, -1)
    frames = a.shape[1] // 480
    a = np.ascontiguousarray(a[:, : frames * 480])
    if frames == 0:
        return a[0] if squeeze else a
    engine = Engine(48_000.0, a.shape[0], device)
    try:
        engine.set_eq_enabled(0)
        engine.set_compressor_enabled(0)
        engine.set_limiter_enabled(0)
        engine.set_suppressor_enabled(1)
        engine.set_suppressor_strength(float(strength))
        engine.suppressor_set_raw_protocol(int(raw_protocol))
        if weight_seed is not None:
            engine.suppressor_set_synthetic_weights(int(weight_seed))
        engine.set_control_block_samples(480)
        if kernel_ms is not None:
            engine.set_timing_enabled(1)
        out = engine.process(a)
        if kernel_ms is not None:
            kernel_ms.append(engine.last_kernel_ms()[0])
    finally:
        engine.close()
    return out[0] if squeeze else out


# ------------------------------------------------- NoiseSuppressor (noise_suppressor.rs:18-194)
class NoiseModel:
    """NoiseModel (noise_suppressor.rs:18-87): ids, display names, the models a build offers."""

    RNNOISE, DEEPFILTER_LL, DEEPFILTER = 0, 1, 2

    @staticmethod
    def from_id(model_id: str):
        model = C.c_int32(0)
        rc = _lib.load().af_noise_model_from_id(str(model_id).encode(), C.byref(model))
        return model.value if rc == 0 else None  # Option<NoiseModel>

    @staticmethod
    def id(model: int) -> str:
        return _lib.load().af_noise_model_id(int(model)).decode()

    @staticmethod
    def display_name(model: int) -> str:
        return _lib.load().af_noise_model_display_name(int(model)).decode()

    @staticmethod
    def available() -> list[int]:
        buf = (C.c_int32 * 4)()
        n = _lib.load().af_noise_model_available(buf, 4)
        return [int(buf[i]) for i in range(n)]


class NoiseSuppressor:
    """The `NoiseSuppressor` trait (noise_suppressor.rs:89-165) over a batch of streams that advance in lock step:
    push_samples -> process_frames -> pop_samples_into, with RNNoiseProcessor's two fixed rings (rnnoise.rs:11)."""

    def __init__(self, model: int | str = "rnnoise", n_streams: int = 1, device: int = 0, weight_seed: int | None = None):
        self._lib = _lib.load()
        if isinstance(model, str):
            parsed = NoiseModel.from_id(model)
            if parsed is None:
                raise ValueError(f"unknown noise model id {model!r}")
            model = parsed
        handle = C.c_void_p()
        _lib.check(self._lib.af_noise_suppressor_create(int(model), int(n_streams), int(device), C.byref(handle)))
        self._h = handle
        self.n_streams = int(n_streams)
        if weight_seed is not None:
            _lib.check(self._lib.af_suppressor_set_synthetic_weights(self._lib.af_noise_suppressor_engine(self._h), int(weight_seed)))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_noise_suppressor_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _count(self, value: int) -> int:
        if value < 0:
            _lib.check(int(value))
        return int(value)

    def push_samples(self, samples: np.ndarray) -> int:
        a = np.ascontiguousarray(samples, dtype=np.float32)
        if a.ndim == 1:
            a = a.reshape(1, -1)
        if a.shape[0] != self.n_streams:
            raise ValueError(f"expected {self.n_streams} streams, got {a.shape[0]}")
        return self._count(self._lib.af_noise_suppressor_push_samples(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[1], a.shape[1]))

    def process_frames(self) -> None:
        _lib.check(self._lib.af_noise_suppressor_process_frames(self._h))

    def available_samples(self) -> int:
        return int(self._lib.af_noise_suppressor_available_samples(self._h))

    def pending_input(self) -> int:
        return int(self._lib.af_noise_suppressor_pending_input(self._h))

    def pop_samples(self, count: int) -> np.ndarray:
        count = max(int(count), 0)
        out = np.zeros((self.n_streams, max(count, 1)), dtype=np.float32)
        n = self._count(self._lib.af_noise_suppressor_pop_samples_into(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), count, out.shape[1]))
        return np.ascontiguousarray(out[:, :n])

    def pop_all_samples(self) -> np.ndarray:
        return self.pop_samples(self.available_samples())

    def drain_pending_input(self) -> np.ndarray:
        cap = 8192 + 480
        out = np.zeros((self.n_streams, cap), dtype=np.float32)
        n = self._count(self._lib.af_noise_suppressor_drain_pending_input(self._h, out.ctypes.data_as(C.POINTER(C.c_float)), cap, cap))
        return np.ascontiguousarray(out[:, :n])

    def set_strength(self, value: float) -> None:
        _lib.check(self._lib.af_noise_suppressor_set_strength(self._h, float(value)))

    def get_strength(self) -> float:
        return float(self._lib.af_noise_suppressor_get_strength(self._h))

    def set_enabled(self, enabled: bool) -> None:
        _lib.check(self._lib.af_noise_suppressor_set_enabled(self._h, int(bool(enabled))))

    def is_enabled(self) -> bool:
        return bool(self._lib.af_noise_suppressor_is_enabled(self._h))

    def soft_reset(self) -> None:
        _lib.check(self._lib.af_noise_suppressor_soft_reset(self._h))

    def reset(self) -> None:
        _lib.check(self._lib.af_noise_suppressor_reset(self._h))

    def model_type(self) -> int:
        return int(self._lib.af_noise_suppressor_model_type(self._h))

    def latency_samples(self) -> int:
        return int(self._lib.af_noise_suppressor_latency_samples(self._h))

    def backend_available(self) -> bool:
        return bool(self._lib.af_noise_suppressor_backend_available(self._h))

    def backend_failed(self) -> bool:
        return bool(self._lib.af_noise_suppressor_backend_failed(self._h))

    def backend_error(self):
        msg = self._lib.af_noise_suppressor_backend_error(self._h)
        return msg.decode() if msg else None


def new_noise_suppression_engine(model: int | str, n_streams: int = 1, device: int = 0) -> NoiseSuppressor:
    """new_noise_suppression_engine (noise_suppressor.rs:168-194)."""
    return NoiseSuppressor(model, n_streams, device)


def rnnoise_benchmark(input_path: str, output_path: str, metadata_path: str, weight_seed: int | None = None) -> dict:
    """File protocol of rust-core/src/bin/rnnoise_benchmark.rs:51-117 (`<in.f32> <out.f32> <meta.json>`),
    the boundary python/tools/evaluate_rnnoise_backends.py:106-125 drives."""
    import json

    data = np.fromfile(input_path, dtype="<f4")
    n = data.size
    frames = -(-n // 480)
    padded = np.zeros(frames * 480, dtype=np.float32)
    padded[:n] = data
    # The reference times every frame on the CPU (rnnoise_benchmark.rs:80-96).  A batched engine runs all frames of the
    # file in one pipelined call, so a per-frame clock does not exist; what is measured instead is the whole call, 1 warm-up
    # + TIMING_REPETITIONS fresh runs (HIP events around the call's kernels), each divided by the frame count: the
    # percentiles below are percentiles of those per-run frame times, and `frame_time_basis` says so.
    kernel_ms: list[float] = []
    out = suppress(padded, 1.0, weight_seed, raw_protocol=True) if frames else padded  # warm-up; its output is the result
    for _ in range(TIMING_REPETITIONS if frames else 0):
        suppress(padded, 1.0, weight_seed, raw_protocol=True, kernel_ms=kernel_ms)
    out[:n].astype("<f4").tofile(output_path)
    per_frame = [ms / 1000.0 / frames for ms in kernel_ms] if frames else [0.0]
    elapsed = _percentile_f64(kernel_ms, 0.5) / 1000.0 if frames else 0.0
    meta = {
        "frames": int(frames), "samples": int(n), "elapsed_seconds": elapsed,
        "rtf": elapsed / max(n / 48_000.0, 1e-12),
        "frame_p95_seconds": _percentile_f64(per_frame, 0.95), "frame_p99_seconds": _percentile_f64(per_frame, 0.99),
        "frame_max_seconds": float(max(per_frame)),
        "frame_time_basis": f"whole-call GPU time / frames, percentiles over {TIMING_REPETITIONS} repetitions (median = elapsed_seconds)",
        "repetitions": TIMING_REPETITIONS if frames else 0,
    }
    with open(metadata_path, "w", encoding="utf-8") as fh:
        json.dump(meta, fh)
    return meta


# ------------------------------------------------------ simulate_auto_makeup_control
def simulate_auto_makeup_control(audio, sample_rate: float, vad_probabilities: Sequence[float], noise_floor_db: float,
                                 noise_reliability: float, settings: Mapping[str, object] | None = None) -> dict[str, Any]:
    """python_api.rs:118-276: the compressor's auto-makeup controller at the 10 ms control cadence."""
    control_block = 480
    if not np.isfinite(sample_rate) or sample_rate <= 0.0:
        raise ValueError("sample_rate must be positive and finite")
    if not np.isfinite(noise_floor_db) or not np.isfinite(noise_reliability) or not 0.0 <= noise_reliability <= 1.0:
        raise ValueError("noise evidence must be finite and reliability must be between 0 and 1")
    vad = np.ascontiguousarray(vad_probabilities, dtype=np.float64)
    if vad.size and (not np.all(np.isfinite(vad)) or vad.min() < 0.0 or vad.max() > 1.0):
        raise ValueError("VAD probabilities must be finite and between 0 and 1")
    audio = _audio_1d(audio)
    n = audio.size
    block_count = -(-n // control_block)
    if vad.size and vad.size != block_count:
        raise ValueError(f"expected {block_count} VAD probabilities at the 10 ms control cadence, got {vad.size}")
    vad_reliability = _get(settings, "vad_reliability", 1.0)
    if not np.isfinite(vad_reliability) or not 0.0 <= vad_reliability <= 1.0:
        raise ValueError("vad_reliability must be finite and between 0 and 1")
    run_ms: list[float] = []

    def run_once():
        engine = Engine(sample_rate, 1)
        try:
            return _auto_makeup_run(engine, audio, n, sample_rate, vad, vad_reliability, noise_floor_db, noise_reliability, settings,
                                    control_block, run_ms)
        finally:
            engine.close()

    output, rows = run_once()  # warm-up; its output is the result
    for _ in range(TIMING_REPETITIONS if n else 0):
        run_once()
    run_ms = run_ms[1:] if len(run_ms) > 1 else run_ms
    lengths = _block_lengths(n, control_block).astype(np.float64)
    # The reference clocks every 480-sample block on the CPU (python_api.rs:203-240).  Here all blocks of the clip run in
    # one launch pair, so the figures are per-run block times (run time / blocks) over TIMING_REPETITIONS fresh runs.
    per_block_ms = [ms / max(block_count, 1) for ms in run_ms] or [0.0]
    result: dict[str, Any] = {
        "control_block_size": control_block,
        "control_cadence_hz": sample_rate / control_block,
        "processed_samples": int(n),
        "makeup_gain_db": rows["compressor_makeup_gain_db"].astype(np.float32).tolist(),
        "activity": rows["auto_makeup_activity"].astype(np.float32).tolist(),
        "reliability": rows["auto_makeup_reliability"].astype(np.float32).tolist(),
        "gain_reduction_db": rows["compressor_gain_reduction_db"].astype(np.float32).tolist(),
        "input_rms_db": _linear_to_db(np.sqrt(rows["input_square_sum"] / np.maximum(lengths, 1.0)).astype(np.float32)).tolist(),
        "output_rms_db": _linear_to_db(np.sqrt(rows["output_square_sum"] / np.maximum(lengths, 1.0)).astype(np.float32)).tolist(),
        "p95_block_runtime_ms": _percentile_f64(per_block_ms, 0.95),
        "p99_block_runtime_ms": _percentile_f64(per_block_ms, 0.99),
        "max_block_runtime_ms": float(max(per_block_ms)),
        "block_runtime_basis": f"whole-clip run time / blocks, percentiles over {TIMING_REPETITIONS} repetitions",
    }
    if _get(settings, "return_output_audio", False):
        result["output_audio"] = output.tolist()
    return result


def _auto_makeup_run(engine, audio, n, sample_rate, vad, vad_reliability, noise_floor_db, noise_reliability, settings,
                     control_block, run_ms):
    """One fresh run of the controller (python_api.rs:150-242 setter sequence); appends its wall-clock ms to `run_ms`."""
    engine.set_eq_enabled(0)
    engine.set_limiter_enabled(0)
    engine.set_compressor_enabled(1)
    engine.compressor_set_threshold(_get(settings, "threshold_db", -24.0))
    engine.compressor_set_ratio(_get(settings, "ratio", 3.0))
    engine.compressor_set_attack_time(_get(settings, "attack_ms", 10.0))
    engine.compressor_set_release_time(_get(settings, "release_ms", 180.0))
    engine.compressor_set_makeup_gain(_get(settings, "makeup_gain_db", 0.0))
    engine.compressor_set_auto_makeup_enabled(1)
    engine.compressor_set_target_lufs(_get(settings, "target_lufs", -18.0))
    engine.compressor_set_noise_reference_reliability(float(noise_reliability))
    engine.compressor_set_adaptive_release(int(_get(settings, "adaptive_release", True)))
    engine.compressor_set_sidechain_highpass_enabled(int(_get(settings, "sidechain_highpass_enabled", True)))
    engine.set_control_block_samples(control_block)
    engine.set_input_scrub_enabled(0)
    dp = C.POINTER(C.c_double)
    _lib.check(engine._lib.af_compressor_set_activity_evidence(
        engine._h, vad.ctypes.data_as(dp), int(vad.size), 0, float(vad_reliability), float(noise_floor_db),
        float(noise_reliability)))
    started = time.perf_counter()
    output = engine.process(audio.reshape(1, -1))[0] if n else audio.copy()
    run_ms.append((time.perf_counter() - started) * 1000.0)
    rows = engine.block_stats()[:, 0]
    return output, rows


# -------------------------------------------------------------------- simulate_eq_v2
def simulate_eq_v2(audio, sample_rate: float, bands, return_output_audio: bool = False) -> dict[str, Any]:
    """lib.rs:214-288: typed 10-band EQ over the whole clip, peaks / true peaks / rms."""
    arr = _bands_v2(list(bands), float(sample_rate))
    audio = _audio_1d(audio)
    if not np.all(np.isfinite(audio)):
        raise ValueError("audio must contain only finite samples")
    lib = _lib.load()
    n = audio.size

    def run(eq_enabled: bool) -> tuple[np.ndarray, np.ndarray, Engine]:
        engine = Engine(sample_rate, 1)
        engine.set_limiter_enabled(0)
        engine.set_compressor_enabled(0)
        engine.set_eq_enabled(int(eq_enabled))
        if eq_enabled:
            for index in range(NUM_BANDS):
                _lib.check(lib.af_eq_set_band_config(engine._h, index, C.byref(arr[index])))
            engine.eq_reset()
        engine.set_control_block_samples(8192)
        out = engine.process(audio.reshape(1, -1))[0] if n else audio.copy()
        return out, engine.block_stats()[:, 0], engine

    started = time.perf_counter()
    output, rows, engine = run(True)
    runtime_ms = (time.perf_counter() - started) * 1000.0
    freqs = 20.0 * np.power(20_000.0 / 20.0, np.arange(512, dtype=np.float64) / 511.0)
    response = np.zeros(512, dtype=np.float64)
    dp = C.POINTER(C.c_double)
    _lib.check(lib.af_engine_eq_magnitude_response(engine._h, freqs.ctypes.data_as(dp), 512, response.ctypes.data_as(dp)))
    engine.close()
    # the input true peak is the same detector over the untouched clip (lib.rs:257-260)
    _, in_rows, probe = run(False)
    probe.close()
    divisor = float(max(n, 1))
    in_sq = float(np.sum(in_rows["input_square_sum"])) if n else 0.0
    out_sq = float(np.sum(rows["output_square_sum"])) if n else 0.0
    result: dict[str, Any] = {
        "input_sample_peak": float(in_rows["input_sample_peak"].max()) if n else 0.0,
        "output_sample_peak": float(rows["output_sample_peak"].max()) if n else 0.0,
        "input_true_peak": float(in_rows["output_true_peak"].max()) if n else 0.0,
        "output_true_peak": float(rows["output_true_peak"].max()) if n else 0.0,
        "input_rms": float(np.sqrt(in_sq / divisor)),
        "output_rms": float(np.sqrt(out_sq / divisor)),
        "max_response_db": float(response.max()),
        "runtime_ms": runtime_ms,
        "sample_count": int(n),
        "algorithmic_latency_samples": 0,
        "non_finite_output": bool(not np.all(np.isfinite(output))),
    }
    if return_output_audio:
        result["output_audio"] = output.tolist()
    return result


# ------------------------------------------------------------- eq_magnitude_response
def eq_magnitude_response(frequencies_hz: Sequence[float], bands: Sequence[tuple[float, float, float]],
                          sample_rate: float) -> list[float]:
    """lib.rs:99-150."""
    if len(bands) != NUM_BANDS:
        raise ValueError(f"expected {NUM_BANDS} EQ bands, got {len(bands)}")
    f = np.ascontiguousarray(frequencies_hz, dtype=np.float64)
    b = np.ascontiguousarray(np.asarray(bands, dtype=np.float64).reshape(NUM_BANDS, 3))
    out = np.zeros_like(f)
    dp = C.POINTER(C.c_double)
    _lib.check(_lib.load().af_eq_magnitude_response(f.ctypes.data_as(dp), f.size, b.ctypes.data_as(dp), float(sample_rate),
                                                     out.ctypes.data_as(dp)))
    return out.tolist()


def eq_magnitude_response_v2(frequencies_hz: Sequence[float], bands, sample_rate: float) -> list[float]:
    """lib.rs:191-212."""
    arr = _bands_v2(list(bands), float(sample_rate))
    f = np.ascontiguousarray(frequencies_hz, dtype=np.float64)
    out = np.zeros_like(f)
    dp = C.POINTER(C.c_double)
    _lib.check(_lib.load().af_eq_magnitude_response_v2(f.ctypes.data_as(dp), f.size, arr, float(sample_rate),
                                                        out.ctypes.data_as(dp)))
    return out.tolist()


# ------------------------------------------------------------------ product resampler
RESAMPLER_CHUNK_SIZE = 1024            # audio/processor.rs:53
PRODUCT_RESAMPLER_SINC_LEN = 128       # audio/processor.rs:54
PRODUCT_RESAMPLER_WINDOW_NAME = "blackman"  # audio/processor.rs:55
RESAMPLER_WINDOW_IDS = {"blackman_harris": 0, "blackman_harris_squared": 1, "blackman": 2, "blackman_squared": 3,
                        "hann": 4, "hann_squared": 5}  # resampler_window_from_name, resampling.rs:158-168


def product_resampler_configuration() -> tuple[int, str, str, int, int]:
    """resampling.rs:263-272."""
    return (PRODUCT_RESAMPLER_SINC_LEN, PRODUCT_RESAMPLER_WINDOW_NAME, "cubic", 256, RESAMPLER_CHUNK_SIZE)


class Resampler:
    """One resampling plan (rates, chunk size, sinc length, window) for any number of equally long streams."""

    def __init__(self, input_rate: int, output_rate: int, chunk_size: int = RESAMPLER_CHUNK_SIZE,
                 sinc_len: int | None = None, window: str | None = None, device: int = 0):
        # argument checks in the order of resampling.rs:187-214
        if int(input_rate) <= 0 or int(output_rate) <= 0:
            raise ValueError("sample rates must be positive")
        if not 1 <= int(chunk_size) <= RESAMPLER_CHUNK_SIZE:
            raise ValueError(f"chunk_size must be between 1 and {RESAMPLER_CHUNK_SIZE}")
        sinc_len = PRODUCT_RESAMPLER_SINC_LEN if sinc_len is None else int(sinc_len)
        if not 32 <= sinc_len <= 2048 or sinc_len & (sinc_len - 1):
            raise ValueError("sinc_len must be a power of two between 32 and 2048")
        name = PRODUCT_RESAMPLER_WINDOW_NAME if window is None else window
        if name not in RESAMPLER_WINDOW_IDS:
            raise ValueError(f"unsupported resampler window {name!r}")
        self._lib = _lib.load()
        handle = C.c_void_p()
        _lib.check(self._lib.af_resampler_create(int(input_rate), int(output_rate), int(chunk_size), sinc_len,
                                                 RESAMPLER_WINDOW_IDS[name], int(device), C.byref(handle)))
        self._h = handle
        self.input_rate, self.output_rate, self.sinc_len = int(input_rate), int(output_rate), sinc_len

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_resampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def output_delay(self) -> int:
        return int(self._lib.af_resampler_output_delay(self._h))

    def expected_frames(self, n_in: int) -> int:
        return int(self._lib.af_resampler_expected_frames(self._h, int(n_in)))

    def plan(self, n_in: int) -> tuple[int, int]:
        """(frames the reference's driver loop returns for n_in input frames, number of chunks it runs)."""
        n_out, blocks = C.c_int64(0), C.c_int64(0)
        _lib.check(self._lib.af_resampler_plan(self._h, int(n_in), C.byref(n_out), C.byref(blocks)))
        return n_out.value, blocks.value

    def sinc_table(self) -> np.ndarray:
        table = np.zeros((256, int(self._lib.af_resampler_sinc_len(self._h))), dtype=np.float64)
        _lib.check(self._lib.af_resampler_copy_sinc_table(self._h, table.ctypes.data_as(C.POINTER(C.c_double))))
        return table

    def process(self, samples: np.ndarray) -> np.ndarray:
        """[n_streams, n_in] (or [n_in]) float64 host array -> [n_streams, n_out]."""
        x = np.ascontiguousarray(samples, dtype=np.float64)
        squeeze = x.ndim == 1
        if squeeze:
            x = x.reshape(1, -1)
        n_streams, n_in = x.shape
        n_out, _ = self.plan(n_in)
        out = np.zeros((n_streams, n_out), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        _lib.check(self._lib.af_resampler_process_host(self._h, x.ctypes.data_as(dp), out.ctypes.data_as(dp), n_in, n_streams,
                                                       max(n_in, 1), max(n_out, 1) if n_out == 0 else n_out))
        return out[0] if squeeze else out

    def process_device(self, in_ptr: int, out_ptr: int, n_in: int, n_streams: int, in_stride: int, out_stride: int,
                       hip_stream: int = 0) -> None:
        _lib.check(self._lib.af_resampler_process_device(self._h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), int(n_in),
                                                         int(n_streams), int(in_stride), int(out_stride), C.c_void_p(hip_stream)))

    def last_kernel_ms(self) -> float:
        ms = C.c_double(0.0)
        _lib.check(self._lib.af_resampler_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    @property
    def launch_form(self) -> tuple[int, int, int]:
        """(form, segment_outputs, streams_per_workgroup) of the kernel ``process`` launches: form 0 is the vector body,
        1 the matrix-core body.  Host only; the launcher's own choice (ratio, sinc length, AF_RESAMPLER_VARIANT at create)."""
        form, seg, streams = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.af_resampler_launch_form(self._h, C.byref(form), C.byref(seg), C.byref(streams)))
        return form.value, seg.value, streams.value


class StreamResampler:
    """The product resampler as the realtime loop drives it (dsp_loop.rs:963-1011): `n_streams` streams in lock step, state
    carried across pushes, float32 in and out.  A push returns the frames of the chunks it completed (possibly none)."""

    def __init__(self, input_rate: int, output_rate: int, n_streams: int = 1, chunk_size: int = RESAMPLER_CHUNK_SIZE,
                 sinc_len: int | None = None, window: str | None = None, device: int = 0):
        sinc_len = PRODUCT_RESAMPLER_SINC_LEN if sinc_len is None else int(sinc_len)
        name = PRODUCT_RESAMPLER_WINDOW_NAME if window is None else window
        # (the library checks the rest of the contract of resampling.rs:187-214, in its order; window names live here)
        window_id = RESAMPLER_WINDOW_IDS.get(name, -1)
        if int(input_rate) < 0 or int(output_rate) < 0:
            raise ValueError("sample rates must be positive")
        self._lib = _lib.load()
        handle = C.c_void_p()
        rc = self._lib.af_stream_resampler_create(int(input_rate), int(output_rate), int(chunk_size), sinc_len, window_id,
                                                  int(n_streams), int(device), C.byref(handle))
        if rc == _lib.AF_ERR_INVALID_ARGUMENT and window_id < 0 and "window" in _lib.last_error():
            raise ValueError(f"unsupported resampler window {name!r}")
        _lib.check(rc)
        self._h = handle
        self.input_rate, self.output_rate, self.n_streams = int(input_rate), int(output_rate), int(n_streams)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_stream_resampler_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def output_frames(self, n_in: int) -> int:
        """Frames per stream the next push of n_in frames would produce (host replay, changes nothing)."""
        return int(self._lib.af_stream_resampler_output_frames(self._h, int(n_in)))

    @property
    def pending_input(self) -> int:
        return int(self._lib.af_stream_resampler_pending_input(self._h))

    @property
    def output_delay(self) -> int:
        return int(self._lib.af_stream_resampler_output_delay(self._h))

    @property
    def frames_in(self) -> int:
        return int(self._lib.af_stream_resampler_frames_in(self._h))

    @property
    def frames_out(self) -> int:
        return int(self._lib.af_stream_resampler_frames_out(self._h))

    def reset(self) -> None:
        _lib.check(self._lib.af_stream_resampler_reset(self._h))

    def clear_pending(self) -> None:
        _lib.check(self._lib.af_stream_resampler_clear_pending(self._h))

    def push(self, x: np.ndarray, out_capacity: int | None = None) -> np.ndarray:
        """float32 [n_streams, n] (or [n] for one stream) -> float32 [n_streams, m]."""
        a = np.ascontiguousarray(x, dtype=np.float32)
        if a.ndim == 1:
            a = a.reshape(1, -1)
        if a.shape[0] != self.n_streams:
            raise ValueError(f"expected {self.n_streams} streams, got {a.shape[0]}")
        n = a.shape[1]
        cap = self.output_frames(n) if out_capacity is None else int(out_capacity)
        out = np.empty((self.n_streams, max(cap, 1)), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        n_out = C.c_int64(0)
        _lib.check(self._lib.af_stream_resampler_push_host(self._h, a.ctypes.data_as(fp), n, max(n, 1), out.ctypes.data_as(fp), cap,
                                                           out.shape[1], C.byref(n_out)))
        return np.ascontiguousarray(out[:, : n_out.value])

    def push_device(self, in_ptr: int, n_in: int, in_stride: int, out_ptr: int, out_capacity: int, out_stride: int,
                    hip_stream: int = 0) -> int:
        """Device pointers, asynchronous on ``hip_stream``; returns the frames per stream the push produces.  The input
        must be finite: nothing on the device checks it."""
        n_out = C.c_int64(0)
        _lib.check(self._lib.af_stream_resampler_push_device(self._h, C.c_void_p(in_ptr), int(n_in), int(in_stride), C.c_void_p(out_ptr),
                                                             int(out_capacity), int(out_stride), C.byref(n_out), C.c_void_p(hip_stream)))
        return n_out.value

    def last_kernel_ms(self) -> float:
        ms = C.c_double(0.0)
        _lib.check(self._lib.af_stream_resampler_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    @property
    def launch_form(self) -> tuple[int, int, int]:
        """As ``Resampler.launch_form``, for the kernel a push launches."""
        form, seg, streams = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _lib.check(self._lib.af_stream_resampler_launch_form(self._h, C.byref(form), C.byref(seg), C.byref(streams)))
        return form.value, seg.value, streams.value


INPUT_CHANNEL_MODE_IDS = {"average": 0, "left": 1, "right": 2, "max_rms": 3, "phase_safe_mono": 4}  # input.rs:158-180
PHASE_RESCUE_STRATEGY_NAMES = ("none", "polarity_flip", "fractional_delay", "max_rms_fallback")  # input.rs:49-56


def input_channel_mode(mode) -> int:
    """An InputChannelMode id (input.rs:158-180) or number -> the number; anything else is a ValueError."""
    if isinstance(mode, str):
        if mode not in INPUT_CHANNEL_MODE_IDS:
            raise ValueError(f"unknown input channel mode {mode!r}; expected one of {sorted(INPUT_CHANNEL_MODE_IDS)}")
        return INPUT_CHANNEL_MODE_IDS[mode]
    if isinstance(mode, (bool, float)) or not isinstance(mode, (int, np.integer)):
        raise ValueError(f"unknown input channel mode {mode!r}")
    return int(mode)


def _read_phase(fn, handle, n_streams: int) -> dict:
    corr = np.empty(n_streams, dtype=np.float32)
    warn = np.empty(n_streams, dtype=np.uint64)
    strategy = np.empty(n_streams, dtype=np.int32)
    delay = np.empty(n_streams, dtype=np.float32)
    flipped = np.empty(n_streams, dtype=np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    _lib.check(fn(handle, corr.ctypes.data_as(fp), warn.ctypes.data_as(C.POINTER(C.c_uint64)), strategy.ctypes.data_as(ip),
                  delay.ctypes.data_as(fp), flipped.ctypes.data_as(ip), int(n_streams)))
    return dict(stereo_correlation=corr, phase_warning_count=warn, strategy=strategy, estimated_delay=delay,
                polarity_flipped=flipped.astype(bool))


class Mixdown:
    """The capture callback's mixdown (input.rs:383-736, 785-843) for `n_streams` streams: interleaved frames of
    `n_channels` channels -> mono, bit-exact with the reference's f32 arithmetic.  A push is one callback; the mode is live."""

    def __init__(self, n_channels: int, mode="average", n_streams: int = 1, device: int = 0):
        self._lib = _lib.load()
        handle = C.c_void_p()
        _lib.check(self._lib.af_mixdown_create(int(n_channels), input_channel_mode(mode), int(n_streams), int(device), C.byref(handle)))
        self._h = handle
        self.n_channels, self.n_streams = int(n_channels), int(n_streams)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_mixdown_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_mode(self, mode) -> None:
        _lib.check(self._lib.af_mixdown_set_mode(self._h, input_channel_mode(mode)))

    @property
    def mode(self) -> int:
        return int(self._lib.af_mixdown_mode(self._h))

    def push(self, x: np.ndarray) -> np.ndarray:
        """float32 [n_streams, n, n_channels] (or [n, n_channels] for one stream) -> float32 [n_streams, n]."""
        a = np.ascontiguousarray(x, dtype=np.float32)
        if a.ndim == 2 and self.n_streams == 1:
            a = a.reshape(1, *a.shape)
        if a.ndim != 3 or a.shape[0] != self.n_streams or a.shape[2] != self.n_channels:
            raise ValueError(f"expected [{self.n_streams}, frames, {self.n_channels}] interleaved frames, got shape {a.shape}")
        n = a.shape[1]
        out = np.empty((self.n_streams, max(n, 1)), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(self._lib.af_mixdown_push_host(self._h, a.ctypes.data_as(fp), n, n, out.ctypes.data_as(fp), out.shape[1]))
        return np.ascontiguousarray(out[:, :n])

    def push_device(self, in_ptr: int, n_frames: int, in_stride_frames: int, out_ptr: int, out_stride: int, hip_stream: int = 0) -> None:
        """Device pointers, asynchronous on ``hip_stream``: in[(s * in_stride_frames + t) * n_channels + c] ->
        out[s * out_stride + t].  The input must be finite: nothing on the device checks it."""
        _lib.check(self._lib.af_mixdown_push_device(self._h, C.c_void_p(in_ptr), int(n_frames), int(in_stride_frames),
                                                    C.c_void_p(out_ptr), int(out_stride), C.c_void_p(hip_stream)))

    def diagnostics(self) -> dict:
        """Arrays per stream: stereo_correlation (NaN until a first one), phase_warning_count, strategy
        (PHASE_RESCUE_STRATEGY_NAMES), estimated_delay, polarity_flipped."""
        return _read_phase(self._lib.af_mixdown_read_diagnostics, self._h, self.n_streams)

    def reset(self) -> None:
        _lib.check(self._lib.af_mixdown_reset(self._h))

    def last_kernel_ms(self) -> tuple[float, float]:
        """(decision passes, mix passes) of the last push, from HIP events."""
        a, b = C.c_double(0.0), C.c_double(0.0)
        _lib.check(self._lib.af_mixdown_last_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


class OutputWriterConfig(C.Structure):
    """af_output_writer_config: the limits of output_writer.rs:20-27 and the queue's capacity."""
    _fields_ = [("output_rate", C.c_int32), ("queue_capacity", C.c_int64), ("target_center", C.c_int64),
                ("hard_backlog", C.c_int64), ("fade_frames", C.c_int64)]


OUTPUT_WRITER_COUNTERS = ("jitter_dropped", "retime_adjustments", "recovery_events", "short_write_dropped", "clip_events",
                          "true_peak_events")  # output_writer.rs:2-5, 10, 12
OUTPUT_WRITER_DB = ("clip_peak_db", "true_peak_db", "true_peak_input_db", "gain_reduction_db", "gain_reduction_history_db",
                    "headroom_db")  # output_writer.rs:11-17
OUTPUT_WRITER_LINEAR = ("input_true_peak", "limiter_output_true_peak", "detector_true_peak", "min_gain", "max_clipped")


def _read_writer_counters(fn, handle, n: int) -> dict:
    rows = np.zeros((6, n), dtype=np.uint64)
    up = C.POINTER(C.c_uint64)
    _lib.check(fn(handle, *[rows[k].ctypes.data_as(up) for k in range(6)], n))
    return dict(zip(OUTPUT_WRITER_COUNTERS, rows))


def _read_writer_meters(fn, handle, n: int) -> dict:
    db, lin = np.zeros((6, n), dtype=np.float32), np.zeros((5, n), dtype=np.float32)
    ratio, ema = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    out_len, fade, fill = (np.zeros(n, dtype=np.int64) for _ in range(3))
    fp, lp = C.POINTER(C.c_float), C.POINTER(C.c_int64)
    _lib.check(fn(handle, db.ctypes.data_as(fp), lin.ctypes.data_as(fp), ratio.ctypes.data_as(fp), ema.ctypes.data_as(fp),
                  out_len.ctypes.data_as(lp), fade.ctypes.data_as(lp), fill.ctypes.data_as(lp), n))
    m = dict(zip(OUTPUT_WRITER_DB, db))
    m.update(zip(OUTPUT_WRITER_LINEAR, lin))
    m.update(ratio=ratio, ema=ema, out_len=out_len, fade_remaining=fade, fill_after=fill)
    return m


def output_writer_default_config(output_rate: int) -> dict:
    """The limits dsp_loop.rs:781-795 derives from the output rate, and the queue capacity of :204."""
    cfg = OutputWriterConfig()
    _lib.check(_lib.load().af_output_writer_default_config(int(output_rate), C.byref(cfg)))
    return {name: int(getattr(cfg, name)) for name, _ in OutputWriterConfig._fields_}


class OutputWriter:
    """The output writer (output_writer.rs:62-343) for `n_streams` streams: drift retime, discontinuity fade, safety
    limiter and the queue write's accounting, bit-exact with the reference's f32 arithmetic.  A push is one write_chunk
    per stream; the caller reports each stream's queue fill and gets ragged rows back."""

    def __init__(self, output_rate: int = 48_000, n_streams: int = 1, device: int = 0, queue_capacity: int | None = None,
                 target_center: int | None = None, hard_backlog: int | None = None, fade_frames: int | None = None):
        self._lib = _lib.load()
        cfg = OutputWriterConfig()
        _lib.check(self._lib.af_output_writer_default_config(int(output_rate), C.byref(cfg)))
        for name, value in (("queue_capacity", queue_capacity), ("target_center", target_center), ("hard_backlog", hard_backlog),
                            ("fade_frames", fade_frames)):
            if value is not None:
                setattr(cfg, name, int(value))
        handle = C.c_void_p()
        _lib.check(self._lib.af_output_writer_create(C.byref(cfg), int(n_streams), int(device), C.byref(handle)))
        self._h = handle
        self.n_streams = int(n_streams)
        self.config = {name: int(getattr(cfg, name)) for name, _ in OutputWriterConfig._fields_}

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_output_writer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_limiter(self, enabled: bool, ceiling_linear: float = 1.0) -> None:
        """Live, read at each push (output_writer.rs:208-215)."""
        _lib.check(self._lib.af_output_writer_set_limiter(self._h, int(bool(enabled)), float(ceiling_linear)))

    def reset(self) -> None:
        _lib.check(self._lib.af_output_writer_reset(self._h))

    def max_output_frames(self, n_in: int) -> int:
        return int(self._lib.af_output_writer_max_output_frames(self._h, int(n_in)))

    def _fill(self, fill) -> np.ndarray:
        f = np.ascontiguousarray(np.broadcast_to(np.asarray(fill), (self.n_streams,)) if np.ndim(fill) == 0 else fill)
        if f.shape != (self.n_streams,) or not np.issubdtype(f.dtype, np.integer):
            raise ValueError(f"fill must be {self.n_streams} integers (frames in each stream's queue)")
        return np.ascontiguousarray(f, dtype=np.int64)

    def push(self, x: np.ndarray, fill, clean_path: bool = False) -> tuple[np.ndarray, np.ndarray]:
        """float32 [n_streams, n] (or [n] for one stream) and fill[n_streams] -> (rows [n_streams, max_output_frames(n)],
        written[n_streams]): row s holds written[s] frames and zeros behind them."""
        a = np.ascontiguousarray(x, dtype=np.float32)
        if a.ndim == 1 and self.n_streams == 1:
            a = a.reshape(1, -1)
        if a.ndim != 2 or a.shape[0] != self.n_streams:
            raise ValueError(f"expected [{self.n_streams}, frames] samples, got shape {a.shape}")
        f = self._fill(fill)
        n = a.shape[1]
        width = max(self.max_output_frames(n), 1)
        out = np.zeros((self.n_streams, width), dtype=np.float32)
        written = np.zeros(self.n_streams, dtype=np.int64)
        fp, lp = C.POINTER(C.c_float), C.POINTER(C.c_int64)
        _lib.check(self._lib.af_output_writer_push_host(self._h, a.ctypes.data_as(fp), n, n, f.ctypes.data_as(lp),
                                                        int(bool(clean_path)), out.ctypes.data_as(fp), width, width,
                                                        written.ctypes.data_as(lp)))
        return out, written

    def push_device(self, in_ptr: int, n_in: int, in_stride: int, fill_ptr: int, clean_path: bool, out_ptr: int,
                    out_capacity: int, out_stride: int, written_ptr: int, hip_stream: int = 0) -> None:
        """Device pointers (fill and written are int64 arrays), asynchronous on ``hip_stream``."""
        _lib.check(self._lib.af_output_writer_push_device(self._h, C.c_void_p(in_ptr), int(n_in), int(in_stride), C.c_void_p(fill_ptr),
                                                          int(bool(clean_path)), C.c_void_p(out_ptr), int(out_capacity),
                                                          int(out_stride), C.c_void_p(written_ptr), C.c_void_p(hip_stream)))

    def counters(self) -> dict:
        """Arrays per stream of the running counts (OUTPUT_WRITER_COUNTERS)."""
        return _read_writer_counters(self._lib.af_output_writer_read_counters, self._h, self.n_streams)

    def meters(self) -> dict:
        """Arrays per stream: the dB fields (OUTPUT_WRITER_DB), the last push's linear statistics (OUTPUT_WRITER_LINEAR), its
        ratio, the drift EMA, out_len, fade_remaining and the modelled fill after the write."""
        return _read_writer_meters(self._lib.af_output_writer_read_meters, self._h, self.n_streams)

    def state(self) -> dict:
        """Test read-out: the limiter's gain [n], delay line [n, 20] and write index [n], the histories [n, 3, 32]."""
        n = self.n_streams
        gain, delay = np.zeros(n, dtype=np.float32), np.zeros((n, 20), dtype=np.float32)
        widx, hist = np.zeros(n, dtype=np.int32), np.zeros((n, 3, 32), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(self._lib.af_output_writer_read_state(self._h, gain.ctypes.data_as(fp), delay.ctypes.data_as(fp),
                                                         widx.ctypes.data_as(C.POINTER(C.c_int32)), hist.ctypes.data_as(fp), n))
        return dict(gain=gain, delay=delay, write_idx=widx, histories=hist)

    def last_kernel_ms(self) -> float:
        """All passes of the last push, from HIP events."""
        ms = C.c_double(0.0)
        _lib.check(self._lib.af_output_writer_last_kernel_ms(self._h, C.byref(ms)))
        return ms.value

    def last_pass_ms(self) -> list[float]:
        """(plan, shape, gain, out, finish) of the last push, from HIP events; gain is 0 with the limiter off."""
        ms = (C.c_double * 5)()
        _lib.check(self._lib.af_output_writer_last_pass_ms(self._h, ms))
        return list(ms)


def simulate_product_resampler_batch(samples: np.ndarray, input_rate: int, output_rate: int,
                                     chunk_size: int = RESAMPLER_CHUNK_SIZE, sinc_len: int | None = None,
                                     window: str | None = None, repetitions: int = 0):
    """Batched form: samples [n_streams, n] -> (output [n_streams, n_out] f64, delay, expected_frames, blocks, kernel ms).

    `repetitions` > 0 re-runs the launch that many times and returns the list of their HIP-event times instead of one."""
    r = Resampler(input_rate, output_rate, chunk_size, sinc_len, window)
    try:
        x = np.asarray(samples, dtype=np.float64)
        if not np.all(np.isfinite(x)):
            raise ValueError("samples must be finite")
        out = r.process(x)
        _, blocks = r.plan(x.shape[-1])
        kernel_ms = [r.last_kernel_ms()]
        for _ in range(int(repetitions)):  # the resampler is stateless across calls: re-running is a pure timing repeat
            r.process(x)
            kernel_ms.append(r.last_kernel_ms())
        timing = kernel_ms[1:] if repetitions else kernel_ms[0]
        return out, r.output_delay, r.expected_frames(x.shape[-1]), blocks, timing
    finally:
        r.close()


def simulate_product_resampler(samples: Sequence[float], input_rate: int, output_rate: int,
                               chunk_size: int = RESAMPLER_CHUNK_SIZE, sinc_len: int | None = None,
                               window: str | None = None) -> tuple[list[float], int, int, list[int]]:
    """resampling.rs:170-261: (output, delay, expected_frames, block_times_ns).

    The reference clocks each 1024-frame chunk on the CPU; here all chunks run in ONE launch, so a per-chunk clock does
    not exist.  The launch is timed TIMING_REPETITIONS times (HIP events, after one warm-up); entry i of block_times_ns is
    repetition (i mod TIMING_REPETITIONS)'s time divided by the number of chunks, so the percentiles the harness takes over
    the list (evaluate_resampler_quality.py `runtime` block) are percentiles over real, separately timed launches."""
    x = np.ascontiguousarray(samples, dtype=np.float64).reshape(-1)
    out, delay, expected, blocks, kernel_ms = simulate_product_resampler_batch(x.reshape(1, -1), input_rate, output_rate,
                                                                             chunk_size, sinc_len, window,
                                                                             repetitions=TIMING_REPETITIONS)
    per_block = [int(round(ms * 1e6 / max(blocks, 1))) for ms in kernel_ms]
    return out[0].tolist(), int(delay), int(expected), [per_block[i % len(per_block)] for i in range(int(blocks))]


# ------------------------------------------------------------------ integrated loudness
LOUDNESS_SAMPLE_RATES = (8000, 16000, 32000, 44100, 48000, 88200, 96000)  # loudness.rs:36-41


def measure_integrated_loudness_batch(audio: np.ndarray, sample_rate: int, device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """[n_streams, n] float32 -> (LUFS per stream, status per stream: 0 ok, -3 non-finite, -5 nothing passed the gates)."""
    a = np.ascontiguousarray(audio, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError("audio must be [n_streams, n]")
    if int(sample_rate) not in LOUDNESS_SAMPLE_RATES:
        raise ValueError(f"Invalid sample rate: {sample_rate}")
    if a.shape[1] == 0:
        raise ValueError("Invalid audio: at least one sample is required")
    lufs = np.zeros(a.shape[0], dtype=np.float64)
    status = np.zeros(a.shape[0], dtype=np.int32)
    rc = _lib.load().af_measure_integrated_loudness_host(a.ctypes.data_as(C.POINTER(C.c_float)), a.shape[1], a.shape[0], a.shape[1],
                                                         int(sample_rate), int(device), lufs.ctypes.data_as(C.POINTER(C.c_double)),
                                                         status.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc == _lib.AF_ERR_BACKEND:
        _lib.check(rc)
    return lufs, status


def measure_integrated_loudness(audio, sample_rate: int) -> float:
    """lib.rs:290-298: gated BS.1770 loudness (LUFS) of one clip; ValueError like the reference's PyValueError."""
    a = _audio_1d(audio)
    if int(sample_rate) not in LOUDNESS_SAMPLE_RATES:
        raise ValueError(f"Invalid sample rate: {sample_rate}")
    if a.size == 0:
        raise ValueError("Invalid audio: at least one sample is required")
    lufs, status = measure_integrated_loudness_batch(a.reshape(1, -1), sample_rate)
    if status[0] == _lib.AF_ERR_NON_FINITE:
        raise ValueError("Invalid audio: samples must be finite")
    if status[0] != 0:
        raise ValueError("Loudness measurement failed: audio did not produce a finite gated loudness")
    return float(lufs[0])


# ------------------------------------------------------------------ noise gate + suppressor order
RNNOISE_FRAME = 480  # dsp/rnnoise.rs:3


def gate_batch(audio: np.ndarray, threshold_db: float = -40.0, attack_ms: float = 10.0, release_ms: float = 100.0,
               sample_rate: float = 48_000.0, vad_mode: bool = True, trace_block: int = RNNOISE_FRAME, device: int = 0):
    """NoiseGate expander path (gate.rs:626-637) over [n_streams, n]: (output, gain trace [blocks, n_streams], chatter events)."""
    a = np.ascontiguousarray(audio, dtype=np.float32)
    if a.ndim != 2:
        raise ValueError("audio must be [n_streams, n]")
    n_streams, n = a.shape
    out = np.empty_like(a)
    blocks = -(-n // trace_block)
    trace = np.zeros((blocks, n_streams), dtype=np.float32)
    chatter = np.zeros(n_streams, dtype=np.uint64)
    fp = C.POINTER(C.c_float)
    _lib.check(_lib.load().af_gate_process_host(a.ctypes.data_as(fp), out.ctypes.data_as(fp), n, n_streams, n, float(threshold_db),
                                                float(attack_ms), float(release_ms), float(sample_rate), int(bool(vad_mode)),
                                                int(trace_block), trace.ctypes.data_as(fp),
                                                chatter.ctypes.data_as(C.POINTER(C.c_uint64)), int(device)))
    return out, trace, chatter


def simulate_gate_suppressor_order(audio, vad_probabilities: Sequence[float], suppressor_before_gate: bool,
                                   suppressor_strength: float = 1.0, settings: Mapping[str, object] | None = None) -> dict[str, Any]:
    """python_api.rs:288-376: gate (VadAssisted, no VadAutoGate attached) and RNNoise in either order, 480-sample frames."""
    import time

    strength = float(suppressor_strength)
    if not np.isfinite(strength) or not 0.0 <= strength <= 1.0:
        raise ValueError("suppressor_strength must be finite and between 0 and 1")
    x = _audio_1d(audio)
    n = x.size
    frames = -(-n // RNNOISE_FRAME)
    probs = np.asarray(list(vad_probabilities), dtype=np.float64)
    if probs.size != frames or not np.all(np.isfinite(probs)) or np.any(probs < 0.0) or np.any(probs > 1.0):
        raise ValueError(f"expected {frames} finite VAD probabilities at the 10 ms RNNoise cadence")
    started = time.perf_counter()
    padded = np.zeros((1, frames * RNNOISE_FRAME), dtype=np.float32)
    padded[0, :n] = x
    gate_args = (_get(settings, "gate_threshold_db", -40.0), _get(settings, "gate_attack_ms", 10.0),
                 _get(settings, "gate_release_ms", 100.0), 48_000.0, True, RNNOISE_FRAME)
    if frames == 0:
        out, trace, chatter = padded, np.zeros((0, 1), np.float32), np.zeros(1, np.uint64)
    elif suppressor_before_gate:
        out, trace, chatter = gate_batch(suppress(padded, strength), *gate_args)
    else:
        gated, trace, chatter = gate_batch(padded, *gate_args)
        out = suppress(gated, strength)
    return {
        "output_audio": out[0, :n].tolist(),
        "gate_gain": [float(v) for v in trace[:, 0]],
        "gate_chatter_event_count": int(chatter[0]),
        "gate_noise_floor_db": -60.0,            # NoiseGate::noise_floor() without a VadAutoGate, gate.rs:929-934
        "gate_noise_floor_reliability": 0.0,     # gate.rs:938-943
        "suppressor_latency_samples": RNNOISE_FRAME,  # rnnoise.rs:313-315
        "runtime_ms": (time.perf_counter() - started) * 1000.0,
    }


# ------------------------------------------------------------------ voice spectrum measurement
NOISE_REFERENCE_SOURCES = ("unavailable", "explicit_capture", "in_capture_non_speech", "validated_conservative")  # spectrum.py:553-586


class VoiceSpectrum:
    """python/mic_eq/analysis/spectrum.py for a batch of captures on the device: frame levels, voiced frames (optionally fused
    with a VAD posterior), Hamming-windowed spectra, the Welch spectrum, median speech and noise spectra, per-bin SNR and the
    perceptual smoothing of the voiced windows.  One object per (sample rate, nperseg); scratch is kept between calls."""

    def __init__(self, sample_rate: int = 48_000, nperseg: int = 4096, device: int = 0):
        self._lib = _lib.load()
        handle = C.c_void_p()
        _lib.check(self._lib.af_voice_spectrum_create(int(sample_rate), int(nperseg), int(device), C.byref(handle)))
        self._h = handle
        self.sample_rate, self.nperseg = int(sample_rate), int(nperseg)
        self.bins = int(self._lib.af_voice_spectrum_bins(handle))
        self.freqs = np.arange(self.bins) * (1.0 / (self.nperseg * (1.0 / self.sample_rate)))  # np.fft.rfftfreq

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_voice_spectrum_destroy(self._h)
            self._h = None

    __del__ = close

    def frames(self, n_samples: int) -> int:
        return int(self._lib.af_voice_spectrum_frames(self._h, int(n_samples)))

    def smooth(self, spectra_db) -> np.ndarray:
        """smooth_spectrum_perceptual "balanced" (spectrum.py:949-967) of spectra_db [n, bins] (or one [bins]) on this
        object's grid, on the device: the pass every voiced window goes through."""
        rows = np.ascontiguousarray(np.atleast_2d(spectra_db), dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != self.bins or rows.shape[0] == 0:
            raise ValueError(f"spectra_db must be [n, {self.bins}]")
        out = np.empty_like(rows)
        dp = C.POINTER(C.c_double)
        _lib.check(self._lib.af_voice_spectrum_smooth_rows(self._h, rows.ctypes.data_as(dp), rows.shape[0], out.ctypes.data_as(dp)))
        return out if np.ndim(spectra_db) == 2 else out[0]

    def set_noise_override(self, noise_override=None) -> None:
        """noise_spectrum_override of spectrum.py:554-569 for the calls that follow: (freqs [n], spectrum_db [n] for every stream
        or [n_streams, n]), or None to clear it.  A stream whose override is not at least two finite points falls through."""
        dp = C.POINTER(C.c_double)
        if noise_override is None:
            _lib.check(self._lib.af_voice_spectrum_set_noise_override(self._h, None, None, 0, 0, 0, 0))
            return
        freqs = np.ascontiguousarray(noise_override[0], dtype=np.float64)
        spectrum = np.ascontiguousarray(noise_override[1], dtype=np.float64)
        if freqs.ndim != 1 or spectrum.ndim not in (1, 2) or spectrum.shape[-1] != freqs.size or freqs.size == 0:
            raise ValueError("noise_override must be (freqs [n], spectrum_db [n] or [n_streams, n]) with n >= 1")
        shared = spectrum.ndim == 1
        _lib.check(self._lib.af_voice_spectrum_set_noise_override(self._h, freqs.ctypes.data_as(dp), spectrum.ctypes.data_as(dp), freqs.size,
                                                                  1 if shared else spectrum.shape[0], freqs.size, int(shared)))

    def analyze(self, audio, vad_probabilities=None, noise_audio=None, keep_windows: bool = False, device_pointers=None,
                reliability: bool = False, noise_override=None) -> dict:
        """audio [n_streams, n] float32 (host), or with `device_pointers=(d_audio, n, n_streams, stride[, d_noise, n_noise,
        noise_stride])` device memory.  Returns arrays by field: the scalars of af_voice_spectrum_row as [n_streams] arrays,
        spectra [n_streams, bins] (NaN rows where the reference returns None), frame levels and masks [n_streams, frames].
        `reliability` also computes the second half of analyze_voice_spectrum (spectrum.py:647-742) for reliability().
        `noise_override`: see set_noise_override; it holds for this call only (None leaves none set)."""
        dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        self.set_noise_override(noise_override)
        vad = None if vad_probabilities is None else np.ascontiguousarray(vad_probabilities, dtype=np.float64)
        if device_pointers is None:
            a = np.ascontiguousarray(audio, dtype=np.float32)
            if a.ndim != 2:
                raise ValueError("audio must be [n_streams, n]")
            B, n = a.shape
            noise = None if noise_audio is None else np.ascontiguousarray(noise_audio, dtype=np.float32)
            if noise is not None and (noise.ndim != 2 or noise.shape[0] != B):
                raise ValueError("noise_audio must be [n_streams, n_noise]")
        else:
            B, n = int(device_pointers[2]), int(device_pointers[1])
        if vad is not None and (vad.ndim != 2 or vad.shape[0] != B):
            raise ValueError("vad_probabilities must be [n_streams, n_vad]")
        if n < self.nperseg:
            raise ValueError(f"Audio too short for FFT: need {self.nperseg} samples, got {n} ({n / self.sample_rate:.2f} seconds)")
        F, K = self.frames(n), self.bins
        _lib.check(self._lib.af_voice_spectrum_set_reliability(self._h, int(bool(reliability))))
        self._last_shape = (B, F)
        rows = (_lib.VoiceSpectrumRow * B)()
        out = {name: np.empty((B, K)) for name in ("speech_db", "noise_db", "spectral_snr_db", "welch_db", "welch_sum")}
        out.update(frame_power=np.empty((B, F)), frame_rms_db=np.empty((B, F)), voiced_mask=np.empty((B, F), dtype=np.uint8))
        o = _lib.VoiceSpectrumOutputs(rows=rows, keep_windows=int(bool(keep_windows)),
                                      voiced_mask=out["voiced_mask"].ctypes.data_as(C.POINTER(C.c_uint8)),
                                      **{k: v.ctypes.data_as(dp) for k, v in out.items() if k != "voiced_mask"})
        vad_args = (None, 0) if vad is None else (vad.ctypes.data_as(dp), vad.shape[1])
        if device_pointers is None:
            noise_args = (None, 0, 0) if noise is None else (noise.ctypes.data_as(fp), noise.shape[1], noise.shape[1])
            rc = self._lib.af_voice_spectrum_analyze_host(self._h, a.ctypes.data_as(fp), n, B, n, *vad_args, *noise_args, C.byref(o))
        else:
            d_audio, _, _, stride = device_pointers[:4]
            noise_args = tuple(device_pointers[4:7]) if len(device_pointers) >= 7 else (None, 0, 0)
            rc = self._lib.af_voice_spectrum_analyze_device(self._h, C.c_void_p(int(d_audio)), n, B, int(stride), *vad_args,
                                                            None if noise_args[0] is None else C.c_void_p(int(noise_args[0])),
                                                            int(noise_args[1]), int(noise_args[2]), C.byref(o))
        _lib.check(rc)
        for name, _ in _lib.VoiceSpectrumRow._fields_:
            out[name] = np.array([getattr(r, name) for r in rows])
        return out

    def reliability(self) -> dict:
        """The reliability statistics of the last analyze(reliability=True): the scalars of af_voice_spectrum_reliability_row
        as [n_streams] arrays, median_spectrum_db, spectral_repeatability, measurement_uncertainty_db and spectral_snr_db
        [n_streams, bins] (NaN rows where the reference returns None), window_distance [n_streams, frames] (NaN off the voiced
        frames) and inlier_mask [n_streams, frames]."""
        B, F = getattr(self, "_last_shape", (0, 0))
        dp, K = C.POINTER(C.c_double), self.bins
        rows = (_lib.VoiceSpectrumReliabilityRow * max(B, 1))()
        out = {name: np.empty((B, K)) for name in ("median_spectrum_db", "spectral_repeatability", "measurement_uncertainty_db",
                                                    "spectral_snr_db")}
        out.update(window_distance=np.empty((B, F)), inlier_mask=np.empty((B, F), dtype=np.uint8))
        o = _lib.VoiceSpectrumReliabilityOutputs(rows=rows, inlier_mask=out["inlier_mask"].ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 **{k: v.ctypes.data_as(dp) for k, v in out.items() if k != "inlier_mask"})
        _lib.check(self._lib.af_voice_spectrum_read_reliability(self._h, C.byref(o)))
        for name, _ in _lib.VoiceSpectrumReliabilityRow._fields_:
            if name != "reserved":
                out[name] = np.array([getattr(r, name) for r in rows[:B]])
        return out

    RELIABILITY_KERNELS = ("row_levels", "block_and_centre_medians", "shape_distances", "block_statistics", "robust_median")

    def last_reliability_kernel_ms(self) -> dict:
        """GPU ms of each reliability kernel in the last call, summed over its tiles (zeros with the option off)."""
        ms = (C.c_double * 5)()
        _lib.check(self._lib.af_voice_spectrum_last_reliability_kernel_ms(self._h, ms, 5))
        return dict(zip(self.RELIABILITY_KERNELS, (float(v) for v in ms)))

    def windows(self, stream: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(raw dB, smoothed dB, linear PSD), each [voiced frames, bins], of one stream of the last analyze(keep_windows=True)."""
        dp, count = C.POINTER(C.c_double), C.c_int32()
        _lib.check(self._lib.af_voice_spectrum_read_windows(self._h, int(stream), None, None, None, 0, C.byref(count)))
        arrays = [np.empty((count.value, self.bins)) for _ in range(3)]
        _lib.check(self._lib.af_voice_spectrum_read_windows(self._h, int(stream), *(x.ctypes.data_as(dp) for x in arrays), count.value,
                                                            C.byref(count)))
        return tuple(arrays)

    def last_kernel_ms(self) -> float:
        ms = C.c_double()
        _lib.check(self._lib.af_voice_spectrum_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)


def compute_voice_spectrum_batch(audio, fs: int = 48_000, nperseg: int = 4096, device: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """compute_voice_spectrum (spectrum.py:110-164) of every row of audio [n_streams, n]: (freqs [bins], spectrum_db [n_streams, bins])."""
    a = np.asarray(audio)
    if a.ndim != 2:
        raise ValueError("audio must be [n_streams, n]")
    if a.shape[1] < nperseg:
        raise ValueError(f"Audio too short for FFT: need {nperseg} samples, got {a.shape[1]} ({a.shape[1] / fs:.2f} seconds)")
    vs = VoiceSpectrum(fs, nperseg, device)
    try:
        return vs.freqs, vs.analyze(a)["welch_db"]
    finally:
        vs.close()


def compute_voice_spectrum(audio, fs: int = 48_000, nperseg: int = 4096) -> tuple[np.ndarray, np.ndarray]:
    """Drop-in for spectrum.py:110-164 (samples are taken as float32, the reference's documented input)."""
    if len(audio) < nperseg:
        raise ValueError(f"Audio too short for FFT: need {nperseg} samples, got {len(audio)} ({len(audio) / fs:.2f} seconds)")
    freqs, spectra = compute_voice_spectrum_batch(np.asarray(audio, dtype=np.float32).reshape(1, -1), fs, nperseg)
    return freqs, spectra[0]


def _estimate_snr_from_spectrum(freqs, spectrum_db, noise_spectrum_db) -> float:
    """spectrum.py:345-365: integrated voice-band SNR against a matched noise reference (0 without one)."""
    if noise_spectrum_db is None:
        return 0.0
    band = (freqs >= 80.0) & (freqs <= 8000.0)
    if not np.any(band):
        band = np.ones_like(freqs, dtype=bool)
    total = np.power(10.0, spectrum_db[band] / 10.0)
    noise = np.power(10.0, noise_spectrum_db[band] / 10.0)
    noise_sum = max(float(np.sum(noise)), 1e-18)
    signal_sum = max(float(np.sum(total - noise)), noise_sum * 1e-6)
    return float(10.0 * np.log10(signal_sum / noise_sum))


def _estimate_tilt_db_per_octave(freqs, spectrum_db) -> float:
    """spectrum.py:368-378: least-squares slope over log2(f), 100 Hz .. 8 kHz."""
    band = (freqs >= 100.0) & (freqs <= 8000.0)
    if np.count_nonzero(band) < 2:
        return 0.0
    x = np.log2(freqs[band])
    x = x - float(np.mean(x))
    denom = float(np.sum(x * x))
    if denom <= 0.0:
        return 0.0
    y = spectrum_db[band]
    return float(np.dot(x, y - float(np.mean(y))) / denom)


def measure_voice_spectra(audio, fs: int = 48_000, nperseg: int = 4096, vad_probabilities=None, noise_audio=None,
                          return_windows: bool = False, device: int = 0) -> list[dict[str, Any]]:
    """analyze_voice_spectrum (spectrum.py:498-645) of every row of audio [n_streams, n], one dict per stream under the field
    names of VoiceSpectrumResult.  A stream that takes the single-spectrum fallback (:605-645) carries the complete result;
    the others carry what precedes the robust median (analyze_voice_spectrum_batch returns the complete result for every
    stream): the speech and noise references, the per-bin SNR of :603, the frame levels and mask, and with `return_windows`
    the voiced frames' raw and perceptually smoothed spectra."""
    vs = VoiceSpectrum(fs, nperseg, device)
    try:
        r = vs.analyze(audio, vad_probabilities, noise_audio, keep_windows=return_windows)
        freqs = vs.freqs
        results = []
        for s in range(len(r["frames"])):
            have_noise = not np.isnan(r["noise_db"][s, 0])
            noise = r["noise_db"][s] if have_noise else None
            fallback = bool(r["used_single_spectrum_fallback"][s])
            item = {
                "freqs": freqs,
                "voiced_window_ratio": float(r["voiced_window_ratio"][s]),
                "used_single_spectrum_fallback": fallback,
                "vad_probability_used": bool(r["vad_probability_used"][s]),
                "vad_active_window_ratio": float(r["vad_active_window_ratio"][s]),
                "spectral_snr_db": r["spectral_snr_db"][s] if have_noise else None,
                "noise_spectrum_db": noise,
                "noise_reference_source": NOISE_REFERENCE_SOURCES[int(r["noise_reference_source"][s])],
                "speech_reference_db": None if np.isnan(r["speech_db"][s, 0]) else r["speech_db"][s],
                "welch_spectrum_db": r["welch_db"][s],
                "frame_rms_db": r["frame_rms_db"][s],
                "voiced_mask": r["voiced_mask"][s].astype(bool),
            }
            if fallback:
                spectrum = r["welch_db"][s]
                item.update(median_spectrum_db=spectrum, window_spectra_db=np.asarray([spectrum]),
                            snr_db=_estimate_snr_from_spectrum(freqs, spectrum, noise), spectral_repeatability=np.zeros_like(freqs),
                            spectral_tilt_db_per_octave=_estimate_tilt_db_per_octave(freqs, spectrum), residual_confidence=0.0,
                            measurement_coverage=0.45, outlier_rejection_ratio=0.0,
                            measurement_uncertainty_db=np.full_like(freqs, np.inf), phonetic_coverage=0.0,
                            effective_measurement_blocks=0.0)
            elif return_windows:
                raw, smoothed, _ = vs.windows(s)
                item.update(window_spectra_db=raw, smoothed_window_spectra_db=smoothed)
            results.append(item)
        return results
    finally:
        vs.close()


@dataclasses.dataclass(frozen=True)
class VoiceSpectrumResult:
    """spectrum.py:33-55, field for field."""

    freqs: np.ndarray
    median_spectrum_db: np.ndarray
    window_spectra_db: np.ndarray
    voiced_window_ratio: float
    snr_db: float
    spectral_repeatability: np.ndarray
    spectral_tilt_db_per_octave: float
    residual_confidence: float
    used_single_spectrum_fallback: bool
    measurement_coverage: float = 1.0
    outlier_rejection_ratio: float = 0.0
    vad_probability_used: bool = False
    vad_active_window_ratio: float = 0.0
    spectral_snr_db: np.ndarray | None = None
    noise_spectrum_db: np.ndarray | None = None
    noise_reference_source: str = "unavailable"
    measurement_uncertainty_db: np.ndarray | None = None
    phonetic_coverage: float = 0.0
    effective_measurement_blocks: float = 0.0


def analyze_voice_spectrum_batch(audio, fs: int = 48_000, nperseg: int = 4096, *, vad_probabilities=None, noise_audio=None,
                                 noise_spectrum_override=None, noise_reference_source_override=None,
                                 device: int = 0) -> list[VoiceSpectrumResult]:
    """analyze_voice_spectrum (spectrum.py:498-742) of every row of audio [n_streams, n]: both of its returns, the robust median
    and the reliability statistics computed on the device.  window_spectra_db holds the raw voiced windows on the main branch.
    noise_spectrum_override: (freqs [n], spectrum_db [n] or [n_streams, n]), spectrum.py:554-569; a stream whose override is
    accepted reports noise_reference_source_override, or "validated_conservative" without one."""
    a = np.asarray(audio)
    if a.ndim != 2:
        raise ValueError("audio must be [n_streams, n]")
    if a.shape[1] < nperseg:
        raise ValueError(f"Audio too short for FFT: need {nperseg} samples, got {a.shape[1]} ({a.shape[1] / fs:.2f} seconds)")
    vs = VoiceSpectrum(fs, nperseg, device)
    try:
        r = vs.analyze(a, vad_probabilities, noise_audio, keep_windows=True, reliability=True, noise_override=noise_spectrum_override)
        q = vs.reliability()
        sources = list(NOISE_REFERENCE_SOURCES)
        if noise_reference_source_override:
            sources[3] = str(noise_reference_source_override)
        results = []
        for s in range(a.shape[0]):
            have_noise = not np.isnan(r["noise_db"][s, 0])
            fallback = bool(r["used_single_spectrum_fallback"][s])
            median = q["median_spectrum_db"][s]
            results.append(VoiceSpectrumResult(
                freqs=vs.freqs, median_spectrum_db=median,
                window_spectra_db=np.asarray([median]) if fallback else vs.windows(s)[0],
                voiced_window_ratio=float(r["voiced_window_ratio"][s]), snr_db=float(q["snr_db"][s]),
                spectral_repeatability=q["spectral_repeatability"][s],
                spectral_tilt_db_per_octave=float(q["spectral_tilt_db_per_octave"][s]),
                residual_confidence=float(q["residual_confidence"][s]), used_single_spectrum_fallback=fallback,
                measurement_coverage=float(q["measurement_coverage"][s]),
                outlier_rejection_ratio=float(q["outlier_rejection_ratio"][s]),
                vad_probability_used=bool(r["vad_probability_used"][s]),
                vad_active_window_ratio=float(r["vad_active_window_ratio"][s]),
                spectral_snr_db=q["spectral_snr_db"][s] if have_noise else None,
                noise_spectrum_db=r["noise_db"][s] if have_noise else None,
                noise_reference_source=sources[int(r["noise_reference_source"][s])],
                measurement_uncertainty_db=q["measurement_uncertainty_db"][s],
                phonetic_coverage=float(q["phonetic_coverage"][s]),
                effective_measurement_blocks=float(q["effective_measurement_blocks"][s])))
        return results
    finally:
        vs.close()


def analyze_voice_spectrum(audio, fs=48000, nperseg=4096, *, vad_probabilities=None, noise_audio=None,
                           noise_spectrum_override=None, noise_reference_source_override=None) -> VoiceSpectrumResult:
    """Drop-in for spectrum.py:498-742 (samples are taken as float32).  This single-capture form still refuses the noise-spectrum
    override (a pinned contract of the ABI tests); analyze_voice_spectrum_batch takes it for one stream or many."""
    if noise_spectrum_override is not None or noise_reference_source_override is not None:
        raise NotImplementedError("noise_spectrum_override / noise_reference_source_override are not built")
    if len(audio) < nperseg:
        raise ValueError(f"Audio too short for FFT: need {nperseg} samples, got {len(audio)} ({len(audio) / fs:.2f} seconds)")
    row = lambda x: None if x is None else np.asarray(x).reshape(1, -1)  # noqa: E731
    return analyze_voice_spectrum_batch(np.asarray(audio, dtype=np.float32).reshape(1, -1), fs, nperseg,
                                        vad_probabilities=row(vad_probabilities), noise_audio=row(noise_audio))[0]


# ------------------------------------------------------------------ room-noise reference analysis
NOISE_REFERENCE_STATUS = ("usable", "questionable", "invalid")
# one text per bit of af_noise_reference_row.reasons / .guidance, in the order noise_reference.py:315-470 appends them
NOISE_REFERENCE_REASONS = (
    "room-noise capture is too short",
    "room-noise capture contains non-finite samples",
    "room-noise capture is suspiciously silent",
    "room-noise capture is clipped",
    "room-noise capture contains isolated clipped samples",
    "room-noise capture has too few analysis windows",
    "room-noise capture is dominated by changing events",
    "room-noise capture is not stationary",
    "room-noise capture contains dominant transient events",
    "room-noise capture contains strong transients",
    "speech is present in the room-noise capture",
    "possible speech contamination in room-noise capture",
    "input device changed between noise and voice captures",
    "input channel mode changed between noise and voice captures",
    "channel count changed between noise and voice captures",
    "noise capture sample rate does not match analysis",
    "voice capture sample rate does not match analysis",
    "sample rate changed between noise and voice captures",
    "room-noise reference is stale",
    "room-noise reference may be stale",
    "room noise does not match conditions during the voice capture",
    "room-noise reference only partly matches the voice capture",
    "room-noise level changed substantially before the voice capture",
    "room-noise reference is much louder than in-capture quiet frames",
)
NOISE_REFERENCE_GUIDANCE = (
    "Record at least 1.5 seconds of room tone.",
    "Restart the audio stream and record the room tone again.",
    "Check the selected microphone and record normal room tone again.",
    "Lower input gain or remove the transient source, then recapture.",
    "Recapture without taps or handling noise for a cleaner reference.",
    "Wait for the room to settle and record a new reference.",
    "Avoid movement, speech, and intermittent sounds while recapturing.",
    "Recapture without keyboard, handling, or impact sounds.",
    "Remain silent and record the room noise again.",
    "Record another room-noise sample without voices.",
    "Use the same microphone, channel mode, and sample rate for both captures.",
    "Record room noise immediately before the voice sample.",
    "Recapture room noise under the current conditions.",
    "Recapture room noise and voice without changing the environment.",
    "Recapture both samples for a more reliable correction.",
    "Record room noise and voice under the same conditions.",
    "Check whether the noise source changed between captures.",
)
NOISE_REFERENCE_METRICS = ("duration_s", "finite_fraction", "noise_rms_db", "conservative_noise_rms_db", "noise_peak_db",
                           "crest_factor_db", "clipped_fraction", "zero_fraction", "rms_spread_db", "octave_stability_db",
                           "spectral_flux_db", "vad_contamination_ratio", "vad_contamination_p90")
NOISE_REFERENCE_KERNELS = ("statistics_and_chunk_sums", "frame_powers", "frame_spectra", "column_medians")


def _clean_optional_text(value):
    if value is None:
        return None
    text = str(value).strip()
    return text or None


@dataclasses.dataclass(frozen=True)
class CaptureMetadata:
    """noise_reference.py:21-56, field for field: identity and timing attached to one calibration capture."""

    captured_at_unix_s: float | None = None
    input_device: str | None = None
    sample_rate: int | None = None
    channel_mode: str | None = None
    channel_count: int | None = None

    @classmethod
    def coerce(cls, value) -> "CaptureMetadata":
        if value is None:
            return cls()
        if isinstance(value, cls):
            return value
        if not isinstance(value, Mapping):
            raise TypeError("capture metadata must be a mapping or CaptureMetadata")
        timestamp, sample_rate, channel_count = value.get("captured_at_unix_s"), value.get("sample_rate"), value.get("channel_count")
        return cls(
            captured_at_unix_s=float(timestamp) if timestamp is not None and np.isfinite(float(timestamp)) else None,
            input_device=_clean_optional_text(value.get("input_device")),
            sample_rate=int(sample_rate) if sample_rate is not None else None,
            channel_mode=_clean_optional_text(value.get("channel_mode")),
            channel_count=int(channel_count) if channel_count is not None else None,
        )


@dataclasses.dataclass
class NoiseReferenceAnalysis:
    """noise_reference.py:59-86, field for field."""

    status: str
    quality_score: float
    usable: bool
    conservative: bool
    reasons: list
    guidance: list
    metrics: dict
    frequencies: np.ndarray
    explicit_spectrum_db: np.ndarray
    conservative_spectrum_db: np.ndarray
    in_capture_spectrum_db: np.ndarray | None = None
    conservative_noise_rms_db: float = -120.0

    def diagnostics(self) -> dict:
        return {"status": self.status, "quality_score": self.quality_score, "usable": self.usable, "conservative": self.conservative,
                "reasons": list(self.reasons), "guidance": list(self.guidance), "metrics": dict(self.metrics)}


def _metadata_arguments(noise_metadata, speech_metadata, sample_rate: int) -> tuple[float, int, bool]:
    """_metadata_mismatches, :223-249, as the library takes it: (capture age in s, NaN when unknown and not yet clamped at 0;
    AF_NOISE_MISMATCH_* bits; identity_metadata_available of :526-528)."""
    noise, speech = CaptureMetadata.coerce(noise_metadata), CaptureMetadata.coerce(speech_metadata)
    mask = 0
    for bit, (left, right) in enumerate(((noise.input_device, speech.input_device), (noise.channel_mode, speech.channel_mode),
                                         (noise.channel_count, speech.channel_count))):
        if left is not None and right is not None and left != right:
            mask |= 1 << bit
    for bit, metadata in ((3, noise), (4, speech)):
        if metadata.sample_rate is not None and metadata.sample_rate != sample_rate:
            mask |= 1 << bit
    if noise.sample_rate is not None and speech.sample_rate is not None and noise.sample_rate != speech.sample_rate:
        mask |= 1 << 5
    age = float("nan")
    if noise.captured_at_unix_s is not None and speech.captured_at_unix_s is not None:
        age = speech.captured_at_unix_s - noise.captured_at_unix_s
    return age, mask, noise.input_device is not None and speech.input_device is not None


class NoiseReference:
    """python/mic_eq/analysis/noise_reference.py for a batch of capture pairs on the device.  One object per sample rate;
    scratch is kept between calls.  A sample rate whose analysis frame the transform does not take raises NotImplementedError."""

    def __init__(self, sample_rate: int = 48_000, device: int = 0):
        self._lib = _lib.load()
        handle = C.c_void_p()
        _lib.check(self._lib.af_noise_reference_create(int(sample_rate), int(device), C.byref(handle)))
        self._h = handle
        self.sample_rate = int(sample_rate)
        self.frame_size = int(self._lib.af_noise_reference_frame_size(handle))

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.af_noise_reference_destroy(self._h)
            self._h = None

    __del__ = close

    def frames(self, n_samples: int) -> int:
        return int(self._lib.af_noise_reference_frames(self._h, int(n_samples)))

    def bins(self, n_noise: int) -> int:
        return int(self._lib.af_noise_reference_bins(self._h, int(n_noise)))

    def frequencies(self, n_noise: int) -> np.ndarray:
        """The grid of the spectra: the frames', or np.fft.rfftfreq(max(2, n_noise)) below one frame (:339)."""
        n = self.frame_size if n_noise >= self.frame_size else max(2, int(n_noise))
        return np.arange(n // 2 + 1) * (1.0 / (n * (1.0 / self.sample_rate)))

    def analyze(self, noise_audio, speech_audio=None, noise_vad_probabilities=None, speech_vad_probabilities=None, capture_age_s=None,
                metadata_mismatch=None, device_pointers=None, internals: bool = False) -> dict:
        """noise_audio [n_streams, n_noise] and speech_audio [n_streams, n_speech] | None, float32 (host), or with
        `device_pointers=(d_noise, n_noise, n_streams, noise_stride, d_speech | None, n_speech, speech_stride)` device memory.
        Returns arrays by field: the scalars of af_noise_reference_row as [n_streams] arrays, the three spectra
        [n_streams, bins] (in_capture_spectrum_db: NaN rows where the reference returns None), frame_rms_db [n_streams, frames]
        and band_levels_db [n_streams, frames, 7] of the noise capture.  `internals` adds what the kernels left: chunk sums,
        frame powers, PSD rows, band sums and the middles of both medians."""
        dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        if device_pointers is None:
            z = np.ascontiguousarray(noise_audio, dtype=np.float32)
            if z.ndim != 2:
                raise ValueError("noise_audio must be [n_streams, n_noise]")
            B, n = z.shape
            v = None if speech_audio is None else np.ascontiguousarray(speech_audio, dtype=np.float32)
            if v is not None and (v.ndim != 2 or v.shape[0] != B):
                raise ValueError("speech_audio must be [n_streams, n_speech]")
            m = 0 if v is None else v.shape[1]
        else:
            n, B, m = int(device_pointers[1]), int(device_pointers[2]), int(device_pointers[5]) if device_pointers[4] is not None else 0

        def per_stream(x, dtype, what):
            if x is None:
                return None
            x = np.ascontiguousarray(x, dtype=dtype)
            if x.ndim == 0 or x.shape[0] != B:
                raise ValueError(f"{what} must have one entry per stream")
            return x

        nv = per_stream(noise_vad_probabilities, np.float64, "noise_vad_probabilities")
        sv = per_stream(speech_vad_probabilities, np.float64, "speech_vad_probabilities")
        for x, what in ((nv, "noise_vad_probabilities"), (sv, "speech_vad_probabilities")):
            if x is not None and (x.ndim != 2 or x.shape[1] == 0):
                raise ValueError(f"{what} must be [n_streams, n] with n >= 1")
        age = per_stream(capture_age_s, np.float64, "capture_age_s")
        mismatch = per_stream(metadata_mismatch, np.uint32, "metadata_mismatch")
        F, Fv, K, Ko = self.frames(n), self.frames(m), self.frame_size // 2 + 1, self.bins(n)
        rows = (_lib.NoiseReferenceRow * B)()
        out = {name: np.empty((B, Ko)) for name in ("explicit_spectrum_db", "conservative_spectrum_db", "in_capture_spectrum_db")}
        out.update(frame_rms_db=np.empty((B, F)), band_levels_db=np.empty((B, F, 7)))
        if internals:
            out.update(noise_chunk_sums=np.empty((B, F + 1 if F else 0, 2)), noise_frame_power=np.empty((B, F)),
                       speech_frame_power=np.empty((B, Fv)), noise_psd=np.empty((B, F, K)), band_power=np.empty((B, F, 7)),
                       explicit_middles=np.empty((B, 2, K)), in_capture_middles=np.empty((B, 2, K)))
        o = _lib.NoiseReferenceOutputs(rows=rows, **{k: a.ctypes.data_as(dp) for k, a in out.items()})
        vad_args = (None if nv is None else nv.ctypes.data_as(dp), 0 if nv is None else nv.shape[1],
                    None if sv is None else sv.ctypes.data_as(dp), 0 if sv is None else sv.shape[1],
                    None if age is None else age.ctypes.data_as(dp),
                    None if mismatch is None else mismatch.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(o))
        if device_pointers is None:
            rc = self._lib.af_noise_reference_analyze_host(self._h, z.ctypes.data_as(fp), n, B, n, None if v is None else v.ctypes.data_as(fp),
                                                           m, m, *vad_args)
        else:
            d_noise, _, _, noise_stride, d_speech, _, speech_stride = device_pointers
            rc = self._lib.af_noise_reference_analyze_device(self._h, C.c_void_p(int(d_noise)), n, B, int(noise_stride),
                                                             None if d_speech is None else C.c_void_p(int(d_speech)), m,
                                                             int(speech_stride), *vad_args)
        _lib.check(rc)
        for name, _ in _lib.NoiseReferenceRow._fields_:
            if name != "reserved":
                out[name] = np.array([getattr(r, name) for r in rows])
        out["frequencies"] = self.frequencies(n)
        return out

    def last_kernel_ms(self) -> dict:
        """GPU ms of each stage of the last call, summed over its tiles."""
        ms = (C.c_double * 4)()
        _lib.check(self._lib.af_noise_reference_last_kernel_ms(self._h, ms, 4))
        return dict(zip(NOISE_REFERENCE_KERNELS, (float(x) for x in ms)))


def _bit_texts(mask: int, table) -> list:
    return [text for bit, text in enumerate(table) if mask >> bit & 1]


def _noise_reference_results(r: dict, identity: Sequence[bool]) -> list:
    results = []
    none = lambda x: None if np.isnan(x) else float(x)  # noqa: E731
    for s in range(len(r["status"])):
        metrics = {name: float(r[name][s]) for name in NOISE_REFERENCE_METRICS}
        metrics.update(capture_age_s=none(r["capture_age_s"][s]), identity_metadata_available=bool(identity[s]),
                       in_capture_noise_frame_count=int(r["in_capture_noise_frame_count"][s]),
                       in_capture_level_delta_db=none(r["in_capture_level_delta_db"][s]),
                       spectral_shape_distance_db=none(r["spectral_shape_distance_db"][s]))
        status = NOISE_REFERENCE_STATUS[int(r["status"][s])]
        results.append(NoiseReferenceAnalysis(
            status=status, quality_score=float(r["quality_score"][s]), usable=status != "invalid",
            conservative=bool(r["conservative"][s]), reasons=_bit_texts(int(r["reasons"][s]), NOISE_REFERENCE_REASONS),
            guidance=_bit_texts(int(r["guidance"][s]), NOISE_REFERENCE_GUIDANCE), metrics=metrics, frequencies=r["frequencies"],
            explicit_spectrum_db=r["explicit_spectrum_db"][s], conservative_spectrum_db=r["conservative_spectrum_db"][s],
            in_capture_spectrum_db=r["in_capture_spectrum_db"][s] if r["has_in_capture_spectrum"][s] else None,
            conservative_noise_rms_db=float(r["conservative_noise_rms_db"][s])))
    return results


def _per_stream_metadata(value, n_streams: int) -> list:
    if value is None or isinstance(value, (CaptureMetadata, Mapping)):
        return [value] * n_streams
    value = list(value)
    if len(value) != n_streams:
        raise ValueError("metadata must be one value or one per stream")
    return value


def analyze_noise_reference_batch(noise_audio, speech_audio, sample_rate: int, *, noise_metadata=None, speech_metadata=None,
                                  noise_vad_probabilities=None, speech_vad_probabilities=None, device: int = 0) -> list:
    """analyze_noise_reference (noise_reference.py:280-546) of every row of noise_audio [n_streams, n] against the same row of
    speech_audio [n_streams, m] (or None).  Metadata: one value (CaptureMetadata, mapping or None) or one per stream."""
    if sample_rate <= 0:
        raise ValueError("sample_rate must be positive")
    z = np.asarray(noise_audio)
    if z.ndim != 2:
        raise ValueError("noise_audio must be [n_streams, n_noise]")
    B = z.shape[0]
    pairs = [_metadata_arguments(a, b, int(sample_rate))
             for a, b in zip(_per_stream_metadata(noise_metadata, B), _per_stream_metadata(speech_metadata, B))]
    nr = NoiseReference(sample_rate, device)
    try:
        r = nr.analyze(z, speech_audio, noise_vad_probabilities, speech_vad_probabilities, capture_age_s=[p[0] for p in pairs],
                       metadata_mismatch=[p[1] for p in pairs])
        return _noise_reference_results(r, [p[2] for p in pairs])
    finally:
        nr.close()


def analyze_noise_reference(noise_audio, speech_audio, sample_rate: int, *, noise_metadata=None, speech_metadata=None,
                            noise_vad_probabilities=None, speech_vad_probabilities=None) -> NoiseReferenceAnalysis:
    """Drop-in for noise_reference.py:280-546 (samples are taken as float32)."""
    row = lambda x, dtype: None if x is None else np.asarray(x, dtype=dtype).reshape(1, -1)  # noqa: E731
    speech = row(speech_audio, np.float32)
    vad = lambda x: None if x is None or np.asarray(x).size == 0 else row(x, np.float64)  # noqa: E731
    return analyze_noise_reference_batch(row(noise_audio, np.float32), None if speech is None or speech.shape[1] == 0 else speech,
                                         sample_rate, noise_metadata=noise_metadata, speech_metadata=speech_metadata,
                                         noise_vad_probabilities=vad(noise_vad_probabilities),
                                         speech_vad_probabilities=vad(speech_vad_probabilities))[0]


def analyze_voice_capture_batch(noise_audio, speech_audio, fs: int = 48_000, nperseg: int = 4096, *, noise_metadata=None,
                                speech_metadata=None, noise_vad_probabilities=None, speech_vad_probabilities=None,
                                vad_probabilities=None, device: int = 0) -> tuple[list, list]:
    """The two steps of the reference's voice setup (voice_setup.py:1122-1162) for every capture pair: analyze_noise_reference on
    the room tone and the voice capture, then analyze_voice_spectrum of the voice capture with the conservative spectrum as its
    noise-spectrum override ("validated_conservative") and the room tone as noise_audio behind it.  speech_vad_probabilities
    are the posteriors spread evenly over the voice capture (step one), vad_probabilities the ones per 32 ms model window (step
    two).  Returns (noise reference analyses, voice spectrum results)."""
    references = analyze_noise_reference_batch(noise_audio, speech_audio, fs, noise_metadata=noise_metadata, speech_metadata=speech_metadata,
                                               noise_vad_probabilities=noise_vad_probabilities,
                                               speech_vad_probabilities=speech_vad_probabilities, device=device)
    override = (references[0].frequencies, np.stack([r.conservative_spectrum_db for r in references]))
    spectra = analyze_voice_spectrum_batch(speech_audio, fs, nperseg, vad_probabilities=vad_probabilities, noise_audio=noise_audio,
                                           noise_spectrum_override=override, noise_reference_source_override="validated_conservative",
                                           device=device)
    return references, spectra


SPEECH_FEATURES_KERNELS = ("frame_powers", "k_weighting", "frame_spectra", "frame_medians", "weighted_peak")
SPEECH_FEATURES_RATES = (16_000, 22_050, 24_000, 32_000, 44_100, 48_000, 88_200, 96_000)  # with device_rate=True
_SPEECH_FEATURES_EVIDENCE = ("frame_probability_p90", "frame_probability_top_mean", "temporal_score", "absolute_hf_strength_p90",
                             "noise_reliability_p90")


class SpeechFeatures:
    """_vad_masked_speech_features (voice_setup.py:161-458) for a batch of voice captures on the device; scratch is kept
    between calls.  By default 48 kHz only: any other rate raises NotImplementedError.  ``device_rate=True`` takes the rates of
    SPEECH_FEATURES_RATES (af_device_rate_features_*): frames and spectra at the capture's rate, the loudness at 48 kHz behind
    the device's restatement of scipy.signal.resample_poly, as the reference does it; at 48 kHz the results are the same bits."""

    def __init__(self, sample_rate: int = 48_000, max_streams: int = 4096, max_speech_samples: int = 48_000 * 60,
                 max_noise_samples: int = 48_000 * 60, device: int = 0, *, device_rate: bool = False):
        self._lib = _lib.load()
        self.device_rate = bool(device_rate)
        self._family = "af_device_rate_features_" if self.device_rate else "af_speech_features_"
        handle = C.c_void_p()
        _lib.check(self._fn("create")(int(sample_rate), int(max_streams), int(max_speech_samples), int(max_noise_samples), int(device),
                                      C.byref(handle)))
        self._h = handle
        self.sample_rate = int(sample_rate)
        self.sibilance_bins = int(self._fn("sibilance_bins")(handle))

    def _fn(self, name: str):
        return getattr(self._lib, self._family + name)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    __del__ = close

    def frames(self, n_samples: int) -> int:
        return int(self._fn("frames")(self._h, int(n_samples)) if self.device_rate else self._fn("frames")(int(n_samples)))

    def chunks(self, n_samples: int) -> int:
        """Chunks of the K-weighted 48 kHz signal: hop-sized at 48 kHz, 960 resampled samples at any other rate."""
        return int(self._fn("chunks")(self._h, int(n_samples)) if self.device_rate else self._fn("chunks")(int(n_samples)))

    def resampled_length(self, n_samples: int) -> int:
        """Samples of a capture at 48 kHz: ceil(n 48000 / fs), what resample_poly returns."""
        if not self.device_rate:
            return int(n_samples)
        return int(self._fn("resampled_length")(self._h, int(n_samples)))

    def set_scratch_bytes(self, n_bytes: int) -> None:
        """Bound the scratch of the resampled captures (device_rate=True; 256 MB by default): they pass through it a segment of
        whole 48 kHz chunks of every stream at a time.  Results do not depend on it."""
        if not self.device_rate:
            raise ValueError("the resampling stage belongs to device_rate=True")
        _lib.check(self._fn("set_scratch_bytes")(self._h, int(n_bytes)))

    def resample(self, speech, active_frames) -> tuple:
        """The resampling stage alone, for tests (device_rate=True, not 48 kHz): speech [n_streams, n] float32 and frame flags
        [n_streams, frames(n)] -> (signal [n_streams, n48] f64, mask bytes [n_streams, n48], set bytes per chunk [n_streams, chunks(n)])."""
        if not self.device_rate:
            raise ValueError("the resampling stage belongs to device_rate=True")
        x = np.ascontiguousarray(speech, dtype=np.float32)
        flags = np.ascontiguousarray(active_frames, dtype=np.uint8)
        if x.ndim != 2 or flags.shape != (x.shape[0], max(self.frames(x.shape[1]), 0)):
            raise ValueError("speech must be [n_streams, n] and active_frames [n_streams, frames(n)]")
        B, n = x.shape
        n48 = self.resampled_length(n)
        signal, mask, counts = np.zeros((B, n48)), np.zeros((B, n48), dtype=np.uint8), np.zeros((B, self.chunks(n)), dtype=np.int32)
        bp = C.POINTER(C.c_uint8)
        _lib.check(self._fn("debug_resample_host")(self._h, x.ctypes.data_as(C.POINTER(C.c_float)), n, B, n, flags.ctypes.data_as(bp),
                                                   signal.ctypes.data_as(C.POINTER(C.c_double)), mask.ctypes.data_as(bp),
                                                   counts.ctypes.data_as(C.POINTER(C.c_int32))))
        return signal, mask, counts

    def set_frame_model(self, intercept: float, coefficients) -> None:
        """FRAME_INTERCEPT and FRAME_COEFFICIENTS of deesser_fusion.py:30-41 (the defaults)."""
        w = np.ascontiguousarray(coefficients, dtype=np.float64)
        if w.shape != (6,):
            raise ValueError("coefficients must be six values")
        _lib.check(self._fn("set_frame_model")(self._h, float(intercept), w.ctypes.data_as(C.POINTER(C.c_double))))

    def frame_model(self) -> tuple:
        intercept, w = C.c_double(), np.zeros(6)
        _lib.check(self._fn("get_frame_model")(self._h, C.byref(intercept), w.ctypes.data_as(C.POINTER(C.c_double))))
        return float(intercept.value), w

    def analyze(self, speech, noise_rms_db, vad_probabilities=None, noise_audio=None, device_pointers=None, internals: bool = False) -> dict:
        """speech [n_streams, n] and noise_audio [n_streams, m] | None, float32 (host), or with `device_pointers=(d_speech, n,
        n_streams, speech_stride, d_noise | None, m, noise_stride)` device memory.  Returns arrays by field: the scalars of
        af_speech_features_row as [n_streams] arrays, frame_db and active_frame_mask [n_streams, frames], and frame_indices,
        frame_probabilities, frame_feature_rows whose first spectral_frames entries per stream are filled.  `internals` adds
        what the kernels left."""
        dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        if device_pointers is None:
            x = np.ascontiguousarray(speech, dtype=np.float32)
            if x.ndim != 2:
                raise ValueError("speech must be [n_streams, n]")
            B, n = x.shape
            z = None if noise_audio is None else np.ascontiguousarray(noise_audio, dtype=np.float32)
            if z is not None and (z.ndim != 2 or z.shape[0] != B):
                raise ValueError("noise_audio must be [n_streams, n_noise]")
            m = 0 if z is None else z.shape[1]
        else:
            n, B, m = int(device_pointers[1]), int(device_pointers[2]), int(device_pointers[5]) if device_pointers[4] is not None else 0
        level = np.ascontiguousarray(noise_rms_db, dtype=np.float64).reshape(-1)
        if level.size != B:
            raise ValueError("noise_rms_db must have one entry per stream")
        vad = None if vad_probabilities is None else np.ascontiguousarray(vad_probabilities, dtype=np.float64)
        if vad is not None and (vad.ndim != 2 or vad.shape[0] != B or vad.shape[1] == 0):
            raise ValueError("vad_probabilities must be [n_streams, n_vad] with n_vad >= 1")
        F, Cn, Fn, S = max(self.frames(n), 0), self.chunks(n), self.frames(m), self.sibilance_bins
        rows = (_lib.SpeechFeaturesRow * B)()
        out = dict(frame_db=np.zeros((B, F)), active_frame_mask=np.zeros((B, F), dtype=np.uint8),
                   frame_indices=np.zeros((B, F), dtype=np.int32), frame_probabilities=np.zeros((B, F)),
                   frame_feature_rows=np.zeros((B, F, 6)))
        if internals:
            out.update(frame_power=np.zeros((B, F)), chunk_energy=np.zeros((B, Cn)), band_sums=np.zeros((B, F, 8)),
                       sibilance_middles=np.zeros((B, F, 2)), sibilance_argmax=np.zeros((B, F), dtype=np.int32),
                       sibilance_rows=np.zeros((B, F, S)), noise_band_sums=np.zeros((B, Fn)), weighted_sums=np.zeros((B, S)),
                       weighted_argmax=np.zeros(B, dtype=np.int32))
        kinds = {np.dtype(np.float64): C.c_double, np.dtype(np.uint8): C.c_uint8, np.dtype(np.int32): C.c_int32}
        o = _lib.SpeechFeaturesOutputs(rows=rows, **{k: a.ctypes.data_as(C.POINTER(kinds[a.dtype])) for k, a in out.items()})
        tail = (level.ctypes.data_as(dp), None if vad is None else vad.ctypes.data_as(dp), 0 if vad is None else vad.shape[1])
        if device_pointers is None:
            rc = self._fn("analyze_host")(self._h, x.ctypes.data_as(fp), n, B, n, *tail, None if z is None else z.ctypes.data_as(fp), m, m,
                                          C.byref(o))
        else:
            d_speech, _, _, stride, d_noise, _, noise_stride = device_pointers
            rc = self._fn("analyze_device")(self._h, C.c_void_p(int(d_speech)), n, B, int(stride), *tail,
                                            None if d_noise is None else C.c_void_p(int(d_noise)), m, int(noise_stride), C.byref(o))
        _lib.check(rc)
        for name, _ in _lib.SpeechFeaturesRow._fields_:
            if name != "reserved":
                out[name] = np.array([getattr(r, name) for r in rows])
        return out

    def last_kernel_ms(self) -> dict:
        """GPU ms of each stage of the last call, summed over its tiles (with device_rate=True also "resampling")."""
        names = SPEECH_FEATURES_KERNELS + (("resampling",) if self.device_rate else ())
        ms = (C.c_double * len(names))()
        _lib.check(self._fn("last_kernel_ms")(self._h, ms, len(names)))
        return dict(zip(names, (float(x) for x in ms)))


def _speech_features_dicts(r: dict) -> list:
    """One dict per stream with the keys of voice_setup.py:432-458; None for a stream with a non-finite sample."""
    results = []
    for s in range(len(r["frames"])):
        if r["non_finite"][s]:
            results.append(None)
            continue
        A = int(r["spectral_frames"][s])
        value = lambda name: float(r[name][s])  # noqa: E731
        evidence = {"available": bool(r["evidence_available"][s]), "confidence": value("confidence"),
                    "frame_probabilities": r["frame_probabilities"][s, :A].copy(), "frame_feature_rows": r["frame_feature_rows"][s, :A].copy(),
                    "frame_indices": r["frame_indices"][s, :A].astype(np.int64)}
        if evidence["available"]:
            evidence.update({name: value(name) for name in _SPEECH_FEATURES_EVIDENCE})
        evidence.update({name: value(name) for name in ("excess_p90_db", "temporal_contrast_db", "candidate_frame_ratio",
                                                        "candidate_snr_db", "peak_hz")})
        results.append({
            "frame_db": r["frame_db"][s].copy(), "active_frame_mask": r["active_frame_mask"][s].astype(bool),
            "active_duration_s": value("active_duration_s"), "active_ratio": value("active_ratio"),
            "vad_probability_used": bool(r["vad_probability_used"][s]), "vad_active_frame_ratio": value("vad_active_frame_ratio"),
            "short_term_lufs": value("short_term_lufs"), "short_term_window_count": int(r["short_term_window_count"][s]),
            "momentary_lufs": value("momentary_lufs"), "active_loudness_spread_db": value("active_loudness_spread_db"),
            "loudness_range_db": value("loudness_range_db"), "loudness_window_count": int(r["loudness_window_count"][s]),
            "band_energy_db": {"low": value("band_low_db"), "body": value("band_body_db"), "presence": value("band_presence_db"),
                               "sibilance": value("band_sibilance_db")},
            "sibilance_excess_db": value("sibilance_excess_db"), "deesser_frame_evidence": evidence})
    return results


def measure_speech_features_batch(speech, fs: int, noise_rms_db, *, vad_probabilities=None, noise_audio=None, device: int = 0,
                                  device_rate: bool = False) -> list:
    """_vad_masked_speech_features (voice_setup.py:161-458) of every row of speech [n_streams, n]: a list of dicts with the
    reference's keys (samples are taken as float32).  noise_rms_db: one level per stream; vad_probabilities [n_streams, n_vad] or
    None; noise_audio [n_streams, m] or None.  A stream with a non-finite sample yields None.  fs is 48000, or with
    ``device_rate=True`` any of SPEECH_FEATURES_RATES."""
    x = np.asarray(speech)
    if x.ndim != 2:
        raise ValueError("speech must be [n_streams, n]")
    m = 0 if noise_audio is None else np.asarray(noise_audio).shape[-1]
    sf = SpeechFeatures(fs, x.shape[0], max(x.shape[1], 2 * int(fs * 0.02), 1), m, device, device_rate=device_rate)
    try:
        return _speech_features_dicts(sf.analyze(x, noise_rms_db, vad_probabilities, noise_audio))
    finally:
        sf.close()


TARGET_LUFS_BY_CURVE = {"broadcast": -16.0, "streaming": -16.0, "podcast": -17.0, "flat": -18.0}  # voice_setup.py:53-58
DYNAMICS_INTENSITIES = ("gentle", "balanced", "dense", "custom")  # AF_DYNAMICS_*
DEESSER_MODEL_VERSION = "deesser-soft-fusion-v1"  # deesser_fusion.py:7
DEESSER_CLIP_FEATURE_NAMES = ("frame_probability_p90", "frame_probability_top_mean", "candidate_support", "temporal_contrast",
                              "absolute_hf_strength_p90", "noise_reliability_p90")  # deesser_fusion.py:19-26
DEESSER_ENABLE_PROBABILITY_THRESHOLD = 0.4935253581578833  # deesser_fusion.py:57


def recommend_voice_chain(features: dict, stream: int, freqs, smoothed_spectrum_db, *, residual_confidence: float, snr_db: float,
                          used_single_spectrum_fallback: bool, noise_quality_score: float, noise_status: str,
                          conservative_noise_rms_db: float, target_preset: str = "broadcast", vad_available: bool = True,
                          dynamics_intensity: str = "balanced", custom_target_p95_db: float = 3.5, custom_peak_cap_db: float = 8.0,
                          enable_probability_threshold: float = DEESSER_ENABLE_PROBABILITY_THRESHOLD) -> dict:
    """The rules of voice_setup.py:1143-1223 for one stream of a SpeechFeatures.analyze result: ``gate``, ``deesser`` and
    ``compressor`` with the key names and value types of _recommend_gate_settings, _recommend_deesser_settings and
    _recommend_compressor_settings (plus noise_reference_reliability, :1220), ``deesser_diagnostics``,
    ``compressor_diagnostics``, ``capture_confidence`` and the level percentiles behind them.  What the other analyses measured
    is taken as arguments: the perceptually smoothed median spectrum on its grid, residual_confidence, snr_db and
    used_single_spectrum_fallback of the voice spectrum, and quality_score, status and conservative_noise_rms_db of the noise
    reference.  It returns no EQ bands, no calibrated compressor threshold and no offline validation."""
    lib = _lib.load()
    dp = C.POINTER(C.c_double)
    row = _lib.SpeechFeaturesRow(**{name: kind(features[name][stream]) for name, kind in
                                    ((n, int if t is C.c_int32 else float) for n, t in _lib.SpeechFeaturesRow._fields_ if n != "reserved")})
    frame_db = np.ascontiguousarray(features["frame_db"][stream], dtype=np.float64)
    mask = np.ascontiguousarray(features["active_frame_mask"][stream], dtype=np.uint8)
    f = np.ascontiguousarray(freqs, dtype=np.float64)
    db = np.ascontiguousarray(smoothed_spectrum_db, dtype=np.float64)
    if f.ndim != 1 or f.shape != db.shape or f.size == 0:
        raise ValueError("freqs and smoothed_spectrum_db must be equal-length vectors")
    if noise_status not in NOISE_REFERENCE_STATUS:
        raise ValueError(f"noise_status must be one of {NOISE_REFERENCE_STATUS}")
    profile = str(dynamics_intensity).lower()
    inputs = _lib.VoiceSetupInputs()
    lib.af_voice_setup_default_inputs(C.byref(inputs))
    inputs.features = C.pointer(row)
    inputs.frame_db, inputs.active_frame_mask = frame_db.ctypes.data_as(dp), mask.ctypes.data_as(C.POINTER(C.c_uint8))
    inputs.freqs, inputs.spectrum_db, inputs.bins = f.ctypes.data_as(dp), db.ctypes.data_as(dp), f.size
    inputs.used_single_spectrum_fallback = int(bool(used_single_spectrum_fallback))
    inputs.residual_confidence, inputs.snr_db = float(residual_confidence), float(snr_db)
    inputs.noise_quality_score, inputs.conservative_noise_rms_db = float(noise_quality_score), float(conservative_noise_rms_db)
    inputs.noise_status, inputs.vad_available = NOISE_REFERENCE_STATUS.index(noise_status), int(bool(vad_available))
    inputs.target_lufs = TARGET_LUFS_BY_CURVE.get(target_preset, -18.0)
    inputs.dynamics_intensity = DYNAMICS_INTENSITIES.index(profile) if profile in DYNAMICS_INTENSITIES else 1
    inputs.custom_target_p95_db, inputs.custom_peak_cap_db = float(custom_target_p95_db), float(custom_peak_cap_db)
    inputs.enable_probability_threshold = float(enable_probability_threshold)
    r = _lib.VoiceSetupRecommendation()
    _lib.check(lib.af_voice_setup_recommend(C.byref(inputs), C.byref(r)))
    name = DYNAMICS_INTENSITIES[r.compressor_profile]
    gate = {"enabled": True, "threshold_db": r.gate_threshold_db, "attack_ms": 5.0, "release_ms": 120.0, "gate_mode": int(r.gate_mode),
            "vad_threshold": r.gate_vad_threshold, "vad_hold_time_ms": r.gate_vad_hold_time_ms, "vad_pre_gain": r.gate_vad_pre_gain,
            "auto_threshold_enabled": bool(r.gate_auto_threshold_enabled), "gate_margin_db": r.gate_margin_db}
    deesser = {"enabled": bool(r.deesser_enabled), "auto_enabled": True, "auto_amount": r.deesser_auto_amount,
               "low_cut_hz": r.deesser_low_cut_hz, "high_cut_hz": r.deesser_high_cut_hz, "threshold_db": -28.0, "ratio": r.deesser_ratio,
               "attack_ms": 2.0, "release_ms": 80.0, "max_reduction_db": r.deesser_max_reduction_db}
    value = lambda key: float(features[key][stream])  # noqa: E731
    deesser_diagnostics = {
        "enabled": bool(r.deesser_enabled), "sibilance_excess_db": r.deesser_sibilance_excess_db, "peak_hz": r.deesser_peak_hz,
        "frame_evidence_available": bool(r.deesser_frame_evidence_available),
        "frame_evidence_confidence": r.deesser_frame_evidence_confidence, "detection_probability": r.deesser_detection_probability,
        "enable_probability_threshold": float(enable_probability_threshold), "model_version": DEESSER_MODEL_VERSION,
        "clip_features": dict(zip(DEESSER_CLIP_FEATURE_NAMES, (float(x) for x in r.deesser_clip_features))),
        "invalid_evidence": bool(r.deesser_invalid_evidence), "temporal_contrast_db": value("temporal_contrast_db"),
        "candidate_frame_ratio": value("candidate_frame_ratio"), "candidate_snr_db": value("candidate_snr_db")}
    compressor = {"enabled": True, "threshold_db": r.compressor_threshold_db, "ratio": r.compressor_ratio,
                  "attack_ms": r.compressor_attack_ms, "release_ms": r.compressor_release_ms,
                  "makeup_gain_db": r.compressor_makeup_gain_db, "adaptive_release": True,
                  "base_release_ms": r.compressor_base_release_ms, "auto_makeup_enabled": bool(r.compressor_auto_makeup_enabled),
                  "target_lufs": r.compressor_target_lufs, "sidechain_highpass_enabled": True,
                  "measured_short_term_lufs": value("short_term_lufs"), "measured_loudness_range_db": value("loudness_range_db"),
                  "dynamics_intensity": name, "target_p95_reduction_db": r.compressor_target_p95_db,
                  "peak_reduction_cap_db": r.compressor_peak_cap_db,
                  "noise_reference_reliability": r.compressor_noise_reference_reliability}
    compressor_diagnostics = {"auto_makeup_enabled": bool(r.compressor_auto_makeup_enabled), "target_lufs": r.compressor_target_lufs,
                              "dynamics_intensity": name, "target_p95_reduction_db": r.compressor_target_p95_db,
                              "target_median_reduction_db": r.compressor_target_median_db,
                              "peak_reduction_cap_db": r.compressor_peak_cap_db}
    return {"gate": gate, "deesser": deesser, "compressor": compressor, "deesser_diagnostics": deesser_diagnostics,
            "compressor_diagnostics": compressor_diagnostics, "capture_confidence": r.capture_confidence,
            "snr_confidence": r.snr_confidence, "speech_floor_db": r.speech_floor_db, "speech_body_db": r.speech_body_db,
            "speech_frame_peak_db": r.speech_frame_peak_db, "speech_snr_db": r.speech_snr_db}


def configure_voice_chain(engine: Engine, recommendation: Mapping[str, Any]) -> None:
    """Hand the gate, de-esser and compressor dicts of recommend_voice_chain to an engine's setters, unchanged.  vad_pre_gain
    has no setter (it only reaches a Silero instance, which this engine does not have) and is not applied."""
    gate, deesser, compressor = recommendation["gate"], recommendation["deesser"], recommendation["compressor"]
    engine.set_gate_enabled(int(gate["enabled"]))
    engine.gate_set_threshold(gate["threshold_db"])
    engine.gate_set_attack_time(gate["attack_ms"])
    engine.gate_set_release_time(gate["release_ms"])
    engine.gate_set_mode(int(gate["gate_mode"]))
    engine.gate_set_vad_threshold(gate["vad_threshold"])
    engine.gate_set_hold_time(gate["vad_hold_time_ms"])
    engine.gate_set_margin(gate["gate_margin_db"])
    engine.gate_set_auto_threshold(int(gate["auto_threshold_enabled"]))
    engine.set_deesser_enabled(int(deesser["enabled"]))
    engine.deesser_set_auto_enabled(int(deesser["auto_enabled"]))
    engine.deesser_set_auto_amount(deesser["auto_amount"])
    engine.deesser_set_low_cut_hz(deesser["low_cut_hz"])
    engine.deesser_set_high_cut_hz(deesser["high_cut_hz"])
    engine.deesser_set_threshold_db(deesser["threshold_db"])
    engine.deesser_set_ratio(deesser["ratio"])
    engine.deesser_set_attack_ms(deesser["attack_ms"])
    engine.deesser_set_release_ms(deesser["release_ms"])
    engine.deesser_set_max_reduction_db(deesser["max_reduction_db"])
    engine.set_compressor_enabled(int(compressor["enabled"]))
    engine.compressor_set_threshold(compressor["threshold_db"])
    engine.compressor_set_ratio(compressor["ratio"])
    engine.compressor_set_attack_time(compressor["attack_ms"])
    engine.compressor_set_release_time(compressor["release_ms"])
    engine.compressor_set_makeup_gain(compressor["makeup_gain_db"])
    engine.compressor_set_adaptive_release(int(compressor["adaptive_release"]))
    engine.compressor_set_base_release_time(compressor["base_release_ms"])
    engine.compressor_set_auto_makeup_enabled(int(compressor["auto_makeup_enabled"]))
    engine.compressor_set_target_lufs(compressor["target_lufs"])
    engine.compressor_set_sidechain_highpass_enabled(int(compressor["sidechain_highpass_enabled"]))
    engine.compressor_set_noise_reference_reliability(compressor["noise_reference_reliability"])


NOISE_MIN_DURATION_S, SPEECH_MIN_DURATION_S = 1.5, 3.0  # voice_setup.py:42-43


def recommend_voice_chain_batch(noise_audio, speech_audio, fs: int, target_preset: str = "broadcast", *, vad_probabilities=None,
                                noise_vad_probabilities=None, vad_available: bool = True, dynamics_intensity: str = "balanced",
                                custom_target_p95_db: float = 3.5, custom_peak_cap_db: float = 8.0, noise_metadata=None,
                                speech_metadata=None, device: int = 0, calibrate_compressor: bool = False, eq_settings=None,
                                device_rate: bool = False, offline_validation: bool = False, validate_eq_headroom: bool = False) -> list:
    """analyze_voice_setup (voice_setup.py:1082-1223) for every pair of noise_audio [n_streams, m] and speech_audio
    [n_streams, n] up to its three rule-based recommendations: analyze_voice_capture_batch (the noise reference, then the voice
    spectrum with the conservative spectrum as its override), the "balanced" smoothing of the median spectrum, the speech
    features against the conservative noise level, and the rules.  Per pair a dict with ``gate``, ``deesser``, ``compressor``
    (the reference's keys and value types), ``deesser_diagnostics``, ``compressor_diagnostics``, ``capture_confidence`` and
    ``features`` (the dict of measure_speech_features_batch), plus the level percentiles, the noise reference's status and
    conservative level and the spectrum's noise-referenced SNR behind them.

    vad_probabilities [n_streams, n_vad] are the voice capture's posteriors per 32 ms model window and
    noise_vad_probabilities [n_streams, k] the room tone's; the reference gets both from its native VAD helper.
    ``vad_available=True`` with no probabilities behaves as the reference does without that helper: the energy fallback, with
    gate_mode still 1.  ``vad_available=False`` ignores any probabilities, as the reference never asks for them then.  Captures
    below 1.5 s of room tone or 3 s of voice are refused with the reference's messages (:1099-1102).

    ``calibrate_compressor=True`` runs the reference's calibration search (voice_setup.py:742-1079; compressor_search.py) on
    every voice capture behind the EQ of ``eq_settings`` (band_freqs / band_gains / band_qs, one dict or one per stream: the
    Auto-EQ optimiser that makes them in the reference is not built) and the recommended de-esser: ``compressor`` is then the
    calibrated dict and ``compressor_calibration`` the search's diagnostics, as voice_setup.py:1241-1263 returns them; without
    ``eq_settings`` the calibration reads "unavailable" and the compressor stays, as in the reference when its EQ analysis
    failed.  With the default (False) the return is what it was: threshold_db is the rule's starting value.

    fs is 48000, or with ``device_rate=True`` any of SPEECH_FEATURES_RATES: the noise reference, the voice spectrum and the
    speech features then run at that rate (the loudness behind the resampling to 48 kHz of voice_setup.py:127-140).

    It does NOT return EQ bands (the Auto-EQ optimiser is not built).  With ``offline_validation=True`` every record gains a
    ``diagnostics`` dict with the reference's keys of voice_setup.py:1265-1364 (the setup passage through the recommended chain,
    the offline validation, the stage and setup confidences, uncertainty_reasons, weak_capture, apply_recommended); ``eq_settings``
    plays the role it plays for the calibration, and without it the flat bands apply and Auto-EQ counts as abstained.  48 kHz only.
    Without the keyword the return is what it was.

    ``validate_eq_headroom=True`` first takes the caller's ``eq_settings`` through apply_headroom_validation_batch (headroom.py) on
    the voice capture with default chain settings, as voice_setup.py:1227-1237 does with the optimiser's result: every record gains
    an ``eq`` key with the validated settings, and the calibration and the offline validation use their scaled gains.  Without the
    keyword the return is what it was."""
    noise, speech = np.asarray(noise_audio), np.asarray(speech_audio)
    if validate_eq_headroom and eq_settings is None:
        raise ValueError("validate_eq_headroom needs eq_settings")
    if noise.ndim != 2 or speech.ndim != 2 or noise.shape[0] != speech.shape[0]:
        raise ValueError("noise_audio and speech_audio must be [n_streams, m] and [n_streams, n]")
    if noise.shape[1] < int(fs * NOISE_MIN_DURATION_S):
        raise ValueError("Room-noise capture was too short for setup.")
    if speech.shape[1] < int(fs * SPEECH_MIN_DURATION_S):
        raise ValueError("Voice capture was too short for setup.")
    if not vad_available:
        vad_probabilities = noise_vad_probabilities = None
    sf = SpeechFeatures(fs, speech.shape[0], speech.shape[1], noise.shape[1], device, device_rate=device_rate)  # first: it refuses a rate
    try:
        references, spectra = analyze_voice_capture_batch(noise, speech, fs, noise_metadata=noise_metadata, speech_metadata=speech_metadata,
                                                          noise_vad_probabilities=noise_vad_probabilities,
                                                          speech_vad_probabilities=vad_probabilities, vad_probabilities=vad_probabilities,
                                                          device=device)
        vs = VoiceSpectrum(fs, 4096, device)
        try:
            smoothed = vs.smooth(np.stack([r.median_spectrum_db for r in spectra]))
        finally:
            vs.close()
        raw = sf.analyze(speech, [r.conservative_noise_rms_db for r in references], vad_probabilities, noise)
    finally:
        sf.close()
    features = _speech_features_dicts(raw)
    results = []
    for s, (reference, spectrum) in enumerate(zip(references, spectra)):
        rec = recommend_voice_chain(raw, s, spectrum.freqs, smoothed[s], residual_confidence=spectrum.residual_confidence,
                                    snr_db=spectrum.snr_db, used_single_spectrum_fallback=spectrum.used_single_spectrum_fallback,
                                    noise_quality_score=reference.quality_score, noise_status=reference.status,
                                    conservative_noise_rms_db=reference.conservative_noise_rms_db, target_preset=target_preset,
                                    vad_available=vad_available, dynamics_intensity=dynamics_intensity,
                                    custom_target_p95_db=custom_target_p95_db, custom_peak_cap_db=custom_peak_cap_db)
        rec.update(features=features[s], noise_reference_status=reference.status, noise_referenced_snr_db=float(spectrum.snr_db),
                   conservative_noise_rms_db=float(reference.conservative_noise_rms_db))
        results.append(rec)
    if validate_eq_headroom:
        from .headroom import apply_headroom_validation_batch

        eq_settings = apply_headroom_validation_batch(speech, fs, eq_settings, device=device)
        for rec, validated in zip(results, eq_settings):
            rec["eq"] = validated
    if calibrate_compressor:
        calibrations = [{"backend": "unavailable", "target_gain_reduction_db": 0.0, "measured_gain_reduction_db": 0.0, "iterations": 0}
                        for _ in results]  # voice_setup.py:1241-1246
        if eq_settings is not None:
            from .compressor_search import calibrate_compressor_batch

            pairs = calibrate_compressor_batch(
                speech, fs, eq_settings, [rec["deesser"] for rec in results], [rec["compressor"] for rec in results],
                [rec["compressor_diagnostics"]["target_p95_reduction_db"] for rec in results],
                [rec["compressor_diagnostics"]["target_median_reduction_db"] for rec in results],
                [rec["compressor_diagnostics"]["peak_reduction_cap_db"] for rec in results], device=device)
            for rec, (calibrated, _) in zip(results, pairs):
                rec["compressor"] = calibrated
            calibrations = [diagnostics for _, diagnostics in pairs]
        for rec, calibration in zip(results, calibrations):
            rec["compressor_calibration"] = calibration
    if offline_validation:
        if int(fs) != 48_000:
            raise NotImplementedError(f"sample rate {fs}: the offline validation is built for 48000 Hz")
        from .setup_verification import offline_validation_diagnostics

        for rec, diagnostics in zip(results, offline_validation_diagnostics(results, [r.reasons for r in references], speech, fs,
                                                                            eq_settings, device)):
            rec["diagnostics"] = diagnostics
    return results
