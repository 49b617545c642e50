"""The realtime loop's resampler protocol (dsp_loop.rs:963-1011, 843-895) on the CPU oracle, one stream: f32 samples go
into a queue as f64, `afo_resampler_process_chunk` (the stateful routine the pinned one-shot driver
`afo_simulate_product_resampler` calls, oracle/af_resampler.c) runs while a whole chunk is queued, and the produced frames
come back as f32.  Helper for the tests (CPU side of a comparison), not a test."""
from __future__ import annotations

import ctypes as C

import numpy as np

import af_oracle_py as O


def _lib() -> C.CDLL:
    L = O.lib()
    if L.afo_resampler_process_chunk.restype is not C.c_size_t:
        dp = C.POINTER(C.c_double)
        L.afo_resampler_new.restype = C.c_void_p
        L.afo_resampler_new.argtypes = [C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_int, C.c_float]
        L.afo_resampler_free.restype = None
        L.afo_resampler_free.argtypes = [C.c_void_p]
        L.afo_resampler_output_frames_max.restype = C.c_size_t
        L.afo_resampler_output_frames_max.argtypes = [C.c_void_p]
        L.afo_resampler_process_chunk.restype = C.c_size_t
        L.afo_resampler_process_chunk.argtypes = [C.c_void_p, dp, dp]
    return L


class StreamOracle:
    """One stream of the loop's protocol.  `push(x)` returns the f32 frames the wake-up produces; `push_f64(x)` the same
    frames before the cast (what the one-shot oracle's blocks hold)."""

    def __init__(self, input_rate: int, output_rate: int, chunk_size: int = 1024, sinc_len: int = 128, window: str = "blackman"):
        self.L = _lib()
        self.args = (int(input_rate), int(output_rate), int(chunk_size), int(sinc_len), O.RESAMPLER_WINDOWS[window], 0.0)
        self.chunk = int(chunk_size)
        self.h = None
        self.reset()

    def reset(self) -> None:
        """A fresh resampler: zero history, position -sinc_len / 2, nothing queued."""
        if self.h:
            self.L.afo_resampler_free(self.h)
        self.h = self.L.afo_resampler_new(*self.args)
        self.queue = np.zeros(0, dtype=np.float64)
        self._out = np.zeros(int(self.L.afo_resampler_output_frames_max(self.h)), dtype=np.float64)

    def clear_pending(self) -> None:
        """dsp_loop.rs:941-944: the queue is emptied; filter history and position stay."""
        self.queue = np.zeros(0, dtype=np.float64)

    def close(self) -> None:
        if self.h:
            self.L.afo_resampler_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def pending_input(self) -> int:
        return int(self.queue.size)

    def push_f64(self, x) -> np.ndarray:
        dp = C.POINTER(C.c_double)
        self.queue = np.concatenate([self.queue, np.asarray(x, dtype=np.float32).astype(np.float64)])  # `sample as f64`
        made = []
        while self.queue.size >= self.chunk:  # input_frames_next() == chunk_size
            block = np.ascontiguousarray(self.queue[: self.chunk])
            n = int(self.L.afo_resampler_process_chunk(self.h, block.ctypes.data_as(dp), self._out.ctypes.data_as(dp)))
            made.append(self._out[:n].copy())
            self.queue = self.queue[self.chunk :]
        return np.concatenate(made) if made else np.zeros(0, dtype=np.float64)

    def push(self, x) -> np.ndarray:
        return self.push_f64(x).astype(np.float32)  # `sample as f32`: round to nearest even


def run_calls(x: np.ndarray, calls, input_rate: int, output_rate: int, **kw) -> list[np.ndarray]:
    """One stream through a fresh StreamOracle in calls of the given lengths: the f32 output of every call."""
    o = StreamOracle(input_rate, output_rate, **kw)
    outs, at = [], 0
    for n in calls:
        outs.append(o.push(x[at : at + n]))
        at += n
    o.close()
    return outs


def plan_counts(calls, input_rate: int, output_rate: int, **kw) -> list[int]:
    """Frames each call of a fresh resampler produces (the positions never depend on the audio)."""
    return [y.size for y in run_calls(np.zeros(int(sum(calls)), dtype=np.float32), calls, input_rate, output_rate, **kw)]
