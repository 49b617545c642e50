"""ctypes front of tests/ref/mixdown_ref.c: the reference's input mixdown (input.rs:84-135, 383-736) and its callback wrapper
(input.rs:789-842), one object per stream, f32 input.  Used by the tests only (CPU side of a comparison)."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "ref" / "mixdown_ref.c"
LIB = HERE / "ref" / "libmixdown_ref.so"
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=c11", "-Wall", "-Wextra"]

AVERAGE, LEFT, RIGHT, MAX_RMS, PHASE_SAFE_MONO = range(5)
MODE_IDS = ("average", "left", "right", "max_rms", "phase_safe_mono")  # input.rs:158-180
NONE, POLARITY_FLIP, FRACTIONAL_DELAY, MAX_RMS_FALLBACK = range(4)
STRATEGY_NAMES = ("none", "polarity_flip", "fractional_delay", "max_rms_fallback")  # input.rs:49-56
WARNING_CORRELATION = np.float32(-0.75)
HISTORY, LATENCY, CHUNK = 16, 2, 8192
COUNTERS = ("strategy_none", "strategy_flip", "strategy_fractional", "strategy_fallback", "warm_up", "lagrange_clamp",
            "best_delay_edge", "parabola_flat", "parabola_missing", "delayed_none_short", "delayed_none_denom", "stereo_none",
            "hysteresis_reused", "hysteresis_cleared", "tie")


def build(force: bool = False) -> pathlib.Path:
    """Compile the restatement next to its source (git-ignored) unless it is there and newer than the source."""
    if force or not LIB.exists() or LIB.stat().st_mtime < SRC.stat().st_mtime:
        subprocess.run(["gcc", *CFLAGS, "-shared", "-o", str(LIB), str(SRC), "-lm"], check=True)
    return LIB


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(str(build()))
        vp, f, i, z = C.c_void_p, C.c_float, C.c_int, C.c_size_t
        fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_uint64)
        sig = {
            "mdr_new": (vp, [i, i]), "mdr_free": (None, [vp]), "mdr_set_mode": (None, [vp, i]), "mdr_mode": (i, [vp]),
            "mdr_reset": (None, [vp]), "mdr_callback": (None, [vp, fp, z, fp]),
            "mdr_diagnostics": (None, [vp, fp, up, ip, fp, ip]), "mdr_counters": (None, [vp, up]), "mdr_counter_count": (i, []),
            "mdr_state": (None, [vp, fp, ip, ip, ip, fp]), "mdr_mix": (z, [vp, fp, z, fp, z, ip, fp, ip, fp, ip]),
            "mdr_lagrange_sample": (f, [fp, f]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        assert L.mdr_counter_count() == len(COUNTERS)
        _LIB = L
    return _LIB


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def lagrange_sample(history, delay: float) -> np.float32:
    """PhaseSafeMonoState::lagrange_sample on a 16-frame history (newest first)."""
    h = np.ascontiguousarray(history, dtype=np.float32)
    assert h.size == HISTORY
    return np.float32(lib().mdr_lagrange_sample(_fptr(h), float(delay)))


class Mixdown:
    """One input stream: its channel count, the live mode, a PhaseSafeMonoState and the callback's diagnostics."""

    def __init__(self, n_channels: int, mode: int = AVERAGE):
        self._l = lib()
        self.n_channels = int(n_channels)
        self._h = C.c_void_p(self._l.mdr_new(int(n_channels), int(mode)))

    def __del__(self):
        if getattr(self, "_h", None):
            self._l.mdr_free(self._h)
            self._h = None

    def set_mode(self, mode: int): self._l.mdr_set_mode(self._h, int(mode))
    def mode(self) -> int: return int(self._l.mdr_mode(self._h))
    def reset(self): self._l.mdr_reset(self._h)

    def callback(self, data) -> np.ndarray:
        """The input callback on [frames, channels] (or interleaved 1-D) f32 data -> mono [frames]."""
        a = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
        frames = a.size // self.n_channels
        out = np.empty(frames, dtype=np.float32)
        self._l.mdr_callback(self._h, _fptr(a), frames, _fptr(out))
        return out

    def mix(self, interleaved, mono_len: int):
        """mix_interleaved_to_mono_with_mode_and_state on this object's state: (written, mono, correlation | None,
        (strategy, estimated_delay, polarity_flipped)).  `mono` is returned whole; slots past `written` keep `fill`."""
        a = np.ascontiguousarray(interleaved, dtype=np.float32).reshape(-1)
        mono = np.zeros(mono_len, dtype=np.float32)
        some, strat, flipped = C.c_int(), C.c_int(), C.c_int()
        corr, delay = C.c_float(), C.c_float()
        w = self._l.mdr_mix(self._h, _fptr(a), a.size, _fptr(mono), mono_len, C.byref(some), C.byref(corr), C.byref(strat),
                            C.byref(delay), C.byref(flipped))
        return int(w), mono, (np.float32(corr.value) if some.value else None), (strat.value, np.float32(delay.value), bool(flipped.value))

    def diagnostics(self) -> dict:
        corr, delay = C.c_float(), C.c_float()
        warn = C.c_uint64()
        strat, flipped = C.c_int(), C.c_int()
        self._l.mdr_diagnostics(self._h, C.byref(corr), C.byref(warn), C.byref(strat), C.byref(delay), C.byref(flipped))
        return dict(stereo_correlation=np.float32(corr.value), phase_warning_count=int(warn.value), strategy=int(strat.value),
                    estimated_delay=np.float32(delay.value), polarity_flipped=bool(flipped.value))

    def counters(self) -> dict:
        buf = (C.c_uint64 * len(COUNTERS))()
        self._l.mdr_counters(self._h, buf)
        return dict(zip(COUNTERS, (int(v) for v in buf)))

    def state(self) -> dict:
        hist = np.empty((2, HISTORY), dtype=np.float32)
        lc = np.empty(3, dtype=np.float32)
        filled, valid, strat = C.c_int(), C.c_int(), C.c_int()
        self._l.mdr_state(self._h, _fptr(hist), C.byref(filled), C.byref(valid), C.byref(strat), _fptr(lc))
        return dict(history=hist, filled=filled.value, last_candidate=(None if not valid.value else
                                                                       (strat.value, lc[0], lc[1], lc[2])))


def mix_with_mode(interleaved, n_channels: int, mode: int, mono_len: int):
    """mix_interleaved_to_mono_with_mode (input.rs:639-657): a fresh state per call."""
    return Mixdown(n_channels, mode).mix(interleaved, mono_len)


DIAG_KEYS = ("stereo_correlation", "phase_warning_count", "strategy", "estimated_delay", "polarity_flipped")
_DIAG_DTYPES = dict(stereo_correlation=np.float32, phase_warning_count=np.uint64, strategy=np.int32, estimated_delay=np.float32,
                    polarity_flipped=np.int32)


class Batch:
    """`n_streams` independent streams of one channel count and one (live) mode: what af_mixdown is compared against."""

    def __init__(self, n_channels: int, mode: int, n_streams: int):
        self.streams = [Mixdown(n_channels, mode) for _ in range(n_streams)]

    def set_mode(self, mode: int):
        for m in self.streams:
            m.set_mode(mode)

    def reset(self):
        for m in self.streams:
            m.reset()

    def push(self, x: np.ndarray) -> np.ndarray:
        """[streams, frames, channels] -> [streams, frames]"""
        return np.stack([m.callback(x[s]) for s, m in enumerate(self.streams)]) if x.shape[1] else \
            np.zeros((len(self.streams), 0), dtype=np.float32)

    def diagnostics(self) -> dict:
        rows = [m.diagnostics() for m in self.streams]
        return {k: np.asarray([r[k] for r in rows], dtype=_DIAG_DTYPES[k]) for k in DIAG_KEYS}

    def counters(self) -> list:
        return [m.counters() for m in self.streams]
