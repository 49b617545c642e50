"""ctypes front of tests/ref/output_writer_ref.c: the reference's output writer (output_writer.rs:62-343 over
resampling.rs:81-120, routing.rs:651-655, 697-703, 768-799) in front of a modelled queue, one object per stream.  The
true-peak limiter and detector are the built oracle's afo_tp_*.  Used by the tests only (CPU side of a comparison)."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
ORACLE = HERE.parent / "oracle"
SRC = HERE / "ref" / "output_writer_ref.c"
LIB = HERE / "ref" / "liboutput_writer_ref.so"
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=c11", "-Wall", "-Wextra"]

MAX_BLOCK = 8672
BRANCHES = ("pass_through", "expanded", "compressed", "emergency", "out_len_one", "max_src_clamp", "fade_continued",
            "fade_ended_inside", "short_write", "zero_free", "limiter_off", "limited", "clip", "non_finite")
COUNTERS = ("jitter_dropped", "retime_adjustments", "recovery_events", "short_write_dropped", "clip_events", "true_peak_events")
DB = ("clip_peak_db", "true_peak_db", "true_peak_input_db", "gain_reduction_db", "gain_reduction_history_db", "headroom_db")
LINEAR = ("input_true_peak", "limiter_output_true_peak", "detector_true_peak", "min_gain", "max_clipped")


def build(force: bool = False) -> pathlib.Path:
    """Compile the restatement next to its source (git-ignored), linked against the built oracle."""
    oracle_lib = ORACLE / "libaf_oracle.so"
    if not oracle_lib.exists():
        subprocess.run(["make", "-C", str(ORACLE)], check=True)
    stale = not LIB.exists() or LIB.stat().st_mtime < max(SRC.stat().st_mtime, oracle_lib.stat().st_mtime)
    if force or stale:
        subprocess.run(["gcc", *CFLAGS, "-shared", "-o", str(LIB), str(SRC), f"-I{ORACLE}", f"-L{ORACLE}", "-laf_oracle",
                        "-Wl,-rpath,$ORIGIN/../../oracle", "-lm"], check=True)
    return LIB


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(str(build()))
        vp, f, i, z = C.c_void_p, C.c_float, C.c_int, C.c_size_t
        fp, up, zp = C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.POINTER(C.c_size_t)
        sig = {
            "owr_duration_samples": (z, [C.c_uint32, C.c_uint32]), "owr_default_limits": (None, [C.c_uint32, zp, zp, zp, zp]),
            "owr_new": (vp, [f, z, z, z, z, z]), "owr_free": (None, [vp]), "owr_reset": (None, [vp]),
            "owr_set_limiter": (None, [vp, i, f]), "owr_set_state": (None, [vp, f, z]),
            "owr_retime": (z, [fp, z, f, z, z, fp, up]), "owr_update_decaying_peak_db": (None, [f, fp, f]),
            "owr_sanitize_and_clamp": (None, [fp, z, f, up, fp, fp]), "owr_write_chunk": (z, [vp, fp, z, z, i, fp]),
            "owr_branch_count": (i, []), "owr_branches": (None, [vp, up]), "owr_counters": (None, [vp, up]),
            "owr_meters": (None, [vp, fp, fp, fp, fp, C.POINTER(C.c_int64)]),
            "owr_state": (None, [vp, fp, fp, C.POINTER(C.c_int32), fp]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        assert L.owr_branch_count() == len(BRANCHES)
        _LIB = L
    return _LIB


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def duration_samples(rate: int, ms: int) -> int:
    return int(lib().owr_duration_samples(rate, ms))


def default_limits(rate: int) -> dict:
    """dsp_loop.rs:781-795, :204: capacity, target centre, hard backlog, fade frames."""
    v = [C.c_size_t() for _ in range(4)]
    lib().owr_default_limits(rate, *[C.byref(x) for x in v])
    return dict(zip(("capacity", "center", "hard", "fade"), (int(x.value) for x in v)))


def retime(x, ratio: float, max_output_len: int, scratch_capacity: int = MAX_BLOCK * 16) -> np.ndarray:
    """retime_audio_block (resampling.rs:81-120)."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    out = np.zeros(max(min(max_output_len, scratch_capacity), a.size, 1), dtype=np.float32)
    n = lib().owr_retime(_fptr(a), a.size, float(ratio), max_output_len, scratch_capacity, _fptr(out), None)
    return out[:n].copy()


def update_decaying_peak_db(value_db: float, history: float, decay: float) -> np.float32:
    h = C.c_float(history)
    lib().owr_update_decaying_peak_db(float(value_db), C.byref(h), float(decay))
    return np.float32(h.value)


def sanitize_and_clamp(x, ceiling: float, clip_events: int = 0, clip_peak_db: float = -120.0):
    """sanitize_and_clamp_output_inplace_with_metrics: (buffer, clip events, clip peak dB, max clipped amplitude)."""
    a = np.array(x, dtype=np.float32)
    ev, pk, mx = C.c_uint64(clip_events), C.c_float(clip_peak_db), C.c_float()
    lib().owr_sanitize_and_clamp(_fptr(a), a.size, float(ceiling), C.byref(ev), C.byref(pk), C.byref(mx))
    return a, int(ev.value), np.float32(pk.value), np.float32(mx.value)


class Writer:
    """One stream: an OutputWriteContext with its limits, limiter, detector, counters and a modelled queue."""

    def __init__(self, rate: float = 48_000.0, capacity: int | None = None, center: int | None = None, hard: int | None = None,
                 fade: int | None = None, scratch_capacity: int = 0):
        self._l = lib()
        d = default_limits(int(rate))
        self.capacity = d["capacity"] if capacity is None else int(capacity)
        self.center = d["center"] if center is None else int(center)
        self.hard = d["hard"] if hard is None else int(hard)
        self.fade = d["fade"] if fade is None else int(fade)
        self._h = C.c_void_p(self._l.owr_new(float(rate), self.capacity, self.center, self.hard, self.fade, scratch_capacity))

    def __del__(self):
        if getattr(self, "_h", None):
            self._l.owr_free(self._h)
            self._h = None

    def reset(self): self._l.owr_reset(self._h)
    def set_limiter(self, enabled: bool, ceiling_linear: float): self._l.owr_set_limiter(self._h, int(bool(enabled)), float(ceiling_linear))
    def set_state(self, ema: float, fade_remaining: int): self._l.owr_set_state(self._h, float(ema), int(fade_remaining))

    def write_chunk(self, x, fill: int, clean_path: bool = False) -> np.ndarray:
        """write_chunk with `fill` frames in the queue: the frames that reached the queue."""
        a = np.ascontiguousarray(x, dtype=np.float32)
        assert a.size <= 8192 and 0 <= fill <= self.capacity
        out = np.zeros(MAX_BLOCK, dtype=np.float32)
        n = self._l.owr_write_chunk(self._h, _fptr(a), a.size, int(fill), int(bool(clean_path)), _fptr(out))
        return out[:n].copy()

    def branches(self) -> dict:
        buf = (C.c_uint64 * len(BRANCHES))()
        self._l.owr_branches(self._h, buf)
        return dict(zip(BRANCHES, (int(v) for v in buf)))

    def counters(self) -> dict:
        buf = (C.c_uint64 * len(COUNTERS))()
        self._l.owr_counters(self._h, buf)
        return dict(zip(COUNTERS, (int(v) for v in buf)))

    def meters(self) -> dict:
        db, lin = np.zeros(6, dtype=np.float32), np.zeros(5, dtype=np.float32)
        ratio, ema = C.c_float(), C.c_float()
        rec = (C.c_int64 * 4)()
        self._l.owr_meters(self._h, _fptr(db), _fptr(lin), C.byref(ratio), C.byref(ema), rec)
        m = dict(zip(DB, db))
        m.update(zip(LINEAR, lin))
        m.update(ratio=np.float32(ratio.value), ema=np.float32(ema.value), out_len=int(rec[0]), fade_remaining=int(rec[1]),
                 fill_after=int(rec[2]), free=int(rec[3]))
        return m

    def state(self) -> dict:
        gain, widx = C.c_float(), C.c_int32()
        delay, hist = np.zeros(20, dtype=np.float32), np.zeros((3, 32), dtype=np.float32)
        self._l.owr_state(self._h, C.byref(gain), _fptr(delay), C.byref(widx), _fptr(hist))
        return dict(gain=np.float32(gain.value), delay=delay, write_idx=int(widx.value), histories=hist)


METER_DTYPES = {**{k: np.float32 for k in DB + LINEAR}, "ratio": np.float32, "ema": np.float32, "out_len": np.int64,
                "fade_remaining": np.int64, "fill_after": np.int64, "free": np.int64}


class Batch:
    """`n_streams` independent writers of one configuration: what af_output_writer is compared against."""

    def __init__(self, n_streams: int, **kw):
        self.streams = [Writer(**kw) for _ in range(n_streams)]

    def reset(self):
        for w in self.streams:
            w.reset()

    def set_limiter(self, enabled: bool, ceiling_linear: float):
        for w in self.streams:
            w.set_limiter(enabled, ceiling_linear)

    def push(self, x: np.ndarray, fill, clean_path: bool = False) -> list:
        """[streams, frames] and fill[streams] -> one row per stream, each of its own length"""
        return [w.write_chunk(x[s], int(fill[s]), clean_path) for s, w in enumerate(self.streams)]

    def counters(self) -> dict:
        rows = [w.counters() for w in self.streams]
        return {k: np.asarray([r[k] for r in rows], dtype=np.uint64) for k in COUNTERS}

    def meters(self) -> dict:
        rows = [w.meters() for w in self.streams]
        return {k: np.asarray([r[k] for r in rows], dtype=t) for k, t in METER_DTYPES.items()}

    def state(self) -> dict:
        rows = [w.state() for w in self.streams]
        return dict(gain=np.asarray([r["gain"] for r in rows], dtype=np.float32), delay=np.stack([r["delay"] for r in rows]),
                    write_idx=np.asarray([r["write_idx"] for r in rows], dtype=np.int32),
                    histories=np.stack([r["histories"] for r in rows]))

    def branches(self) -> dict:
        rows = [w.branches() for w in self.streams]
        return {k: sum(r[k] for r in rows) for k in BRANCHES}


def run_sequence(pushes, n_streams: int, **kw) -> list:
    """A stimulus sequence (tests/output_writer_stimulus.py) through a fresh Batch: per push the rows, counters, meters, state."""
    batch = Batch(n_streams, **kw)
    steps = []
    for p in pushes:
        for action in p["pre"]:
            if action[0] == "limiter":
                batch.set_limiter(action[1], action[2])
            else:
                batch.reset()
        rows = batch.push(p["x"], p["fill"], p["clean_path"])
        steps.append(dict(rows=rows, counters=batch.counters(), meters=batch.meters(), state=batch.state(), branches=batch.branches()))
    return steps
