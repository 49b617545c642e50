"""ctypes front of tests/ref/vad_gate_ref.c: the reference's NoiseGate with a VadAutoGate::without_backend attached
(gate.rs:652-741 over vad.rs:714-966), and the front half of the engine's realtime chain on it, batched, in the style of
gate_oracle.py: scrub / clamp, DC block + 80 Hz high-pass, the gate fed one speech probability per control block, optionally
the suppressor and the dynamics chain.  Used by the tests only (CPU side of a comparison)."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "ref" / "vad_gate_ref.c"
LIB = HERE / "ref" / "libvad_gate_ref.so"
CFLAGS = ["-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-std=c11", "-Wall", "-Wextra"]

THRESHOLD_ONLY, VAD_ASSISTED, VAD_ONLY = 0, 1, 2
CLOSED, OPENING, OPEN, UNCERTAIN, RELEASING = range(5)
FUSED_GATE_OPEN_SCORE, FUSED_GATE_CLOSE_SCORE = np.float32(0.55), np.float32(0.35)
EXPANDER_RANGE_DB, VAD_ONLY_CONTINUOUS_SCALE = 36.0, 0.45
HISTORY_FRAMES = 250
UP_SLEW, DOWN_SLEW = np.float32(0.5), np.float32(0.1)
DEFAULT_CONTROLLER = dict(vad_threshold=0.48, hold_ms=200.0, margin_db=10.0, auto_threshold=True)
FRAME = 480


class Report(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("current_gain", "fused_gate_score", "vad_smoothed_probability", "noise_floor",
                                         "noise_floor_reliability", "last_rms_db", "last_threshold_db", "min_edge_distance_db",
                                         "hold_timer", "closed_counter_samples")] + \
               [(n, C.c_int32) for n in ("is_open", "gate_state", "auto_relax_active", "fused_gate_open", "held_open", "raw_open",
                                         "history_len", "visited_states")] + \
               [("chatter_event_count", C.c_uint64), ("vad_opened_below_level", C.c_uint32), ("floor_bin", C.c_int32)]


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
        vp, f, d, i, z = C.c_void_p, C.c_float, C.c_double, C.c_int, C.c_size_t
        fp = C.POINTER(C.c_float)
        sig = {
            "vgr_new": (vp, [d, d, d, d]), "vgr_free": (None, [vp]), "vgr_attach": (None, [vp, i, f]),
            "vgr_set_mode": (None, [vp, i]), "vgr_set_threshold": (None, [vp, d]), "vgr_set_attack_time": (None, [vp, d]),
            "vgr_set_release_time": (None, [vp, d]), "vgr_set_enabled": (None, [vp, i]),
            "vgr_set_external_vad_probability": (None, [vp, f, i]), "vgr_set_vad_threshold": (None, [vp, f]),
            "vgr_set_hold_time": (None, [vp, f]), "vgr_set_margin": (None, [vp, f]), "vgr_set_auto_threshold": (None, [vp, i]),
            "vgr_process_block": (None, [vp, fp, z]), "vgr_process_sample": (f, [vp, f]), "vgr_reset": (None, [vp]),
            "vgr_ctl_reset": (None, [vp]), "vgr_set_current_gain": (None, [vp, d]), "vgr_current_gain_f64": (d, [vp]),
            "vgr_apply_gain": (f, [vp, d, d]), "vgr_continuous_vad_gain_reduction_db": (d, [vp, i, f, i, i, f]),
            "vgr_is_vad_available": (i, [vp]), "vgr_report_state": (None, [vp, C.POINTER(Report)]),
            "vgr_ctl_process_with_probability": (i, [vp, fp, z, f]), "vgr_ctl_push_noise_floor_sample": (None, [vp, f]),
            "vgr_compute_rms_db": (f, [fp, z]), "vgr_db_to_linear": (d, [d]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _LIB = L
    return _LIB


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def compute_rms_db(x) -> float:
    a = np.ascontiguousarray(x, dtype=np.float32)
    return float(lib().vgr_compute_rms_db(_fptr(a), a.size))


def db_to_linear(db: float) -> float:
    return float(lib().vgr_db_to_linear(db))


class VadGate:
    """NoiseGate::new(threshold_db, attack_ms, release_ms, fs); the method names are the reference's."""

    def __init__(self, threshold_db=-40.0, attack_ms=10.0, release_ms=100.0, fs=48_000.0):
        self._l = lib()
        self._h = C.c_void_p(self._l.vgr_new(threshold_db, attack_ms, release_ms, fs))

    def __del__(self):
        if getattr(self, "_h", None):
            self._l.vgr_free(self._h)
            self._h = None

    def set_vad_auto_gate(self, vad_threshold: float | None):
        """Some(VadAutoGate::without_backend(fs, vad_threshold)), or None to detach."""
        self._l.vgr_attach(self._h, int(vad_threshold is not None), float(vad_threshold or 0.0))

    def set_gate_mode(self, mode): self._l.vgr_set_mode(self._h, int(mode))
    def set_threshold(self, db): self._l.vgr_set_threshold(self._h, float(db))
    def set_attack_time(self, ms): self._l.vgr_set_attack_time(self._h, float(ms))
    def set_release_time(self, ms): self._l.vgr_set_release_time(self._h, float(ms))
    def set_enabled(self, on): self._l.vgr_set_enabled(self._h, int(on))
    def set_external_vad_probability(self, p, available): self._l.vgr_set_external_vad_probability(self._h, float(p), int(available))
    def set_vad_threshold(self, v): self._l.vgr_set_vad_threshold(self._h, float(v))
    def set_hold_time(self, ms): self._l.vgr_set_hold_time(self._h, float(ms))
    def set_margin(self, db): self._l.vgr_set_margin(self._h, float(db))
    def set_auto_threshold(self, on): self._l.vgr_set_auto_threshold(self._h, int(on))
    def reset(self): self._l.vgr_reset(self._h)
    def reset_controller(self): self._l.vgr_ctl_reset(self._h)
    def set_current_gain(self, g): self._l.vgr_set_current_gain(self._h, float(g))
    def current_gain_f64(self): return float(self._l.vgr_current_gain_f64(self._h))
    def apply_gain(self, x, gr_db): return float(self._l.vgr_apply_gain(self._h, float(x), float(gr_db)))
    def is_vad_available(self): return bool(self._l.vgr_is_vad_available(self._h))
    def process_sample(self, x): return float(self._l.vgr_process_sample(self._h, float(x)))

    def continuous_vad_gain_reduction_db(self, mode, probability, available, held_open, vad_threshold):
        return float(self._l.vgr_continuous_vad_gain_reduction_db(self._h, int(mode), float(probability), int(available),
                                                                  int(held_open), float(vad_threshold)))

    def process_block_inplace(self, buf: np.ndarray) -> np.ndarray:
        assert buf.dtype == np.float32 and buf.flags.c_contiguous
        self._l.vgr_process_block(self._h, _fptr(buf), buf.size)
        return buf

    # the controller on its own (VadAutoGate::process_with_probability / push_noise_floor_sample)
    def ctl_process_with_probability(self, frame: np.ndarray, prob: float) -> bool:
        a = np.ascontiguousarray(frame, dtype=np.float32)
        return bool(self._l.vgr_ctl_process_with_probability(self._h, _fptr(a), a.size, float(prob)))

    def ctl_push_noise_floor_sample(self, db): self._l.vgr_ctl_push_noise_floor_sample(self._h, float(db))

    def report(self) -> Report:
        r = Report()
        self._l.vgr_report_state(self._h, C.byref(r))
        return r

    def current_gain(self): return float(self.report().current_gain)
    def gate_state(self): return int(self.report().gate_state)
    def fused_gate_score(self): return np.float32(self.report().fused_gate_score)
    def is_open(self): return bool(self.report().is_open)
    def chatter_event_count(self): return int(self.report().chatter_event_count)
    def auto_relax_active(self): return bool(self.report().auto_relax_active)
    def noise_floor(self): return np.float32(self.report().noise_floor)
    def noise_floor_reliability(self): return np.float32(self.report().noise_floor_reliability)


def controller(fs=48_000, vad_threshold=0.5) -> VadGate:
    """A VadAutoGate::without_backend(fs, vad_threshold) on its own (inside an otherwise unused gate)."""
    g = VadGate(-40.0, 10.0, 100.0, float(fs))
    g.set_vad_auto_gate(vad_threshold)
    return g


# ------------------------------------------------------------------ the engine's front half on the restatement
def apply_settings(g: VadGate, p: dict, ctl: dict | None, was_attached: bool) -> bool:
    """What the engine's live setters do between calls.  `p`: threshold_db / attack_ms / release_ms / mode; `ctl`: None
    (detached) or DEFAULT_CONTROLLER's keys.  The engine keeps the controller's settings engine-wide, so a controller that
    is attached (again) starts from fresh state with those settings."""
    if ctl is None:
        if was_attached:
            g.set_vad_auto_gate(None)
    elif not was_attached:
        g.set_vad_auto_gate(ctl["vad_threshold"])
    g.set_threshold(p["threshold_db"])
    g.set_attack_time(p["attack_ms"])
    g.set_release_time(p["release_ms"])
    g.set_gate_mode(p["mode"])
    if ctl is not None:
        g.set_vad_threshold(ctl["vad_threshold"])
        g.set_hold_time(ctl["hold_ms"])
        g.set_margin(ctl["margin_db"])
        g.set_auto_threshold(ctl["auto_threshold"])
    return ctl is not None


def run_stream(x, fs, calls, gate_params, controllers, evidence, block, *, prefilter=True, clamp=False, suppressor=None,
               chain=None):
    """One stream.  `gate_params` / `controllers`: one entry or one per call.  `evidence`: per call None (probability 0, not
    available) or (probabilities[blocks], available[blocks]) over that call's gate pass cut into `block`-sample chunks.
    Returns (output float32, VadGate, per-block records of the last call)."""
    import af_oracle_py as O
    import chain_oracle as CO
    import gate_oracle as GO

    n_calls = len(calls)
    per_call = [gate_params] * n_calls if isinstance(gate_params, dict) else list(gate_params)
    per_ctl = [controllers] * n_calls if (controllers is None or isinstance(controllers, dict)) else list(controllers)
    out_calls = GO.output_calls(calls, suppressor)
    m = int(sum(out_calls))
    y = CO.sanitize(x[: int(sum(calls))], clamp)[:m]
    if prefilter:
        y = O.prefilter(y, fs)
    y = np.ascontiguousarray(y, dtype=np.float32)
    g = VadGate(per_call[0]["threshold_db"], per_call[0]["attack_ms"], per_call[0]["release_ms"], fs)
    attached = False
    gated = np.empty(m, dtype=np.float32)
    at = 0
    records = []
    for ci, length in enumerate(out_calls):
        attached = apply_settings(g, per_call[ci], per_ctl[ci], attached)
        ev = evidence[ci] if evidence is not None else None
        records = []
        for b, t0 in enumerate(range(0, length, block)):
            n = min(block, length - t0)
            if ev is None:
                g.set_external_vad_probability(0.0, False)
            else:
                g.set_external_vad_probability(float(ev[0][b]), bool(ev[1][b]))
            buf = y[at + t0 : at + t0 + n].copy()
            g.process_block_inplace(buf)
            gated[at + t0 : at + t0 + n] = buf
            r = g.report()
            records.append((r.held_open, r.floor_bin, r.noise_floor))  # per block of the call: decision, floor's bin, floor
        at += length
    if suppressor == "wrapper":
        sig = O.suppressor_process(gated, 1.0)
    elif suppressor == "raw":
        sig = O.rnnoise_benchmark_frames(gated)
    else:
        sig = gated
    if chain is None:
        return np.asarray(sig, dtype=np.float32), g, records
    bands, settings = chain
    out, _ = CO.run_calls(sig, fs, bands, settings, [c for c in out_calls if c > 0])
    return out, g, records


STATE_KEYS = ("current_gain", "chatter_events", "is_open", "auto_relax_active", "gate_state", "fused_score", "probability",
              "noise_floor_db", "noise_floor_reliability", "held_open", "floor_bin", "min_edge_distance_db", "visited_states",
              "vad_opened_below_level", "history_len", "block_held_open", "block_floor_bin", "block_noise_floor")
# (the block_* entries: [len(streams), blocks of the last call])


def run_batch(audio, fs, calls, gate_params, controllers, evidence, block, *, prefilter=True, clamp=False, suppressor=None,
              chain=None, streams=None, workers=16):
    """run_stream over `streams` of [n_streams, n].  `evidence`: per call None or (probabilities, available), each [blocks]
    (shared) or [blocks, n_streams].  Returns (output [len(streams), samples], state dict of arrays)."""
    import gate_oracle as GO

    GO.warm_up()
    lib()
    streams = list(range(audio.shape[0])) if streams is None else list(streams)
    m = int(sum(GO.output_calls(calls, suppressor)))
    out = np.empty((len(streams), m), dtype=np.float32)
    st = {k: [None] * len(streams) for k in STATE_KEYS}

    def stream_evidence(s):
        if evidence is None:
            return None
        res = []
        for ev in evidence:
            if ev is None:
                res.append(None)
            else:
                p, a = np.asarray(ev[0]), np.asarray(ev[1])
                res.append((p[:, s] if p.ndim == 2 else p, a[:, s] if a.ndim == 2 else a))
        return res

    def one(i):
        s = streams[i]
        out[i], g, rec = run_stream(audio[s], fs, calls, gate_params, controllers, stream_evidence(s), block,
                                    prefilter=prefilter, clamp=clamp, suppressor=suppressor, chain=chain)
        r = g.report()
        vals = (r.current_gain, r.chatter_event_count, bool(r.is_open), bool(r.auto_relax_active), r.gate_state,
                r.fused_gate_score, r.vad_smoothed_probability, r.noise_floor, r.noise_floor_reliability, bool(r.held_open),
                r.floor_bin, r.min_edge_distance_db, r.visited_states, r.vad_opened_below_level, r.history_len,
                [bool(b[0]) for b in rec], [b[1] for b in rec], [np.float32(b[2]) for b in rec])
        for k, v in zip(STATE_KEYS, vals):
            st[k][i] = v

    with ThreadPoolExecutor(max_workers=max(1, min(workers, len(streams)))) as pool:
        list(pool.map(one, range(len(streams))))
    return out, {k: np.asarray(v) for k, v in st.items()}
