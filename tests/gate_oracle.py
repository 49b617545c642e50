"""The front half of the engine's realtime chain on the oracle, batched: scrub / clamp, DC block + 80 Hz high-pass
(`prefilter`), the noise gate (`Gate`, one object per stream across the engine's calls, its parameters set between calls
as the engine's live setters set them), optionally the suppressor (`suppressor_process`, or `rnnoise_benchmark_frames`
for the raw protocol), then the dynamics chain over the engine's own call lengths (`chain_oracle.run_calls`).  Returns the
output and each stream's gate state at the end of the last call.  Used by the tests only (CPU side of a comparison)."""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import af_oracle_py as O
import chain_oracle as CO

DEFAULT_GATE = dict(threshold_db=-40.0, attack_ms=10.0, release_ms=100.0, mode=0)  # NoiseGate::new(-40, 10, 100, fs)
FRAME = 480


def _set_params(g: O.Gate, p: dict, fs: float) -> None:
    """What af_gate_set_threshold / _attack_time / _release_time / _mode do between calls (coefficients derived by the
    oracle's own gate.rs:158-225 arithmetic)."""
    fresh = O.Gate(p["threshold_db"], p["attack_ms"], p["release_ms"], fs)
    g.s.threshold_db = fresh.s.threshold_db
    g.s.attack_coeff = fresh.s.attack_coeff
    g.s.release_coeff = fresh.s.release_coeff
    O.lib().afo_gate_set_vad_mode(C.byref(g.s), int(p["mode"] != 0))


def output_calls(calls, suppressor: str | None) -> list[int]:
    """The samples each engine call returns: the call itself, or behind the suppressor the whole frames complete by then."""
    if not suppressor:
        return [int(c) for c in calls]
    out, total, done = [], 0, 0
    for c in calls:
        total += int(c)
        whole = (total // FRAME) * FRAME
        out.append(whole - done)
        done = whole
    return out


def run_stream(x: np.ndarray, fs: float, calls, gate_params, *, prefilter: bool = True, clamp: bool = False,
               suppressor: str | None = None, chain=None):
    """One stream.  `gate_params`: one dict (DEFAULT_GATE's keys) or one per call.  `suppressor`: None, "wrapper" or "raw".
    `chain`: None (the gated / suppressed signal itself) or (bands, settings).  Returns (output float32, Gate)."""
    per_call = [gate_params] * len(calls) if isinstance(gate_params, dict) else list(gate_params)
    out_calls = output_calls(calls, suppressor)
    m = int(sum(out_calls))
    y = CO.sanitize(x[: int(sum(calls))], clamp)[:m]
    if prefilter:
        y = O.prefilter(y, fs)
    g = O.Gate(per_call[0]["threshold_db"], per_call[0]["attack_ms"], per_call[0]["release_ms"], fs,
               vad_mode=per_call[0]["mode"] != 0)
    gated = np.empty(m, dtype=np.float32)
    at = 0
    for length, p in zip(out_calls, per_call):  # (behind the suppressor the gate runs on the frames each call completes)
        _set_params(g, p, fs)
        gated[at : at + length] = g.process(y[at : at + length])
        at += length
    if suppressor == "wrapper":
        sig = O.suppressor_process(gated, 1.0)
    elif suppressor == "raw":
        sig = O.rnnoise_benchmark_frames(gated)
    else:
        sig = gated
    if chain is None:
        return np.asarray(sig, dtype=np.float32), g
    bands, settings = chain
    out, _ = CO.run_calls(sig, fs, bands, settings, [c for c in out_calls if c > 0])
    return out, g


def gate_state(g: O.Gate) -> tuple[float, int, bool, bool]:
    """(current_gain as float32, chatter events, is_open, auto-relax armed): what Engine.gate_state() reports."""
    return g.current_gain, g.chatter_event_count, g.is_open, g.s.auto_relax_remaining_samples > 0


def warm_up() -> None:
    """Load the oracle, set its ctypes signatures and fill the RNNoise restatement's lazily built static tables on this
    thread, before any worker thread starts."""
    CO._lib()
    O.Gate().process(np.zeros(4, np.float32))
    O.prefilter(np.zeros(4, np.float32))
    O.suppressor_process(np.zeros(2 * FRAME, np.float32))
    O.rnnoise_benchmark_frames(np.zeros(2 * FRAME, np.float32))


def run_batch(audio: np.ndarray, fs: float, calls, gate_params=DEFAULT_GATE, *, prefilter: bool = True, clamp: bool = False,
              suppressor: str | None = None, chain=None, streams=None, workers: int = 16):
    """run_stream over the streams `streams` (default: all) of [n_streams, n] on up to `workers` threads.
    Returns (output [len(streams), samples], state dict with arrays like Engine.gate_state())."""
    warm_up()
    streams = list(range(audio.shape[0])) if streams is None else list(streams)
    m = int(sum(output_calls(calls, suppressor)))
    out = np.empty((len(streams), m), dtype=np.float32)
    gain = np.empty(len(streams), dtype=np.float32)
    events = np.empty(len(streams), dtype=np.uint64)
    is_open = np.empty(len(streams), dtype=bool)
    relax = np.empty(len(streams), dtype=bool)

    def one(i):
        out[i], g = run_stream(audio[streams[i]], fs, calls, gate_params, prefilter=prefilter, clamp=clamp,
                               suppressor=suppressor, chain=chain)
        gain[i], events[i], is_open[i], relax[i] = gate_state(g)

    with ThreadPoolExecutor(max_workers=max(1, min(workers, len(streams)))) as pool:
        list(pool.map(one, range(len(streams))))
    return out, {"current_gain": gain, "chatter_events": events, "is_open": is_open, "auto_relax_active": relax}
