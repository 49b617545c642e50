"""Stimulus, chain configuration and retune schedules shared by the live-control tests (tests/test_retune_oracle.py on the
CPU, tests/test_gpu_live_control.py on the GPU).  Not a test module."""
from __future__ import annotations

import numpy as np

import signals as S

FS = 48_000
# A 72-sample crossfade (1.5 ms) scheduled before call 1 is still running at the next boundary (50 of 72 done) and ends
# inside call 2; a 7-sample call; calls that are no multiple of the 960-sample control block.
CALLS = (960, 50, 30, 480, 7, 1000, 960)
N = sum(CALLS)
GAIN = 2.0       # the KAT voice 6 dB hotter: with the make-up gain below the compressor's output sits above the ceiling, and
SKIP = 4 * 480   # (past the KAT's quiet first blocks) the limiter's output keeps the true-peak limiter working as well
SIBILANT_SKIP = 83 * 480  # the de-esser runs start inside one of the KAT's sibilant bursts: >= 2 dB of de-essing from the first block on

# tests/signals.py's limiter settings: compressor on (-20 dB, 4:1, 10 / 200 ms, side-chain high-pass on, fixed release),
# limiter at -1.5 dB effective, 2 ms lookahead -- with make-up gain so that both limiters work all the time
SETTINGS = dict(S.limiter_settings(2.0), compressor_makeup_gain_db=14.0)
BANDS = S.LIMITER_BANDS

SCHEDULE = {
    1: [("eq_set_band_gain", (3, 6.0))],
    2: [("eq_set_band_gain", (3, -4.0)),  # 22 crossfade samples left: restarts from the live state
        ("eq_set_band_config", (7, ("notch", 4021.2060546875, 0.0, 2.0, 12, True)))],  # a bell becomes a notch
    3: [("compressor_set_threshold", (-16.0,)), ("compressor_set_ratio", (3.0,)), ("compressor_set_attack_time", (4.0,)),
        ("compressor_set_release_time", (120.0,)), ("compressor_set_base_release_time", (90.0,)),
        ("compressor_set_makeup_gain", (15.0,))],
    4: [("limiter_set_ceiling", (-3.0,)), ("limiter_set_release_time", (30.0,)), ("true_peak_limiter_set_release_ms", (40.0,))],
    5: [("compressor_set_adaptive_release", (1,)), ("compressor_set_sidechain_highpass_enabled", (0,))],
}

# the de-esser as tests/test_gpu_deesser.py configures it, and its retunes between calls
DEESSER_SETTERS = [("deesser_set_auto_enabled", (1,)), ("deesser_set_auto_amount", (0.7,)), ("deesser_set_low_cut_hz", (3500.0,)),
                   ("deesser_set_high_cut_hz", (9000.0,)), ("deesser_set_threshold_db", (-40.0,)), ("deesser_set_ratio", (6.0,)),
                   ("deesser_set_attack_ms", (1.0,)), ("deesser_set_release_ms", (60.0,)), ("deesser_set_max_reduction_db", (8.0,))]
DEESSER_SCALARS = {
    2: [("deesser_set_threshold_db", (-34.0,)), ("deesser_set_ratio", (3.0,))],
    4: [("deesser_set_max_reduction_db", (5.0,)), ("deesser_set_auto_amount", (0.9,))],
}
DEESSER_CUTS = {1: [("deesser_set_low_cut_hz", (4200.0,)), ("deesser_set_high_cut_hz", (10_000.0,))]}


def merged(*schedules) -> dict:
    out: dict = {}
    for sched in schedules:
        for k, items in sched.items():
            out.setdefault(k, []).extend(items)
    return dict(sorted(out.items()))


_AUDIO: dict = {}


def audio(n_streams: int, n: int = N, skip: int = SKIP) -> np.ndarray:
    """[n_streams, n] float32: the per-stream KAT voices of tests/signals.py, loud."""
    key = (n_streams, n, skip)
    if key not in _AUDIO:
        blocks = (skip + n + 479) // 480
        rows = [S.kat_signal(blocks, *S.stream_params(s))[skip : skip + n] for s in range(n_streams)]
        _AUDIO[key] = np.ascontiguousarray(np.stack(rows) * np.float32(GAIN), dtype=np.float32)
    return _AUDIO[key]


def assert_loud(rows, true_peak_streams: int | None = None) -> None:
    """Every block of every call, on every stream, has the compressor and both limiters reducing gain (oracle rows).
    `true_peak_streams`: the sibilant stimulus leaves a few streams' limiter output without inter-sample overs; there the
    true-peak limiter must work on at least that many streams in every block."""
    for field in ("compressor_gain_reduction_db", "limiter_peak_gain_reduction_db", "true_peak_limiter_gain_reduction_db"):
        busy = rows[field] > 0.0
        if field.startswith("true_peak") and true_peak_streams is not None:
            assert (busy.sum(axis=1) >= true_peak_streams).all(), busy.sum(axis=1).tolist()
            continue
        quiet = np.argwhere(~busy)
        assert quiet.size == 0, f"{field} is 0 in (block, stream) {quiet[:6].tolist()}: the stimulus is not loud enough"
