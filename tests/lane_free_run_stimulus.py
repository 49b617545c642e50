"""The lane stimulus of tests/test_gpu_gate_lanes.py in front of the free-running float64 suppressor reference
(`suppressor_stage_ref.free_run`): ten of the first 94 streams of `signals.gate_lane_batch(., 96000, 2)`, 200 frames, the
wrapper protocol at strength 1.0 with the seed-0x5EED weights.

Streams: 29, 68, 82 and 93 are the ones test_gpu_gate_lanes.py names as SUPPRESSOR_EXCEPTIONS; 0 and 63 are the first and
last row of the full 64-stream group, 64 the first of the ragged one (93 is its last); 4 and 17 are driven into the wrapper's
soft clip in about 135 of their frames; 10 is an ordinary row.

Two configurations of what stands in front of the suppressor:
  A   sanitize (clamp off) -> DC block + 80 Hz high-pass
  B   the same, then the noise gate in mode 1 with its default parameters (the oracle's gated signal)

The engine's tap keeps the last suppressor window only, so the device is driven in calls of one window: 12 calls of 16 frames
and one of 8 at control block 480.

`oracle_and_free_run` is the one place where the oracle (af_oracle_py.RnnoiseTap, the f32 restatement) meets the free run: it
is what the CPU test judges, what yields the device's bounds, and what caps the named exceptions of test_gpu_gate_lanes.py.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import signals as S
import suppressor_stage_ref as R

N_STREAMS, N, SEED = 94, 96_000, 2  # one full group and a ragged one of 30
NAMED = (29, 68, 82, 93)
STREAMS = NAMED + (0, 4, 10, 17, 63, 64)
FRAMES = N // R.FRAME
CALLS = (16,) * 12 + (8,)  # frames per call: one suppressor window each at control block 480
assert sum(CALLS) == FRAMES == 200
STRENGTH, WEIGHT_SEED = 1.0, 0x5EED
CONFIGS = ("A", "B")
CALM_LIMIT, NEIGHBOURHOOD = 2e-6, 2  # a cell is ill-conditioned when the oracle is over CALM_LIMIT from the free run in it
#                                      or within +-NEIGHBOURHOOD frames of it on the same stream


@functools.lru_cache(maxsize=None)
def audio() -> np.ndarray:
    x = S.gate_lane_batch(N_STREAMS, N, SEED)
    x.setflags(write=False)
    return x


def gate_parameters() -> dict:
    import gate_oracle as GO

    return dict(GO.DEFAULT_GATE, mode=1)


def suppressor_input(config: str, rows: np.ndarray) -> np.ndarray:
    """What the suppressor is handed for the raw input `rows` [k, n]: float32 [k, n]."""
    import af_oracle_py as O
    import chain_oracle as CO
    import gate_oracle as GO

    assert config in CONFIGS
    if config == "A":
        return np.stack([O.prefilter(CO.sanitize(row, False)) for row in rows])
    return np.stack([GO.run_stream(row, 48_000.0, (row.size,), gate_parameters())[0] for row in rows])


def scale_for_model(signal: np.ndarray) -> np.ndarray:
    """oracle.scale_sample_for_model over an array (the wrapper's x 32768 with its soft clip)."""
    import af_oracle_py as O

    fn = O.lib().afo_scale_sample_for_model
    fn.restype, fn.argtypes = C.c_float, [C.c_float]
    flat = np.ascontiguousarray(signal, dtype=np.float32).reshape(-1)
    return np.array([fn(v) for v in flat.tolist()], dtype=np.float32).reshape(np.shape(signal))


def oracle_and_free_run(signal: np.ndarray, raw: bool = False, eval_order: int = 0) -> dict:
    """The oracle's taps and the free run for `signal` [k, n] (the suppressor's input, whole frames of it): the wrapper
    protocol at strength 1.0, or the raw protocol.  `distance` [frames, k] is max |oracle out - free run out| per cell."""
    import af_oracle_py as O

    signal = np.ascontiguousarray(signal, dtype=np.float32)
    frames = signal.shape[1] // R.FRAME
    signal = signal[:, :frames * R.FRAME]
    blob = O.rnn_synthetic_weights(WEIGHT_SEED)
    strength = None if raw else STRENGTH
    taps = R.cpu_taps([O.RnnoiseTap(blob, strength, eval_order).run(row) for row in signal])
    x = R.raw_model_input(signal) if raw else scale_for_model(signal)
    free = R.free_run(x, taps["pitch_index"], blob, strength=strength, dry=None if raw else signal)
    distance = cell_max(taps["out"].astype(np.float64) - free["out"])
    return {"signal": signal, "model_input": x, "blob": blob, "strength": strength, "taps": taps, "free": free,
            "distance": distance}


def cell_max(difference: np.ndarray) -> np.ndarray:
    """[k, frames x 480] -> [frames, k]: the largest |difference| of every (frame, stream) cell."""
    k = difference.shape[0]
    return np.abs(difference).reshape(k, -1, R.FRAME).max(axis=2).T


def ill_conditioned(distance: np.ndarray) -> np.ndarray:
    """[frames, k] bool: the oracle is over CALM_LIMIT from the free run in the cell or within +-2 frames of it."""
    over = distance > CALM_LIMIT
    ill = over.copy()
    for shift in range(1, NEIGHBOURHOOD + 1):
        ill[shift:] |= over[:-shift]
        ill[:-shift] |= over[shift:]
    return ill


@functools.lru_cache(maxsize=None)
def run(config: str) -> dict:
    """oracle_and_free_run of configuration A or B on the ten streams, `evaluate` of the oracle's taps (the teacher-forced
    yardstick of the device's stages) and the cells' classes.  Computed once per process; callers must not change it."""
    d = oracle_and_free_run(suppressor_input(config, audio()[list(STREAMS)]))
    d["result"] = R.evaluate(d["model_input"], d["taps"], d["taps"]["out"], d["blob"], dry=d["signal"], strength=STRENGTH)
    d["ill"] = ill_conditioned(d["distance"])
    d["streams"] = STREAMS
    return d


@functools.lru_cache(maxsize=None)
def decisions(config: str) -> np.ndarray:
    """[frames, 94, 2] int32: the oracle's (silence flag, pitch index) of every cell of EVERY stream, in the layout of
    Engine.suppressor_trace."""
    from concurrent.futures import ThreadPoolExecutor

    import af_oracle_py as O
    import gate_oracle as GO

    GO.warm_up()  # the restatement's lazily built tables, before any worker thread starts
    signal = suppressor_input(config, audio())
    with ThreadPoolExecutor(max_workers=16) as pool:
        runs = list(pool.map(lambda row: O.suppressor_process_traced(row, STRENGTH, WEIGHT_SEED), signal))
    return np.stack([np.stack([sil, pitch], axis=1) for _, pitch, sil in runs], axis=1).astype(np.int32)


def expected_rows(config: str) -> np.ndarray:
    """[10, 1728 + 96000] float32: the model-input buffer of the ten streams over the whole timeline behind 1728 zeros
    (prepass_ref's recipe: the model's high-pass restated in numpy float32 over the scaled suppressor input)."""
    d = run(config)
    y = R.biquad_hp_f32(d["model_input"], np.zeros((len(STREAMS), 2), dtype=np.float32))
    return np.concatenate([np.zeros((len(STREAMS), R.PBUF), dtype=np.float32), y], axis=1)
