"""Stimulus of the per-stage suppressor tests: 69 streams x 52 frames whose silent, near-silent, loud and quiet streams sit
inside 16-stream network tiles of ordinary voiced streams.

69 streams fill one network workgroup (4 waves x 16 streams) and leave a second one whose only live wave holds 5 streams;
the spectrum and synthesis kernels (4 streams per workgroup) end on a ragged unit.  The six calls (13, 1, 16, 7, 11, 4
frames; each at most 16 frames, hence one suppressor window, which is all the tap keeps) cover a split of 10 + 3 frames per
wave in the spectrum kernels and 4 + 4 + 4 + 1 in the four-frame pitch-search workgroup, a single frame, a full 16-frame
window and state carried over five call boundaries; the silent span of frames 26-35 crosses the boundary at frame 30.

Roles (every other stream is `kat_signal(52, *stream_params(s))` unchanged):
  start  zeros in samples [0, 3 x 480) and in [16 x 480 + 100, 36 x 480 + 333): the stream starts silent with an empty
         cepstral ring, and falls silent again mid-run
  mid    zeros in [16 x 480 + 100, 36 x 480 + 333) only
  near   frames 16-35 replaced by white noise of sigma 3e-6: the band-energy sum settles near 2e-3, under the 0.04 threshold
  loud   x 2.0 (drives the input clamp), quiet: x 0.02
"""
from __future__ import annotations

import functools

import numpy as np

import signals as S

N_STREAMS, N_FRAMES = 69, 52
CALLS = (13, 1, 16, 7, 11, 4)
assert sum(CALLS) == N_FRAMES and max(CALLS) <= 16
ROLES = {3: "start", 37: "start", 66: "start", 5: "mid", 21: "mid", 65: "mid", 9: "near", 52: "near", 11: "loud", 67: "loud",
         13: "quiet", 50: "quiet"}
SILENT_ROLES = ("start", "mid")
TILE_EDGE_STREAMS = (0, 15, 16, 47, 63, 64, 68)  # first / last rows of network tiles and workgroups, the last stream
READ_STREAMS = tuple(sorted(set(TILE_EDGE_STREAMS) | set(ROLES)))
MID_SPAN = (16 * 480 + 100, 36 * 480 + 333)
EXTREME_WEIGHTS = (127, -127, -128, 126)


def stream_signal(s: int, n_frames: int = N_FRAMES) -> np.ndarray:
    x = S.kat_signal(n_frames, *S.stream_params(s))
    role = ROLES.get(s)
    if role == "start":
        x[:3 * 480] = 0.0
    if role in ("start", "mid"):
        x[MID_SPAN[0]:MID_SPAN[1]] = 0.0
    elif role == "near":
        x[16 * 480:36 * 480] = (3e-6 * np.random.default_rng(1000 + s).standard_normal(20 * 480)).astype(np.float32)
    elif role == "loud":
        x = x * np.float32(2.0)
    elif role == "quiet":
        x = x * np.float32(0.02)
    return np.ascontiguousarray(x, dtype=np.float32)


def batch() -> np.ndarray:
    """[69, 52 x 480] float32."""
    return np.stack([stream_signal(s) for s in range(N_STREAMS)])


def extreme_weight_blob(synthetic: bytes, seed: int = 0xB10B) -> bytes:
    """`synthetic` (the synthetic weights of seed 0xB10B) with 2 % of its bytes set from {127, -127, -128, 126}: the values
    the small-amplitude synthetic weights never produce."""
    w = np.frombuffer(synthetic, dtype=np.int8).copy()
    rng = np.random.default_rng(seed)
    where = rng.choice(w.size, size=w.size // 50, replace=False)
    w[where] = rng.choice(np.array(EXTREME_WEIGHTS, dtype=np.int8), size=where.size)
    return w.tobytes()


# the wrapper-protocol run: 20 streams x 12 frames, strength 0.6, two frames of silence first; every third stream is driven
# into the wrapper's soft clip
WRAPPER_STREAMS, WRAPPER_FRAMES, WRAPPER_STRENGTH = 20, 12, 0.6
WRAPPER_READ_STREAMS = (0, 3, 15, 16, 19)


def wrapper_batch() -> np.ndarray:
    x = S.batch_signal(WRAPPER_STREAMS, WRAPPER_FRAMES)
    x[::3] *= np.float32(2.6)
    x[:, :2 * 480] = 0.0
    return x


# ------------------------------------------------------------------------------------------------------------------
# The three runs the CPU and the GPU tests share: what goes in, and the f32 restatement's taps held against the f64 reference
# (its distance from f64 per stage is the yardstick the device is measured with).  Computed once per process.
RUNS = ("synthetic", "extreme", "wrapper")


def weight_blob(kind: str) -> bytes:
    import af_oracle_py as oracle

    return extreme_weight_blob(oracle.rnn_synthetic_weights(0xB10B)) if kind == "extreme" else oracle.rnn_synthetic_weights(0x5EED)


def model_input(kind: str, audio: np.ndarray) -> np.ndarray:
    """What the suppressor's own high-pass sees: the raw protocol's clamp x 32768, or the wrapper's soft clip."""
    import af_oracle_py as oracle
    import suppressor_stage_ref as R

    if kind != "wrapper":
        return R.raw_model_input(audio)
    flat = np.ascontiguousarray(audio, dtype=np.float32).reshape(-1)
    return np.array([oracle.scale_sample_for_model(float(v)) for v in flat], dtype=np.float32).reshape(audio.shape)


@functools.lru_cache(maxsize=None)
def restatement(kind: str, eval_order: int = 0) -> dict:
    """streams read, their audio and model input, the weight blob, the restatement's taps and `evaluate` of them."""
    import af_oracle_py as oracle
    import suppressor_stage_ref as R

    assert kind in RUNS
    wrapper = kind == "wrapper"
    streams = WRAPPER_READ_STREAMS if wrapper else READ_STREAMS
    audio = wrapper_batch()[list(streams)] if wrapper else np.stack([stream_signal(s) for s in streams])
    blob = weight_blob(kind)
    strength = WRAPPER_STRENGTH if wrapper else None
    taps = R.cpu_taps([oracle.RnnoiseTap(blob, strength, eval_order).run(row) for row in audio])
    x = model_input(kind, audio)
    result = R.evaluate(x, taps, taps["out"], blob, dry=audio if wrapper else None, strength=strength)
    return {"streams": streams, "audio": audio, "model_input": x, "blob": blob, "strength": strength, "taps": taps,
            "result": result}
