"""Stimulus of the pitch-path tests: the 69-stream layout of suppressor_stage_stimulus (16-stream network tiles of ordinary
voiced streams) with pitch-specific streams set into it, 43 frames in twelve calls, and the synthetic spans of the stand-alone
search.  Deterministic, no GPU.

Calls are whole frames, one suppressor window each (the tap keeps the last window): 1, 1, 1, 2, 3, 4, 5, 1, 7, 16, 1, 1.  The
one-frame calls show `last_gain` after single frames; 2, 3, 5 and 7 leave 2, 3, 1 and 3 live waves in the last four-frame
workgroup of the search, 1 leaves one.

Roles (every other stream is `kat_signal(43, *stream_params(s))` unchanged).  A `voice` is a sum of harmonics of a period
given per sample (phase = cumulative sum of 1 / period), optionally with a component at half the fundamental, which makes
the search lock onto the doubled period so that remove_doubling has something to remove:
  sweep_up    f0 50 -> 1000 Hz: f0 <= 62.5 Hz makes the search return 768 (T0 clamped to 383); high f0 puts the sub-multiples
              under the minimum period (the `T1 < minperiod` break) and the final index under 60 (clamped)
  sweep_down  f0 1000 -> 50 Hz
  steps       the period changes frame by frame: halves, doubles, moves by +-2 and +-4 samples (+-1 and +-2 lags of the
              2x-decimated tracker): all three arms of `cont`
  drift       period 346 drifting by 4 samples a frame, with the half-fundamental component
  sub<k>      k = 3 .. 12: a strong component of period 2 T1 samples and a weak one of period 2 k T1.  The search finds
              k T1, and the k-th candidate of remove_doubling (T1 = T0 / k, T1b = second_check[k] T1) is the last one taken,
              on every frame: its correlation .5 (xy(T1) + xy(T1b)) becomes the pitch gain, so `second_check[k]` shows in
              last_gain at every call end.  (A purely periodic voice cannot tell the entries apart: every multiple of its
              period correlates alike.  k = 13 .. 15 never run: T0 <= 383 puts their T1 under the minimum period.)
  zeros       exact zeros (ac[0] == 0)
  drain       a loud voice, exact zeros from frame 28 on: the 1728-sample history drains over the next four frames, and
              the tail of the model-input high-pass decays by e^-0.96 a frame after it.  (Not earlier: twenty frames into
              that tail `num = (xcorr x 1e-12)^2` of find_best_pitch leaves the normal range of f32, where the published f32
              algorithm has no relative precision left and a float64 reference says nothing about it.)
  late        starts after two silent frames
No broadband-noise stream is read: a flat correlation would only fill the excused share.
"""
from __future__ import annotations

import functools

import numpy as np

import signals as S

N_STREAMS, N_FRAMES, FRAME, PBUF = 69, 43, 480, 1728
CALLS = (1, 1, 1, 2, 3, 4, 5, 1, 7, 16, 1, 1)
assert sum(CALLS) == N_FRAMES and max(CALLS) <= 16
assert {n % 4 for n in CALLS} >= {1, 2, 3}  # ragged four-frame groups with 1, 2 and 3 live waves
ROLES = {2: "sweep_up", 18: "sweep_down", 34: "steps", 50: "drift", 6: "zeros", 66: "zeros", 22: "drain", 38: "late",
         54: "sweep_up", 65: "steps", 3: "sub3", 4: "sub4", 5: "sub5", 19: "sub6", 20: "sub7", 21: "sub8", 35: "sub9", 36: "sub10",
         37: "sub11", 51: "sub12"}
# sub<k>: T1, the strong component's period in lags of the 2x-decimated buffer (2 T1 samples); the weak one's is k T1
# (k T1 > 192: two of the weak component's periods do not fit the search's range, where they would tie with one)
SUB_T1 = {3: 65, 4: 49, 5: 40, 6: 32, 7: 32, 8: 32, 9: 32, 10: 32, 11: 32, 12: 31}
SUB_WEAK_POWER = 0.15
NEIGHBOURS = (0, 1, 15, 16, 17, 33, 47, 49, 63, 64, 68)  # ordinary streams beside them, at the edges of every tile
READ_STREAMS = tuple(sorted(set(ROLES) | set(NEIGHBOURS)))
DRAIN_FRAME = 28  # inside the 16-frame call (frames 25-40), across its first two four-frame groups
STEP_PERIODS = (400, 400, 400, 200, 200, 400, 400, 402, 402, 404, 400, 396, 396, 198, 198, 396, 392, 392, 196, 392, 394, 396,
                398, 402, 406, 410, 205, 205, 410, 408, 406, 404, 402, 400, 200, 100, 100, 200, 400, 404, 404, 400, 400)
assert len(STEP_PERIODS) == N_FRAMES


def voice(period: np.ndarray, harmonics=(1.0, 0.6, 0.35, 0.2), half: float = 0.0, level: float = 0.25) -> np.ndarray:
    """Sum of harmonics of a per-sample period (in samples), `half` x a component at half the fundamental."""
    phase = np.cumsum(1.0 / np.asarray(period, dtype=np.float64))
    x = sum(a * np.sin(2.0 * np.pi * (h + 1) * phase + 0.7 * h) for h, a in enumerate(harmonics))
    x = x + half * np.sin(np.pi * phase + 0.3)
    return (level * x / (sum(harmonics) + half)).astype(np.float32)


def stream_signal(s: int) -> np.ndarray:
    n = N_FRAMES * FRAME
    role = ROLES.get(s)
    t = np.arange(n) / (n - 1.0)
    if role == "sweep_up":
        x = voice(48000.0 / (50.0 * 20.0 ** t), half=0.0 if s == 2 else 0.4)
    elif role == "sweep_down":
        x = voice(48000.0 / (1000.0 * 20.0 ** -t))
    elif role == "steps":
        x = voice(np.repeat(np.array(STEP_PERIODS if s == 34 else STEP_PERIODS[::-1], dtype=np.float64), FRAME), half=0.5)
    elif role == "drift":
        x = voice(346.0 + 4.0 * np.arange(n) / FRAME * np.sign(np.sin(2.0 * np.pi * 3.0 * t)), half=0.6)
    elif role is not None and role.startswith("sub"):
        k = int(role[3:])
        i, t1 = np.arange(n), SUB_T1[k]
        x = (0.2 * (np.sin(2.0 * np.pi * i / (2 * t1)) + 0.5 * np.sin(4.0 * np.pi * i / (2 * t1) + 0.6)
                    + np.sqrt(SUB_WEAK_POWER) * np.sin(2.0 * np.pi * i / (2 * k * t1) + 0.9))).astype(np.float32)
    elif role == "zeros":
        x = np.zeros(n, dtype=np.float32)
    elif role == "drain":
        x = voice(np.full(n, 267.0), level=0.9)
        x[DRAIN_FRAME * FRAME:] = 0.0
    else:
        x = S.kat_signal(N_FRAMES, *S.stream_params(s))
        if role == "late":
            x[:2 * FRAME] = 0.0
    return np.ascontiguousarray(x, dtype=np.float32)


def batch() -> np.ndarray:
    """[69, 43 x 480] float32."""
    return np.stack([stream_signal(s) for s in range(N_STREAMS)])


@functools.lru_cache(maxsize=None)
def read_audio() -> np.ndarray:
    """The streams that are read, [len(READ_STREAMS), 43 x 480]."""
    a = np.stack([stream_signal(s) for s in READ_STREAMS])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def model_spans() -> np.ndarray:
    """[len(READ_STREAMS), 1728 + 43 x 480] float32: zero history, then the f32-restated model input (clamp x 32768, the
    input high-pass) of the read streams -- frame f's pitch buffer is span[480 (f + 1) : 480 (f + 1) + 1728]."""
    import suppressor_stage_ref as R

    audio = read_audio()
    x = R.biquad_hp_f32(R.raw_model_input(audio), np.zeros((audio.shape[0], 2), dtype=np.float32))
    spans = np.concatenate([np.zeros((audio.shape[0], PBUF), dtype=np.float32), x], axis=1)
    spans.setflags(write=False)
    return spans


def pitch_buffer(spans: np.ndarray, stream: int, frame: int) -> np.ndarray:
    return spans[stream, FRAME * (frame + 1):FRAME * (frame + 1) + PBUF]


# ------------------------------------------------------------------------------------------------ the search alone
SEARCH_FRAMES = (1, 3, 4, 6)  # 1, 3, 4 and 4 + 2 live waves
SEARCH_STREAMS = ("zeros", "impulse", "lag0", "lag146", "twin")


def _evolving(n: int, period: int, rho: float, n_harmonics: int, seed: int = 7) -> np.ndarray:
    """A waveform of exactly `period` samples whose harmonic amplitudes follow an AR(1) process from one period to the next
    (correlation `rho`): stationary, and among the shifts by whole periods the smallest correlates best -- a plain tone ties
    them all, and its normalised correlation then follows the phase of its own energy window."""
    rng = np.random.default_rng(seed)
    k, phase = np.arange(n) // period, 2.0 * np.pi * (np.arange(n) % period) / period
    c = np.empty((int(k.max()) + 1, 2 * n_harmonics))
    c[0] = rng.standard_normal(2 * n_harmonics)
    for j in range(1, c.shape[0]):
        c[j] = rho * c[j - 1] + np.sqrt(1.0 - rho * rho) * rng.standard_normal(2 * n_harmonics)
    x = np.zeros(n)
    for h in range(n_harmonics):
        x += (c[k, 2 * h] * np.cos((h + 1) * phase) + c[k, 2 * h + 1] * np.sin((h + 1) * phase)) / (h + 1)
    return 4000.0 * x


def search_spans(n_frames: int) -> np.ndarray:
    """[5, 1728 + 480 n_frames] float32 model-input spans (+-32768 units): exact zeros; one unit impulse; a waveform of
    period 768 (the coarse and the fine maximum at lag 0: no interpolation offset); one of period 182 (coarse lag 146, fine
    lag 293, the last one); one of period 402, between the coarse lags 91 (404) and 92 (400): two coarse maxima one lag
    apart, whose fine neighbourhoods overlap.  (tests/test_pitch_stage_ref.py asserts on the f64 search that they do.)"""
    n = PBUF + FRAME * n_frames
    x = np.zeros((len(SEARCH_STREAMS), n))
    x[1, FRAME + PBUF - 200] = 1.0  # sample 1528 of frame 0's buffer, 1048, 568, 88 of the next three; gone after that
    x[2] = _evolving(n, 768, 0.8, 5)
    x[3] = _evolving(n, 182, 0.9, 8)
    x[4] = _evolving(n, 402, 0.95, 3)
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------
# What the CPU and the GPU tests share: the restatement's taps on the same cells, held against the f64 reference.  Its
# distance from f64 is the yardstick the device is measured with.  Computed once per process and evaluation order.
def span_cells(spans: np.ndarray, n_frames: int, eval_order: int) -> dict:
    """The restatement's search alone on every (frame, stream) cell of `spans`: ds [frames, streams, 864], index, ops."""
    import af_oracle_py as oracle

    cells = [[oracle.rnn_pitch_search(pitch_buffer(spans, s, f), eval_order) for s in range(spans.shape[0])] for f in range(n_frames)]
    return {"ds": np.array([[c["pitch_ds"] for c in row] for row in cells]),
            "index": np.array([[c["search_index"] for c in row] for row in cells], dtype=np.int64),
            "ops": np.array([[c["pitch_ops"] for c in row] for row in cells])}


@functools.lru_cache(maxsize=None)
def restatement(eval_order: int = 0) -> dict:
    """engine: the restatement's per-frame taps of the read streams over the 43 frames ([frames, streams, ...]), its
    tracker state at the twelve call ends, buffer errors and the tracker check; search: its search alone on the synthetic
    spans (per frame count) and on the read streams' model-input spans, with the search check; tau, buffer_bound, gain_bound:
    what the device is held to (pitch_stage_ref.tau_bound / magnitude_bound of this evaluation order's own distances)."""
    import af_oracle_py as oracle
    import pitch_stage_ref as P

    runs = [oracle.RnnoiseTap(eval_order=eval_order).run(row) for row in read_audio()]
    eng = {k: np.stack([r[k] for r in runs], axis=1) for k in ("pitch_ds", "pitch_index", "search_index", "pitch_gain", "pitch_ops", "silence")}
    ends = np.cumsum(CALLS) - 1
    eng["end_period"], eng["end_gain"] = eng["pitch_index"][ends], eng["pitch_gain"][ends]
    eng["buffer_err"] = P.check_buffers(eng["pitch_ds"], model_spans())
    search = {"stimulus": {"spans": model_spans(), "ds": eng["pitch_ds"], "index": eng["search_index"], "ops": eng["pitch_ops"][..., :3]}}
    for n in SEARCH_FRAMES:
        spans = search_spans(n)
        search[n] = {"spans": spans, **span_cells(spans, n, eval_order)}
    for part in search.values():
        part["buffer_err"] = P.check_buffers(part["ds"], part["spans"])
    # pass 1, strict: the operand distances of the cells that agree -> tau; pass 2 only where a cell did not agree
    strict = {k: P.check_search(part["ds"], part["index"], 0.0, part["ops"]) for k, part in search.items()}
    tracker = P.check_tracker(eng["pitch_ds"], eng["pitch_index"], CALLS, eng["end_period"], eng["end_gain"], 0.0, eng["pitch_ops"])
    distance = max([tracker["operand_distance"]] + [c["operand_distance"] for c in strict.values()])
    tau = P.tau_bound(distance)
    for k, part in search.items():
        part["check"] = strict[k] if not strict[k]["status"].any() else P.check_search(part["ds"], part["index"], tau)
    if tracker["status"].any():
        tracker = P.check_tracker(eng["pitch_ds"], eng["pitch_index"], CALLS, eng["end_period"], eng["end_gain"], tau)
    eng["check"] = tracker
    buffer_worst = max(float(np.max(part["buffer_err"])) for part in search.values())
    return {"engine": eng, "search": search, "operand_distance": distance, "tau": tau, "buffer_worst": buffer_worst,
            "buffer_bound": P.magnitude_bound(buffer_worst), "gain_worst": float(np.max(tracker["gain_error"])),
            "gain_bound": P.magnitude_bound(float(np.max(tracker["gain_error"])))}
