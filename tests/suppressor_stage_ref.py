"""A float64 reference of every analysis stage of the RNNoise suppressor, one frame at a time, fed by the upstream tap.

The engine (and the CPU restatement, oracle/af_rnnoise.c) expose a per-frame tap: the spectra X and P, the band values Ex,
Ep, Exp, the 42 features (+ 2 pad words on the device), the network's gains before and after the `lastg` floor, the silence
flag and the pitch index.  `evaluate` takes such taps and the audio that went in and came out, and holds every stage against
numpy float64 arithmetic (`np.fft`) computed from the tap of the stage BEFORE it ("teacher forcing"): an error shows in the
stage where it happens, not in everything downstream, and each stage's tolerance can be as tight as f32 rounding allows.

Two things are f32 on purpose.  The input high-pass biquad is restated operation for operation in numpy float32: its poles
sit so close to 1 that an f64 recurrence differs from the f32 one by 9e-4 of the frame peak in bin 0 -- that would be the
filter's own rounding, not an error of the transform under test.  And `gains = max(gains_raw, 0.6f * previous gains)` is
compared bit for bit, so it is evaluated in f32 from the tapped `gains_raw`.

Nothing here reads the implementation under test: the constants below are the published RNNoise ones.
"""
from __future__ import annotations

import numpy as np

FRAME, WINDOW, FREQ, NB, PBUF, CEPS_MEM, NFEAT = 480, 960, 481, 22, 1728, 8, 42
EBAND5MS = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40, 48, 60, 78, 100])
SILENCE_THRESHOLD = 0.04
F32_EPS = float(np.finfo(np.float32).eps)
STAGES = ("X", "P", "Ex", "Ep", "Exp", "feat", "gains_raw", "out")
# the int8 blob: the fifteen arrays of the public RNNoise model in declaration order (dense [in][out]; GRU [in][3 units], z|r|h)
WEIGHT_ARRAYS = (("input_dense_w", 42 * 24), ("input_dense_b", 24), ("vad_gru_w", 24 * 72), ("vad_gru_u", 24 * 72),
                 ("vad_gru_b", 72), ("vad_out_w", 24), ("vad_out_b", 1), ("noise_gru_w", 90 * 144), ("noise_gru_u", 48 * 144),
                 ("noise_gru_b", 144), ("denoise_gru_w", 114 * 288), ("denoise_gru_u", 96 * 288), ("denoise_gru_b", 288),
                 ("denoise_out_w", 96 * 22), ("denoise_out_b", 22))
WEIGHT_BYTES = sum(n for _, n in WEIGHT_ARRAYS)


def _window() -> np.ndarray:
    i = np.arange(FRAME, dtype=np.float64)
    s = np.sin(0.5 * np.pi * (i + 0.5) / FRAME)
    half = np.sin(0.5 * np.pi * s * s)
    return np.concatenate([half, half[::-1]])


def _band_matrices() -> tuple[np.ndarray, np.ndarray]:
    """(W [22, 481]: triangular band sums with the first and last band doubled; I [481, 22]: interp_band_gain, zero from
    bin 400 on)."""
    tri = np.zeros((NB, FREQ))
    for b in range(NB - 1):
        size = int(EBAND5MS[b + 1] - EBAND5MS[b]) << 2
        j = np.arange(size)
        idx = (int(EBAND5MS[b]) << 2) + j
        tri[b, idx] += 1.0 - j / size
        tri[b + 1, idx] += j / size
    w = tri.copy()
    w[0] *= 2.0
    w[NB - 1] *= 2.0
    return w, tri.T.copy()


def _dct_matrix() -> np.ndarray:
    """out = in @ D: D[j, i] = cos((j + 1/2) i pi / 22) sqrt(2 / 22), column 0 times sqrt(1/2)."""
    j = np.arange(NB, dtype=np.float64)[:, None]
    i = np.arange(NB, dtype=np.float64)[None, :]
    d = np.cos((j + 0.5) * i * np.pi / NB)
    d[:, 0] *= np.sqrt(0.5)
    return d * np.sqrt(2.0 / NB)


WIN = _window()
BAND_W, BAND_INTERP = _band_matrices()
DCT = _dct_matrix()
TANSIG_TABLE = np.tanh(0.04 * np.arange(201)).astype(np.float32).astype(np.float64)  # 201 f32 entries


# ------------------------------------------------------------------------------------------------ model input
def biquad_hp_f32(x: np.ndarray, mem: np.ndarray) -> np.ndarray:
    """RNNoise's input high-pass over [streams, n] float32, in float32, operation for operation as the scalar code
    (y = x + m0; m0 = m1 + (b0 x - a0 y); m1 = b1 x - a1 y).  `mem` [streams, 2] float32 is updated in place."""
    b0, b1, a0, a1 = np.float32(-2.0), np.float32(1.0), np.float32(-1.99599), np.float32(0.99600)
    xt = np.ascontiguousarray(x.T, dtype=np.float32)
    yt = np.empty_like(xt)
    m0, m1 = mem[:, 0].copy(), mem[:, 1].copy()
    for i in range(xt.shape[0]):
        xi = xt[i]
        yi = xi + m0
        m0 = m1 + (b0 * xi - a0 * yi)
        m1 = b1 * xi - a1 * yi
        yt[i] = yi
    mem[:, 0], mem[:, 1] = m0, m1
    assert yt.dtype == np.float32
    return np.ascontiguousarray(yt.T)


def raw_model_input(x: np.ndarray) -> np.ndarray:
    """bin/rnnoise_benchmark.rs: clamp(+-1) x 32768 (exact in f32)."""
    return (np.clip(np.asarray(x, dtype=np.float32), -1.0, 1.0) * np.float32(32768.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ network
def tansig_f64(x: np.ndarray) -> np.ndarray:
    """tansig_approx, table form: i = floor(.5 + 25 |x|), second-order step from the table entry."""
    x = np.asarray(x, dtype=np.float64)
    ax = np.minimum(np.abs(x), 8.0)
    i = np.floor(0.5 + 25.0 * ax).astype(np.int64)
    d = ax - 0.04 * i
    y = TANSIG_TABLE[i]
    y = y + d * (1.0 - y * y) * (1.0 - y * d)
    y = np.where(np.abs(x) < 8.0, y, 1.0)
    return np.sign(x) * y


def sigmoid_f64(x: np.ndarray) -> np.ndarray:
    return 0.5 + 0.5 * tansig_f64(0.5 * x)


class NetworkF64:
    """dense 42->24 tanh, GRU 24, GRU 48, GRU 96 (ReLU candidates), dense 96->22 sigmoid, from the int8 blob, weights / 256;
    inputs [dense | vad | feat] and [vad | noise | feat].  States [streams, units] float64; a stream whose frame is silent
    keeps its three states (`hold_silent=False` is the mutant that does not: tests use it to show they can tell)."""

    def __init__(self, blob: bytes, n_streams: int, hold_silent: bool = True):
        if len(blob) != WEIGHT_BYTES:
            raise ValueError(f"weight blob must be {WEIGHT_BYTES} bytes")
        a = np.frombuffer(blob, dtype=np.int8).astype(np.float64)
        self.w, off = {}, 0
        for name, n in WEIGHT_ARRAYS:
            self.w[name] = a[off:off + n]
            off += n
        self.vad = np.zeros((n_streams, 24))
        self.noise = np.zeros((n_streams, 48))
        self.denoise = np.zeros((n_streams, 96))
        self.hold_silent = hold_silent

    def _dense(self, name: str, n_in: int, n_out: int, x: np.ndarray) -> np.ndarray:
        return (self.w[name + "_b"] + x @ self.w[name + "_w"].reshape(n_in, n_out)) / 256.0

    def _gru(self, name: str, m: int, n: int, state: np.ndarray, x: np.ndarray) -> np.ndarray:
        w = self.w[name + "_w"].reshape(m, 3 * n)
        u = self.w[name + "_u"].reshape(n, 3 * n)
        b = self.w[name + "_b"]
        gate = lambda g, rec: (b[g * n:(g + 1) * n] + x @ w[:, g * n:(g + 1) * n] + rec @ u[:, g * n:(g + 1) * n]) / 256.0  # noqa: E731
        z = sigmoid_f64(gate(0, state))
        r = sigmoid_f64(gate(1, state))
        h = np.maximum(gate(2, state * r), 0.0)
        return z * state + (1.0 - z) * h

    def step(self, feat: np.ndarray, silent: np.ndarray) -> np.ndarray:
        """feat [streams, 42] -> gains_raw [streams, 22] (meaningless on a silent stream)."""
        feat = np.asarray(feat, dtype=np.float64)
        dense = tansig_f64(self._dense("input_dense", 42, 24, feat))
        vad = self._gru("vad_gru", 24, 24, self.vad, dense)
        noise = self._gru("noise_gru", 90, 48, self.noise, np.concatenate([dense, vad, feat], axis=1))
        denoise = self._gru("denoise_gru", 114, 96, self.denoise, np.concatenate([vad, noise, feat], axis=1))
        gains = sigmoid_f64(self._dense("denoise_out", 96, 22, denoise))
        keep = (np.asarray(silent, dtype=bool) & self.hold_silent)[:, None]
        self.vad = np.where(keep, self.vad, vad)
        self.noise = np.where(keep, self.noise, noise)
        self.denoise = np.where(keep, self.denoise, denoise)
        return gains


# ------------------------------------------------------------------------------------------------ the stages
def spectrum_f64(segment: np.ndarray) -> np.ndarray:
    """[streams, 960] -> [streams, 481]: rfft(window x segment) / 960."""
    return np.fft.rfft(WIN * segment, axis=-1) / WINDOW


def band_values_f64(X: np.ndarray, P: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(Ex, Ep, Exp) [streams, 22] from spectra [streams, 481]; Exp divided by sqrt(.001 + Ex Ep)."""
    ex = (X.real ** 2 + X.imag ** 2) @ BAND_W.T
    ep = (P.real ** 2 + P.imag ** 2) @ BAND_W.T
    exp = (X.real * P.real + X.imag * P.imag) @ BAND_W.T
    return ex, ep, exp / np.sqrt(0.001 + ex * ep)


class FeaturesF64:
    """compute_frame_features from (Ex, Exp, pitch index), the cepstral ring of 8 and its write index carried per stream."""

    def __init__(self, n_streams: int, advance_on_silence: bool = False):
        self.ring = np.zeros((n_streams, CEPS_MEM, NB))
        self.memid = np.zeros(n_streams, dtype=np.int64)
        self.advance_on_silence = advance_on_silence  # the mutant

    def step(self, ex: np.ndarray, exp: np.ndarray, pitch: np.ndarray, silent: np.ndarray) -> np.ndarray:
        ex, exp = np.asarray(ex, dtype=np.float64), np.asarray(exp, dtype=np.float64)
        n = ex.shape[0]
        rows = np.arange(n)
        ly = np.empty_like(ex)
        log_max = np.full(n, -2.0)
        follow = np.full(n, -2.0)
        for b in range(NB):
            v = np.log10(1e-2 + ex[:, b])
            v = np.maximum(log_max - 7.0, np.maximum(follow - 1.5, v))
            ly[:, b] = v
            log_max = np.maximum(log_max, v)
            follow = np.maximum(follow - 1.5, v)
        ceps = ly @ DCT
        ceps[:, 0] -= 12.0
        ceps[:, 1] -= 4.0
        live = ~np.asarray(silent, dtype=bool)
        write = live | self.advance_on_silence
        m0 = self.memid.copy()
        ring = self.ring.copy()
        ring[rows, m0] = ceps
        self.ring = np.where(write[:, None, None], ring, self.ring)
        self.memid = np.where(write, (m0 + 1) % CEPS_MEM, m0)
        c0 = ring[rows, m0]
        c1 = ring[rows, (m0 - 1) % CEPS_MEM]
        c2 = ring[rows, (m0 - 2) % CEPS_MEM]
        feat = np.zeros((n, NFEAT))
        feat[:, :NB] = ceps
        feat[:, :6] = (c0 + c1 + c2)[:, :6]
        feat[:, 22:28] = (c0 - c2)[:, :6]
        feat[:, 28:34] = (c0 - 2.0 * c1 + c2)[:, :6]
        corr = exp @ DCT[:, :6]
        corr[:, 0] -= 1.3
        corr[:, 1] -= 0.9
        feat[:, 34:40] = corr
        feat[:, 40] = 0.01 * (np.asarray(pitch, dtype=np.float64) - 300.0)
        diff = ring[:, :, None, :] - ring[:, None, :, :]
        dist = np.sum(diff * diff, axis=-1)
        dist[:, np.arange(CEPS_MEM), np.arange(CEPS_MEM)] = 1e15
        feat[:, 41] = np.sum(np.min(dist, axis=-1), axis=-1) / CEPS_MEM - 2.1
        feat[~live] = 0.0
        return feat


def synthesis_f64(X, P, ex, ep, exp, graw, gains, silent, overlap) -> np.ndarray:
    """pitch_filter (branch on Exp > gains_raw), renormalisation, interp_band_gain of `gains`, inverse transform, window and
    overlap-add: [streams, 480] in model units; `overlap` [streams, 480] float64 is updated in place.  A silent frame's X
    goes to the inverse transform as it is."""
    X = np.asarray(X, dtype=np.complex128)
    r = np.where(exp > graw, 1.0, exp * exp * (1.0 - graw * graw) / (0.001 + graw * graw * (1.0 - exp * exp)))
    r = np.sqrt(np.clip(r, 0.0, 1.0)) * np.sqrt(ex / (1e-8 + ep))
    Y = X + (r @ BAND_INTERP.T) * P
    new_e = (Y.real ** 2 + Y.imag ** 2) @ BAND_W.T
    norm = np.sqrt(ex / (1e-8 + new_e))
    Y = Y * (norm @ BAND_INTERP.T) * (gains @ BAND_INTERP.T)
    Y = np.where(np.asarray(silent, dtype=bool)[:, None], X, Y)
    buf = np.fft.irfft(Y, WINDOW, axis=-1) * WINDOW * WIN
    out = buf[:, :FRAME] + overlap
    overlap[:] = buf[:, FRAME:]
    return out


# ------------------------------------------------------------------------------------------------ the checker
def stack_taps(cells: list[list[dict]]) -> dict:
    """cells[frame][stream] (dicts of one cell each, e.g. Engine.suppressor_debug_read) -> arrays [frames, streams, ...]."""
    keys = ("X", "P", "Ex", "Ep", "Exp", "feat", "gains_raw", "gains", "silence", "pitch_index")
    return {k: np.array([[c[k] for c in row] for row in cells]) for k in keys}


def cpu_taps(runs: list[dict]) -> dict:
    """af_oracle_py.RnnoiseTap.run results, one per stream -> the same layout ([frames, streams, ...]; `feat` padded to 44)."""
    out = {}
    for k in ("X", "P", "Ex", "Ep", "Exp", "gains_raw", "gains", "silence", "pitch_index"):
        out[k] = np.stack([r[k] for r in runs], axis=1)
    feat = np.stack([r["features"] for r in runs], axis=1)
    out["feat"] = np.concatenate([feat, np.zeros(feat.shape[:2] + (2,), dtype=feat.dtype)], axis=2)
    out["out"] = np.stack([r["out"].reshape(-1) for r in runs], axis=0)
    return out


def evaluate(model_input: np.ndarray, taps: dict, audio_out: np.ndarray, blob: bytes, dry: np.ndarray | None = None,
             strength: float | None = None, hold_silent: bool = True, advance_on_silence: bool = False) -> dict:
    """Hold `taps` ([frames, streams, ...]) against the float64 reference, stage by stage.

    `model_input` [streams, frames x 480] float32: what the suppressor's own high-pass sees (raw_model_input of the audio, or
    the wrapper's soft clip of it).  `audio_out` [streams, frames x 480]: the output in +-1 full scale.  `strength` / `dry`:
    the wrapper's smoothed wet/dry mix (`smoothed = strength c + smoothed (1 - c)` in f32, mixed when smoothed < 1).
    `hold_silent=False` / `advance_on_silence=True` turn the REFERENCE into a mutant (NetworkF64, FeaturesF64).

    Returns per stage an array [frames, streams] of errors (NaN where the stage does not exist: the network's gains on a
    silent frame), the scales the absolute metrics live on, and the exact checks' failures as lists of (frame, stream):
      X, P          max |d| over the 481 bins / the frame's max |ref|  (P: the transform at the TAPPED pitch index)
      Ex, Ep        max over bands of |d| / max(|ref|, 1e-6 x the frame's largest band value), from the tapped X and P
      Exp           max |d|, from the tapped X and P
      feat          max |d| over the 42 features, from the tapped Ex, Exp, pitch index and silence flag
      gains_raw     max |d|, the f64 network fed the tapped features frame by frame
      out           max |d| in full-scale units, the f64 synthesis of the tapped X, P and record
      silence_wrong the flag differs from sum(Ex_ref) < 0.04 (frames within a relative 1e-4 of 0.04: `near_threshold`)
      pad_nonzero   feat[42:44] != 0;  silent_feat_nonzero: a silent frame's features != 0
      gains_floor_wrong  gains != max(gains_raw, 0.6f x previous gains) bit for bit (held across silent frames)
    """
    n_frames, n_streams = taps["silence"].shape
    x = biquad_hp_f32(model_input[:, :n_frames * FRAME], np.zeros((n_streams, 2), dtype=np.float32)).astype(np.float64)
    hist = np.zeros((n_streams, PBUF))
    features = FeaturesF64(n_streams, advance_on_silence)
    net = NetworkF64(blob, n_streams, hold_silent)
    lastg = np.zeros((n_streams, NB), dtype=np.float32)
    overlap = np.zeros((n_streams, FRAME))
    smoothed = np.ones(n_streams, dtype=np.float32)
    coeff = np.float32(1.0) - np.exp(-((np.float32(480.0) / np.float32(48000.0)) / (np.float32(15.0) / np.float32(1000.0))))
    assert coeff.dtype == np.float32
    err = {k: np.full((n_frames, n_streams), np.nan) for k in STAGES}
    fails = {k: [] for k in ("silence_wrong", "near_threshold", "pad_nonzero", "silent_feat_nonzero", "gains_floor_wrong")}
    feat_scale = 0.0
    rows = np.arange(n_streams)
    for f in range(n_frames):
        t = {k: v[f] for k, v in taps.items() if k != "out"}
        silent = t["silence"] != 0
        live = ~silent
        hist = np.concatenate([hist[:, FRAME:], x[:, f * FRAME:(f + 1) * FRAME]], axis=1)

        def spectrum_error(got, ref):
            peak = np.max(np.abs(ref), axis=1)
            d = np.max(np.abs(got.astype(np.complex128) - ref), axis=1)
            return np.where(peak > 0.0, d / np.where(peak > 0.0, peak, 1.0), np.where(d == 0.0, 0.0, np.inf))

        err["X"][f] = spectrum_error(t["X"], spectrum_f64(hist[:, PBUF - WINDOW:]))
        start = PBUF - WINDOW - t["pitch_index"].astype(np.int64)
        assert np.all((start >= 0) & (start <= PBUF - WINDOW)), "pitch index outside [0, 768]"
        seg = hist[rows[:, None], start[:, None] + np.arange(WINDOW)[None, :]]
        err["P"][f] = spectrum_error(t["P"], spectrum_f64(seg))

        Xd, Pd = t["X"].astype(np.complex128), t["P"].astype(np.complex128)
        ex_ref, ep_ref, exp_ref = band_values_f64(Xd, Pd)
        for key, ref in (("Ex", ex_ref), ("Ep", ep_ref)):
            floor = 1e-6 * np.max(np.abs(ref), axis=1, keepdims=True)
            den = np.maximum(np.abs(ref), floor)
            d = np.abs(t[key].astype(np.float64) - ref)
            err[key][f] = np.max(np.where(den > 0.0, d / np.where(den > 0.0, den, 1.0), np.where(d == 0.0, 0.0, np.inf)), axis=1)
        err["Exp"][f] = np.max(np.abs(t["Exp"].astype(np.float64) - exp_ref), axis=1)

        total = np.sum(ex_ref, axis=1)
        near = np.abs(total - SILENCE_THRESHOLD) <= 1e-4 * SILENCE_THRESHOLD
        wrong = ((total < SILENCE_THRESHOLD) != silent) & ~near
        fails["near_threshold"] += [(f, int(s)) for s in np.flatnonzero(near)]
        fails["silence_wrong"] += [(f, int(s)) for s in np.flatnonzero(wrong)]

        feat_ref = features.step(t["Ex"], t["Exp"], t["pitch_index"], silent)
        feat_scale = max(feat_scale, float(np.max(np.abs(feat_ref))))
        err["feat"][f] = np.max(np.abs(t["feat"][:, :NFEAT].astype(np.float64) - feat_ref), axis=1)
        fails["pad_nonzero"] += [(f, int(s)) for s in np.flatnonzero(np.any(t["feat"][:, NFEAT:].view(np.uint32) != 0, axis=1))]
        fails["silent_feat_nonzero"] += [(f, int(s)) for s in np.flatnonzero(silent & np.any(t["feat"][:, :NFEAT] != 0, axis=1))]

        graw_ref = net.step(t["feat"][:, :NFEAT], silent)
        err["gains_raw"][f] = np.where(live, np.max(np.abs(t["gains_raw"].astype(np.float64) - graw_ref), axis=1), np.nan)
        floor_g = np.maximum(t["gains_raw"].astype(np.float32), np.float32(0.6) * lastg)
        assert floor_g.dtype == np.float32
        bad = live & np.any(floor_g.view(np.uint32) != t["gains"].astype(np.float32).view(np.uint32), axis=1)
        fails["gains_floor_wrong"] += [(f, int(s)) for s in np.flatnonzero(bad)]
        lastg = np.where(live[:, None], t["gains"].astype(np.float32), lastg)

        wet = synthesis_f64(Xd, Pd, t["Ex"].astype(np.float64), t["Ep"].astype(np.float64), t["Exp"].astype(np.float64),
                            np.where(live[:, None], t["gains_raw"], 0).astype(np.float64),
                            np.where(live[:, None], t["gains"], 0).astype(np.float64), silent, overlap) / 32768.0
        if strength is not None:
            smoothed = np.float32(strength) * coeff + smoothed * (np.float32(1.0) - coeff)
            assert smoothed.dtype == np.float32
            mix = smoothed < np.float32(1.0)
            d = dry[:, f * FRAME:(f + 1) * FRAME].astype(np.float64)
            mixed = smoothed.astype(np.float64)[:, None] * wet + (np.float32(1.0) - smoothed).astype(np.float64)[:, None] * d
            wet = np.where(mix[:, None], mixed, wet)
        err["out"][f] = np.max(np.abs(audio_out[:, f * FRAME:(f + 1) * FRAME].astype(np.float64) - wet), axis=1)
    return {"err": err, "fails": fails, "scale": {k: (max(feat_scale, 1.0) if k == "feat" else 1.0) for k in STAGES}}


def worst(errors: np.ndarray) -> tuple[float, int, int]:
    """(largest error, frame, stream index) of an [frames, streams] array, NaN cells (stage absent) left out."""
    if np.all(np.isnan(errors)):
        return 0.0, -1, -1
    f, s = np.unravel_index(int(np.nanargmax(errors)), errors.shape)
    return float(errors[f, s]), int(f), int(s)


def first_frames_after_silence(silence: np.ndarray) -> list[tuple[int, int]]:
    """(frame, stream index) of every live frame that follows a silent one; `silence` [frames, streams]."""
    sil = np.asarray(silence) != 0
    return [(int(f) + 1, int(s)) for f, s in zip(*np.nonzero(sil[:-1] & ~sil[1:]))]


def bound(stage: str, restatement: dict) -> float:
    """The device's tolerance for `stage`: 4 x the f32 restatement's own worst distance from the same f64 reference on the
    same stimulus and metric (a different f32 factorisation of the same 960-point transform and a different summation order
    differ by a small constant, not by an order of magnitude), and not under 4 f32 epsilons of the metric's scale."""
    return max(4.0 * worst(restatement["err"][stage])[0], 4.0 * F32_EPS * restatement["scale"][stage])


# ------------------------------------------------------------------------------------------------ the free run
def mix_coefficient() -> np.float32:
    """The wrapper's wet/dry smoothing coefficient, 1 - exp(-(480 / 48000) / (15 / 1000)), every operation in f32."""
    coeff = np.float32(1.0) - np.exp(-((np.float32(480.0) / np.float32(48000.0)) / (np.float32(15.0) / np.float32(1000.0))))
    assert coeff.dtype == np.float32
    return coeff


def free_run(model_input: np.ndarray, pitch_index: np.ndarray, blob: bytes, strength: float | None = None,
             dry: np.ndarray | None = None) -> dict:
    """The stage functions above chained WITHOUT teacher forcing: every stage is fed the float64 result of the stage before
    it, from the f32-restated high-pass (biquad_hp_f32) to the overlap-add, with the cepstral ring, the three GRU states, the
    `lastg` floor and the overlap carried in f64 over the whole run.  What an exact evaluation of the algorithm gives on this
    model input -- not what any f32 implementation gives: where the algorithm is ill-conditioned, two correct f32
    evaluations leave this and each other by more than their rounding.

    `model_input` [streams, frames x 480] float32 as for `evaluate`.  `pitch_index` [frames, streams]: the only decision
    taken from outside (the pitch path has its own reference, tests/pitch_stage_ref.py).  The silence flag is
    sum(Ex) < 0.04 of the run's own Ex; `gains = max(gains_raw, 0.6 x previous gains)`, held across silent frames.
    `strength` / `dry` [streams, frames x 480]: the wrapper's smoothed wet/dry mix as `evaluate` restates it (the smoothed
    strength in f32, as the wrapper keeps it).

    Returns `out` [streams, frames x 480] float64 in +-1 full scale, and per frame `feat` [frames, streams, 42], `gains_raw`
    [frames, streams, 22] (zeros on a silent frame, like the taps), `silence` [frames, streams] bool and `Ex_sum`
    [frames, streams] (the flag's operand); for reports also `gains`, `Ex`, `Ep`, `Exp` [frames, streams, 22]."""
    pitch_index = np.asarray(pitch_index, dtype=np.int64)
    n_frames, n_streams = pitch_index.shape
    assert model_input.shape[0] == n_streams and model_input.shape[1] >= n_frames * FRAME
    x = biquad_hp_f32(model_input[:, :n_frames * FRAME], np.zeros((n_streams, 2), dtype=np.float32)).astype(np.float64)
    hist = np.zeros((n_streams, PBUF))
    features = FeaturesF64(n_streams)
    net = NetworkF64(blob, n_streams)
    lastg = np.zeros((n_streams, NB))
    overlap = np.zeros((n_streams, FRAME))
    smoothed = np.ones(n_streams, dtype=np.float32)
    coeff = mix_coefficient()
    rows = np.arange(n_streams)
    res = {"out": np.zeros((n_streams, n_frames * FRAME)), "feat": np.zeros((n_frames, n_streams, NFEAT)),
           "gains_raw": np.zeros((n_frames, n_streams, NB)), "silence": np.zeros((n_frames, n_streams), dtype=bool),
           "Ex_sum": np.zeros((n_frames, n_streams)), "gains": np.zeros((n_frames, n_streams, NB)),
           "Ex": np.zeros((n_frames, n_streams, NB)), "Ep": np.zeros((n_frames, n_streams, NB)),
           "Exp": np.zeros((n_frames, n_streams, NB))}
    for f in range(n_frames):
        hist = np.concatenate([hist[:, FRAME:], x[:, f * FRAME:(f + 1) * FRAME]], axis=1)
        X = spectrum_f64(hist[:, PBUF - WINDOW:])
        start = PBUF - WINDOW - pitch_index[f]
        assert np.all((start >= 0) & (start <= PBUF - WINDOW)), "pitch index outside [0, 768]"
        P = spectrum_f64(hist[rows[:, None], start[:, None] + np.arange(WINDOW)[None, :]])
        ex, ep, exp = band_values_f64(X, P)
        total = np.sum(ex, axis=1)
        silent = total < SILENCE_THRESHOLD
        live = ~silent
        feat = features.step(ex, exp, pitch_index[f], silent)
        graw = np.where(live[:, None], net.step(feat, silent), 0.0)
        gains = np.where(live[:, None], np.maximum(graw, 0.6 * lastg), 0.0)
        lastg = np.where(live[:, None], gains, lastg)
        wet = synthesis_f64(X, P, ex, ep, exp, graw, gains, silent, overlap) / 32768.0
        if strength is not None:
            smoothed = np.float32(strength) * coeff + smoothed * (np.float32(1.0) - coeff)
            assert smoothed.dtype == np.float32
            mix = smoothed < np.float32(1.0)
            d = dry[:, f * FRAME:(f + 1) * FRAME].astype(np.float64)
            mixed = smoothed.astype(np.float64)[:, None] * wet + (np.float32(1.0) - smoothed).astype(np.float64)[:, None] * d
            wet = np.where(mix[:, None], mixed, wet)
        res["out"][:, f * FRAME:(f + 1) * FRAME] = wet
        res["feat"][f], res["gains_raw"][f], res["silence"][f], res["Ex_sum"][f] = feat, graw, silent, total
        res["gains"][f], res["Ex"][f], res["Ep"][f], res["Exp"][f] = gains, ex, ep, exp
    return res
