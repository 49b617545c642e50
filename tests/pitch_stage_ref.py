"""A float64 reference of the suppressor's pitch path -- pitch_downsample, pitch_search, remove_doubling -- one stage at a
time, each from a given stage input, so that a stage can be computed from the device's own previous stage.

Written from the published algorithm (celt/pitch.c as RNNoise carries it, restated in oracle/af_rnnoise.c): numpy float64
throughout, plain left-to-right sums, no f32 and no wavefront summation order.  `remove_doubling` is reproduced as published,
including the `T1 < 3 minperiod` / `else if T1 < 2 minperiod` pair whose second arm can never run.

Decisions are compared as integers, and an f32 evaluation may legitimately take the other side of a comparison whose two
sides nearly tie.  Every such comparison goes through a `Decider`: strict in the plain mode; in the TOLERANT REPLAY a
comparison whose sides differ by less than tau x max(|lhs|, |rhs|) may go either way, and `replay` searches the tree of those
choices for a path that ends in the result the implementation under test gave.  A cell that needs the replay is `excused`; a
cell the replay cannot reach is a failure.  So that max(|lhs|, |rhs|) is the scale of the sums the comparison is made of and
not of a cancelled difference, two comparisons are written in an algebraically equal form:
  (c - a) > .7 (b - a)   as   c > .7 b + .3 a        (both interpolation-offset rules)
  xcorr > 0              against the scale sqrt(sum x^2 sum y^2) that bounds the sum's rounding error
The clamps (T0 >= maxperiod, index < minperiod, T1 < minperiod) compare integers and need no tolerance.
"""
from __future__ import annotations

import numpy as np

PMIN, PMAX, PFRAME, PBUF, FRAME = 60, 768, 960, 1728, 480
HALF = PBUF // 2                 # 864: the whitened buffer
MAX_PITCH = PMAX - 3 * PMIN      # 588
SECOND_CHECK = (0, 0, 3, 2, 3, 2, 5, 2, 3, 2, 3, 2, 5, 2, 3, 2)
F32_EPS = float(np.finfo(np.float32).eps)


# ------------------------------------------------------------------------------------------------ decisions
class Decider:
    """`gt(lhs, rhs)` = lhs > rhs.  With tau > 0 a near-tie is ambiguous: it takes the next entry of `script`, or the strict
    outcome once the script has run out, and is recorded in `taken`."""

    def __init__(self, tau: float = 0.0, script: tuple = ()):
        self.tau, self.script, self.taken = float(tau), tuple(script), []

    def gt(self, lhs: float, rhs: float, scale: float | None = None) -> bool:
        strict = bool(lhs > rhs)
        if self.tau <= 0.0 or lhs == rhs == 0.0:
            return strict
        s = max(abs(lhs), abs(rhs)) if scale is None else max(scale, abs(lhs), abs(rhs))
        if abs(lhs - rhs) < self.tau * s:
            i = len(self.taken)
            choice = self.script[i] if i < len(self.script) else strict
            self.taken.append(bool(choice))
            return bool(choice)
        return strict


def replay(fn, target, tau: float, key=lambda r: r, limit: int = 4096):
    """(status, result): 'equal' when the strict evaluation of fn(decider) gives `target` (compared through `key`), 'excused'
    when some path of the tolerant replay does (its result is returned), else 'fail' with the strict result."""
    strict = fn(Decider())
    if key(strict) == target:
        return "equal", strict
    stack, tried = [()], 0
    while stack and tried < limit:
        script = stack.pop()
        d = Decider(tau, script)
        r = fn(d)
        tried += 1
        if key(r) == target:
            return "excused", r
        for i in range(len(script), len(d.taken)):
            stack.append(tuple(d.taken[:i]) + (not d.taken[i],))
    return "fail", strict


# ------------------------------------------------------------------------------------------------ pitch_downsample
def decimate(x: np.ndarray) -> np.ndarray:
    """[1728] -> [864]: x_lp[i] = .5 (.5 (x[2i-1] + x[2i+1]) + x[2i]); the first sample has no left neighbour."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(HALF)
    i = np.arange(1, HALF)
    out[1:] = 0.5 * (0.5 * (x[2 * i - 1] + x[2 * i + 1]) + x[2 * i])
    out[0] = 0.5 * (0.5 * x[1] + x[0])
    return out


def lpc4(ac: np.ndarray) -> np.ndarray:
    """Levinson-Durbin of order 4 with the early exit at error < .001 ac[0]; zeros when ac[0] == 0."""
    lpc = np.zeros(4)
    error = ac[0]
    if ac[0] != 0:
        for i in range(4):
            rr = 0.0
            for j in range(i):
                rr += lpc[j] * ac[i - j]
            rr += ac[i + 1]
            r = -rr / error
            lpc[i] = r
            for j in range((i + 1) >> 1):
                t1, t2 = lpc[j], lpc[i - 1 - j]
                lpc[j] = t1 + r * t2
                lpc[i - 1 - j] = t2 + r * t1
            error = error - r * r * error
            if error < 0.001 * ac[0]:
                break
    return lpc


def whiten(x_lp: np.ndarray) -> tuple[np.ndarray, dict]:
    """Lag-windowed autocorrelation, LPC-4, 0.9^i bandwidth expansion, the 0.8 zero, five-tap FIR with zero initial memory."""
    x_lp = np.asarray(x_lp, dtype=np.float64)
    ac = np.array([np.dot(x_lp[k:], x_lp[:HALF - k]) for k in range(5)])
    ac0_zero = bool(ac[0] == 0)
    ac[0] *= 1.0001
    for i in range(1, 5):
        ac[i] -= ac[i] * (0.008 * i) * (0.008 * i)
    lpc = lpc4(ac)
    tmp = 1.0
    for i in range(4):
        tmp = 0.9 * tmp
        lpc[i] = lpc[i] * tmp
    c1 = 0.8
    num = np.array([lpc[0] + 0.8, lpc[1] + c1 * lpc[0], lpc[2] + c1 * lpc[1], lpc[3] + c1 * lpc[2], c1 * lpc[3]])
    padded = np.concatenate([np.zeros(5), x_lp])
    out = x_lp.copy()
    for k in range(5):
        out = out + num[k] * padded[4 - k:4 - k + HALF]
    return out, {"ac0_zero": ac0_zero}


def pitch_downsample(x: np.ndarray) -> tuple[np.ndarray, dict]:
    return whiten(decimate(x))


# ------------------------------------------------------------------------------------------------ pitch_search
def _find_best_pitch(xcorr, evaluated, xx, y, length, max_pitch, D: Decider):
    """find_best_pitch; `evaluated`: the lags that hold a correlation (the fine stage computes at most ten; the others are
    exact zeros in any arithmetic and never pass xcorr > 0); `xx` = sum x^2 of the fixed operand (the scale of xcorr > 0)."""
    best_num, best_den, best = [-1.0, -1.0], [0.0, 0.0], [0, 1]
    syy = 1.0 + float(np.dot(y[:length], y[:length]))
    for i in range(max_pitch):
        if evaluated[i]:
            if D.gt(float(xcorr[i]), 0.0, scale=float(np.sqrt(xx * max(syy - 1.0, 0.0)))):
                x16 = float(xcorr[i]) * 1e-12
                num = x16 * x16
                if D.gt(num * best_den[1], best_num[1] * syy):
                    if D.gt(num * best_den[0], best_num[0] * syy):
                        best_num[1], best_den[1], best[1] = best_num[0], best_den[0], best[0]
                        best_num[0], best_den[0], best[0] = num, syy, i
                    else:
                        best_num[1], best_den[1], best[1] = num, syy, i
        syy += float(y[i + length] * y[i + length] - y[i] * y[i])
        syy = max(1.0, syy)
    return best


_STRICT_SEARCH: dict = {}  # strict results by buffer contents: the tracker check searches every buffer again


def pitch_search(ds: np.ndarray, D: Decider | None = None) -> tuple[int, dict]:
    """(search index = 768 - pitch_search(ds + 384, ds, 960, 588), info) from the whitened buffer [864]."""
    ds = np.asarray(ds, dtype=np.float64)
    if D is None or D.tau <= 0.0:
        key = ds.tobytes()
        if key not in _STRICT_SEARCH:
            if len(_STRICT_SEARCH) > 8192:
                _STRICT_SEARCH.clear()
            _STRICT_SEARCH[key] = _pitch_search(ds, Decider())
        return _STRICT_SEARCH[key]
    return _pitch_search(ds, D)


def _pitch_search(ds: np.ndarray, D: Decider) -> tuple[int, dict]:
    x_lp, y = ds[PMAX >> 1:], ds
    length, max_pitch = PFRAME, MAX_PITCH
    x4 = x_lp[0:2 * (length >> 2):2]
    y4 = y[0:2 * ((length + max_pitch) >> 2):2]
    n4, mp4 = length >> 2, max_pitch >> 2
    xc4 = np.array([np.dot(x4, y4[i:i + n4]) for i in range(mp4)])
    coarse = _find_best_pitch(xc4, np.ones(mp4, bool), float(np.dot(x4, x4)), y4, n4, mp4, D)
    n2, mp2 = length >> 1, max_pitch >> 1
    xc = np.zeros(mp2)
    done = np.zeros(mp2, bool)
    xh = x_lp[:n2]
    for i in range(mp2):
        if abs(i - 2 * coarse[0]) > 2 and abs(i - 2 * coarse[1]) > 2:
            continue
        xc[i] = max(-1.0, float(np.dot(xh, y[i:i + n2])))
        done[i] = True
    fine = _find_best_pitch(xc, done, float(np.dot(xh, xh)), y, n2, mp2, D)
    offset = 0
    interior = 0 < fine[0] < mp2 - 1
    if interior:
        a, b, c = float(xc[fine[0] - 1]), float(xc[fine[0]]), float(xc[fine[0] + 1])
        if D.gt(c, 0.7 * b + 0.3 * a):      # (c - a) > .7 (b - a)
            offset = 1
        elif D.gt(a, 0.7 * b + 0.3 * c):    # (a - c) > .7 (b - c)
            offset = -1
    else:
        a = b = c = 0.0
    index = PMAX - (2 * fine[0] - offset)
    return index, {"coarse": tuple(coarse), "fine": tuple(fine), "offset": offset, "abc": (a, b, c),
                   "best0_at_edge": not interior, "candidates_overlap": abs(coarse[0] - coarse[1]) <= 2}


# ------------------------------------------------------------------------------------------------ remove_doubling
def _gain(xy, xx, yy):
    return xy / np.sqrt(1.0 + xx * yy)


def remove_doubling(ds: np.ndarray, t0_in: int, prev_period: int, prev_gain: float, D: Decider | None = None,
                    second_check=SECOND_CHECK) -> tuple[int, float, dict]:
    """(final pitch index, pitch gain, info) = remove_doubling(ds, 768, 60, 960, &T0, prev_period, prev_gain).
    `second_check`: the published table; tests pass a changed one to show that the stimulus can tell."""
    D = D or Decider()
    ds = np.asarray(ds, dtype=np.float64)
    minperiod0 = PMIN
    maxperiod, minperiod, N = PMAX // 2, PMIN // 2, PFRAME // 2
    T0 = int(t0_in) // 2
    prev_period = int(prev_period) // 2
    prev_gain = float(prev_gain)
    o = maxperiod                     # x = ds + maxperiod
    x = ds[o:o + N]
    clamped_t0 = T0 >= maxperiod
    if clamped_t0:
        T0 = maxperiod - 1
    T = T0

    def corr(lag: int) -> float:
        return float(np.dot(x, ds[o - lag:o - lag + N]))

    xx, xy = float(np.dot(x, x)), corr(T0)
    yy_lookup = np.empty(maxperiod + 1)
    yy_lookup[0] = xx
    yy = xx
    for i in range(1, maxperiod + 1):
        yy = yy + ds[o - i] * ds[o - i] - ds[o + N - i] * ds[o + N - i]
        yy_lookup[i] = max(0.0, yy)
    yy = float(yy_lookup[T0])
    best_xy, best_yy = xy, yy
    g = g0 = _gain(xy, xx, yy)
    arms, past_min, accepted = set(), False, 0  # accepted: the k of the candidate that was taken last (0: T0 kept)
    for k in range(2, 16):
        T1 = (2 * T0 + k) // (2 * k)
        if T1 < minperiod:
            past_min = True
            break
        if k == 2:
            T1b = T0 if T1 + T0 > maxperiod else T0 + T1
        else:
            T1b = (2 * second_check[k] * T0 + k) // (2 * k)
        xy = 0.5 * (corr(T1) + corr(T1b))
        yy = 0.5 * float(yy_lookup[T1] + yy_lookup[T1b])
        g1 = _gain(xy, xx, yy)
        if abs(T1 - prev_period) <= 1:
            cont = prev_gain
            arms.add("full")
        elif abs(T1 - prev_period) <= 2 and 5 * k * k < T0:
            cont = 0.5 * prev_gain
            arms.add("half")
        else:
            cont = 0.0
            arms.add("none")
        thresh = max(0.3, 0.7 * g0 - cont)
        if T1 < 3 * minperiod:
            thresh = max(0.4, 0.85 * g0 - cont)
        elif T1 < 2 * minperiod:  # as published: never taken
            thresh = max(0.5, 0.9 * g0 - cont)
        if D.gt(g1, thresh):
            best_xy, best_yy, T, g = xy, yy, T1, g1
            accepted = k
    best_xy = max(0.0, best_xy)
    pg = 1.0 if not D.gt(best_yy, best_xy) else best_xy / (best_yy + 1.0)  # (best_yy <= best_xy) ? 1 : ...
    xc = [corr(T + k - 1) for k in range(3)]
    offset = 0
    if D.gt(xc[2], 0.7 * xc[1] + 0.3 * xc[0]):
        offset = 1
    elif D.gt(xc[0], 0.7 * xc[1] + 0.3 * xc[2]):
        offset = -1
    if D.gt(pg, g):
        pg = g
    index = 2 * T + offset
    clamped_final = index < minperiod0
    if clamped_final:
        index = minperiod0
    ops = (xx, corr(T0), float(yy_lookup[T0]), g0, best_xy, best_yy, xc[0], xc[1], xc[2], pg)
    return index, float(pg), {"clamped_t0": clamped_t0, "clamped_final": clamped_final, "past_min": past_min, "arms": arms,
                              "T": T, "T0": T0, "accepted": accepted, "ops": ops}


# ------------------------------------------------------------------------------------------------ metrics and bounds
def buffer_error(got: np.ndarray, ref: np.ndarray) -> float:
    """max |d| / the reference buffer's peak; an all-zero reference demands exact zeros (else inf)."""
    ref = np.asarray(ref, dtype=np.float64)
    d = float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref)))
    peak = float(np.max(np.abs(ref)))
    if peak == 0.0:
        return 0.0 if d == 0.0 and not np.any(np.asarray(got).view(np.uint32) & 0x7FFFFFFF) else float("inf")
    return d / peak


def operand_distance(f32_ops: np.ndarray, f64_ops: np.ndarray, scales: np.ndarray) -> float:
    """Largest |f32 - f64| / max(|f32|, |f64|) over the comparison operands that are well conditioned: |f64| at least 1 % of
    the scale that bounds the operand's own rounding error (a correlation that cancels to nearly nothing has no bounded
    relative error in ANY f32 summation order, and says nothing about the arithmetic)."""
    a, b, s = (np.asarray(v, dtype=np.float64) for v in (f32_ops, f64_ops, scales))
    ok = (np.abs(b) >= 1e-2 * s) & (np.abs(b) > 0)
    if not np.any(ok):
        return 0.0
    return float(np.max(np.abs(a - b)[ok] / np.maximum(np.abs(a), np.abs(b))[ok]))


def magnitude_bound(restatement_worst: float, scale: float = 1.0) -> float:
    """4 x the restatement's own worst distance from f64 on the same cells, never under 4 f32 epsilons of the scale."""
    return max(4.0 * restatement_worst, 4.0 * F32_EPS * scale)


def tau_bound(restatement_operand_distance: float) -> float:
    return max(4.0 * restatement_operand_distance, 4.0 * F32_EPS)


# ------------------------------------------------------------------------------------------------ the checker
def check_buffers(got: np.ndarray, spans: np.ndarray) -> np.ndarray:
    """got [frames, streams, 864] against pitch_downsample of span[s, 480 (f + 1) : 480 (f + 1) + 1728]: buffer_error per cell."""
    frames, streams = got.shape[:2]
    err = np.empty((frames, streams))
    for f in range(frames):
        for s in range(streams):
            ref, _ = pitch_downsample(spans[s, FRAME * (f + 1):FRAME * (f + 1) + PBUF])
            err[f, s] = buffer_error(got[f, s], ref)
    return err


def check_search(ds: np.ndarray, index: np.ndarray, tau: float, ops: np.ndarray | None = None) -> dict:
    """The subject's search index per cell ([..., 864] / [...]) against the f64 search of the SUBJECT'S whitened buffer.
    status [...]: 0 equal, 1 excused by the replay, 2 not reachable.  `info`: the strict f64 search's, per cell (flat order).
    `ops` [..., 3]: the subject's f32 a b c -> `operand_distance` over the cells that are equal."""
    shape = index.shape
    flat_ds, flat_i = ds.reshape(-1, HALF), np.asarray(index).reshape(-1)
    status, infos, dist = np.zeros(flat_i.size, dtype=np.int64), [], 0.0
    for c in range(flat_i.size):
        state, result = replay(lambda D: pitch_search(flat_ds[c], D), int(flat_i[c]), tau, key=lambda r: r[0])
        status[c] = {"equal": 0, "excused": 1, "fail": 2}[state]
        strict = pitch_search(flat_ds[c])[1] if state != "equal" else result[1]
        infos.append(strict)
        if ops is not None and state == "equal" and not strict["best0_at_edge"]:
            x = flat_ds[c].astype(np.float64)[PMAX >> 1:][:PFRAME >> 1]
            dist = max(dist, operand_distance(ops.reshape(-1, 3)[c], strict["abc"], np.full(3, float(np.dot(x, x)))))
    return {"status": status.reshape(shape), "info": infos, "operand_distance": dist}


TRACKER_OP_SCALES = ("xx", "xx", "xx", 1.0, "xx", "xx", "xx", "xx", "xx", 1.0)


def check_tracker(ds: np.ndarray, final_index: np.ndarray, calls, end_period: np.ndarray, end_gain: np.ndarray, tau: float,
                  ops: np.ndarray | None = None) -> dict:
    """The subject's final pitch index per cell and its tracker state per call end, against f64.

    ds [frames, streams, 864], final_index [frames, streams]: the subject's.  `calls`: frames per call; end_period /
    end_gain [calls, streams]: the subject's last_period / last_gain after each call.  Per cell the f64 search of the
    subject's whitened buffer feeds the f64 remove_doubling together with the SUBJECT'S previous final index and a carried
    f64 gain, which is re-synchronised to the subject's last_gain at every call end.  status [frames, streams] as
    check_search (the replay runs through the search and the tracker together); gain_error [calls, streams] = |subject's
    last_gain - carried gain| before the re-synchronisation; period_wrong: (call, stream) where last_period is not the last
    frame's index.  `ops` [frames, streams, 13]: the subject's f32 operands (af_rnnoise.h) -> operand_distance."""
    frames, streams = final_index.shape
    status = np.zeros((frames, streams), dtype=np.int64)
    gain_error = np.zeros((len(calls), streams))
    period_wrong, infos, dist = [], {}, 0.0
    ends = np.cumsum(calls) - 1
    for s in range(streams):
        prev_index, carried, call = 0, 0.0, 0
        for f in range(frames):
            buf = ds[f, s]

            def fn(D, buf=buf, prev_index=prev_index, carried=carried):
                si, _ = pitch_search(buf, D)
                return remove_doubling(buf, si, prev_index, carried, D)

            state, result = replay(fn, int(final_index[f, s]), tau, key=lambda r: r[0])
            status[f, s] = {"equal": 0, "excused": 1, "fail": 2}[state]
            infos[(f, s)] = result[2]
            if ops is not None and state == "equal":
                xx = result[2]["ops"][0]
                scales = np.array([xx if v == "xx" else v for v in TRACKER_OP_SCALES])
                dist = max(dist, operand_distance(ops[f, s, 3:13], result[2]["ops"], scales))
            carried = result[1]
            prev_index = int(final_index[f, s])
            if f == ends[call]:
                gain_error[call, s] = abs(float(end_gain[call, s]) - carried)
                if int(end_period[call, s]) != prev_index:
                    period_wrong.append((call, s))
                carried = float(end_gain[call, s])
                call += 1
    return {"status": status, "gain_error": gain_error, "period_wrong": period_wrong, "info": infos, "operand_distance": dist}


def excused_share(status: np.ndarray) -> float:
    return float(np.mean(np.asarray(status) == 1))
