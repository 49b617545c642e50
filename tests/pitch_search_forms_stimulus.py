"""Stimulus of the pitch-search form tests: what the stand-alone search tap is run on when one build of
supp_pitchsearch4_kernel is held to a recording of another, bit for bit.  Deterministic, numpy only, no GPU.

Three parts (`parts()` gives them in recording order):
  search<n>   pitch_stage_stimulus.search_spans(n), n = 1, 3, 4, 6 frames (1, 3, 4 and 4 + 2 live waves)
  stimulus    pitch_stage_stimulus.model_spans(): the 31 read streams x 43 frames
  steer       single-frame spans built to steer the coarse winner (below)

The steering spans are sparse: raised-cosine bumps a few samples wide in otherwise exact zeros.  In the 4x-decimated domain of
the coarse stage (y4[i] = whitened[2 i], x4 = y4[192:432]) a bump at x4[a] and bumps at y4[a + L0] and y4[a + L1] give a
correlation that is positive at the lags L0 and L1 (and, weaker, at their neighbours) and next to nothing elsewhere: L0 and
L1 become the two coarse candidates, in the order their amplitudes and the window energies decide.  The decimation and the
five-tap whitening filter are short, so the exact zeros between the bumps survive them.  A shift of the y bumps by -1, 0 or +1
input samples moves the fine maximum between the two fine lags of a coarse one and steers the interpolation offset.
  pair        (L0, L0 + d mod 147) for every L0 and d = 37, 75, 110; the second bump alternately weaker and stronger
  near        L1 = L0 + 1 and L0 + 2: overlapping fine neighbourhoods
  edge        the lags 0, 1, 145, 146 as the stronger and as the weaker bump
  negative    a one-sided decaying pulse (halving per sample, 24 samples) in x and its negative in y: the whitened pulses keep
              one sign each, so the correlation is negative where they overlap and exactly zero elsewhere (index 768)
  quiet       faint bumps with the x bump beyond every energy window and a stretch of lags whose window holds exact zeros
              only: the window-energy recurrence comes back to 1 + e - e there, and its max(1, .) clamp decides
tests/test_pitch_search_forms_ref.py proves on the f64 search which classes these reach.
"""
from __future__ import annotations

import functools

import numpy as np

import pitch_stage_stimulus as T

FRAME, PBUF = T.FRAME, T.PBUF
N_LAGS = 147                      # coarse lags
ANCHOR = 20                       # a: the x bump sits at x4[a] = y4[192 + a]
WIDTH = 6                         # half width of a bump, input samples
LEVEL = 3000.0                    # of +-32768
PAIR_STEPS = (37, 75, 110)
EDGE_LAGS = (0, 1, 145, 146)


def _bump(x: np.ndarray, pos: int, amp: float) -> None:
    k = np.arange(-WIDTH, WIDTH + 1)
    x[pos - WIDTH:pos + WIDTH + 1] += amp * 0.5 * (1.0 + np.cos(np.pi * k / (WIDTH + 1)))


def steer_span(lag0: int, lag1: int, second: float = 0.7, shift: int = 0, level: float = LEVEL, anchor: int = ANCHOR) -> np.ndarray:
    """[1728 + 480] float32: one frame whose pitch buffer holds a bump at x4[anchor], one at y4[anchor + lag0] and one of
    `second` times that at y4[anchor + lag1], the y bumps `shift` input samples late."""
    x = np.zeros(PBUF + FRAME)
    _bump(x, FRAME + 4 * (192 + anchor), level)
    _bump(x, FRAME + 4 * (anchor + lag0) + shift, level)
    _bump(x, FRAME + 4 * (anchor + lag1) + shift, second * level)
    return x.astype(np.float32)


def quiet_span(level: float) -> np.ndarray:
    """The x bump at y4[400] (no energy window of the coarse or the fine stage reaches it), y bumps at y4[10] and y4[300]
    (lag 92): the windows of the coarse lags 12 .. 59 hold exact zeros only."""
    x = np.zeros(PBUF + FRAME)
    _bump(x, FRAME + 4 * 400, level)
    _bump(x, FRAME + 4 * 10, level)
    _bump(x, FRAME + 4 * 300, level)
    return x.astype(np.float32)


QUIET_LEVELS = (0.5, 1.0, 3.0, 7.0)


@functools.lru_cache(maxsize=None)
def steer_cases() -> tuple:
    """((kind, lag0, lag1, second, shift), ...) in span order."""
    cases = []
    for lag0 in range(N_LAGS):
        for n, d in enumerate(PAIR_STEPS):
            cases.append(("pair", lag0, (lag0 + d) % N_LAGS, 0.7 if (lag0 + n) % 2 == 0 else 1.0 / 0.7, (lag0 + d) % 3 - 1))
    for lag0 in range(0, N_LAGS - 2, 9):
        cases.append(("near", lag0, lag0 + 1, 0.9, 0))
        cases.append(("near", lag0, lag0 + 2, 0.9, lag0 % 3 - 1))
    for e in EDGE_LAGS:
        for other in (60, 100):
            cases.append(("edge", e, other, 0.6, 0))
            cases.append(("edge", other, e, 0.6, 0))
    cases.append(("negative", 40, 40, -1.0, 0))
    for level in QUIET_LEVELS:
        cases.append(("quiet", 92, 92, level, 0))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def steer_spans() -> np.ndarray:
    """[len(steer_cases()), 1728 + 480] float32."""
    rows = []
    for kind, lag0, lag1, second, shift in steer_cases():
        if kind == "quiet":
            rows.append(quiet_span(second))
        elif kind == "negative":
            x = np.zeros(PBUF + FRAME)
            pulse = LEVEL * 0.5 ** np.arange(24)
            x[FRAME + 4 * (192 + ANCHOR):][:24] += pulse
            x[FRAME + 4 * (ANCHOR + lag0):][:24] -= pulse
            rows.append(x.astype(np.float32))
        else:
            rows.append(steer_span(lag0, lag1, second, shift))
    spans = np.stack(rows)
    spans.setflags(write=False)
    return spans


def parts() -> tuple:
    """((name, spans [streams, 1728 + 480 frames], frames), ...): every run of the tap, in recording order."""
    out = [(f"search{n}", T.search_spans(n), n) for n in T.SEARCH_FRAMES]
    out.append(("stimulus", T.model_spans(), T.N_FRAMES))
    out.append(("steer", steer_spans(), 1))
    return tuple(out)


def buffer_hashes(ds: np.ndarray) -> np.ndarray:
    """[frames, streams, 864] float32 -> [frames, streams] uint64: FNV-1a over the 864 words' bit patterns of every cell
    (a negative zero or another NaN payload is another hash)."""
    w = np.ascontiguousarray(ds, dtype=np.float32).view(np.uint32).astype(np.uint64)
    h = np.full(w.shape[:-1], 0xCBF29CE484222325, dtype=np.uint64)
    prime = np.uint64(0x100000001B3)
    with np.errstate(over="ignore"):
        for i in range(w.shape[-1]):
            h = (h ^ w[..., i]) * prime
    return h
