"""Stimulus and expected values for tests/test_gpu_prepass.py: what the suppressor's pre-pass must leave in the model-input
buffer, from the oracle alone.

    front end     afo_sanitize_and_clamp (clamped variants), then oracle.prefilter (DC block + 80 Hz high-pass)
    model input   oracle.scale_sample_for_model per sample (wrapper protocol) or suppressor_stage_ref.raw_model_input (raw)
    high-pass     RNNoise's second-order input high-pass, restated in numpy float32 with one rounded operation per line
                  (suppressor_stage_ref.biquad_hp_f32; the library is built with -ffp-contract=off: nothing is fused)

Every filter runs once over the whole timeline of a stream, so its state is carried across the calls exactly as the engine
carries it.  A window's row of the buffer is the 1728 model-input samples in front of the window (zeros before the stream's
start) followed by the window's own.
"""
from __future__ import annotations

import functools

import numpy as np

import chain_oracle
import signals as S
import suppressor_stage_ref as R

N_STREAMS = 66              # one full 64-stream group and a group of two, whose other 62 rows are clamped to stream 65
READ = (0, 63, 64, 65)      # first and last row of the full group, both rows of the short one
SILENT = 64
# 1, 4 and 12 frames are one window each (a window is up to 16 frames at control block 480): history from the zeroed state,
# then from the saved state.  The 20-frame call is two windows, 16 + 4: the second takes its history from the first one's buffer.
CALLS = (1, 4, 12, 20)
FRAMES = sum(CALLS)
HISTORY = 1728
VARIANTS = {  # name: (input clamp, DC block + 80 Hz high-pass, raw protocol): every instantiation of supp_prefilter_kernel
    "front-end-off": (False, False, False),
    "raw": (False, False, True),
    "dc-hp": (False, True, False),
    "raw-dc-hp": (False, True, True),
    "clamp": (True, False, False),
    "raw-clamp": (True, False, True),
    "clamp-dc-hp": (True, True, False),
    "raw-clamp-dc-hp": (True, True, True),
}


@functools.lru_cache(maxsize=None)
def stimulus(nonfinite: bool) -> np.ndarray:
    """[66, 37 x 480] float32: per stream a gain of 2.6 / 1.0 / 0.4 (2.6 drives the soft clip far beyond +-1) and a DC offset
    of +0.05 / -0.03; stream 65 at 2.2; stream 64 silent.  `nonfinite`: one NaN, one +inf, one -inf (clamped variants only)."""
    x = S.batch_signal(N_STREAMS, FRAMES).astype(np.float64)
    for s in range(N_STREAMS):
        gain = (2.6, 1.0, 0.4)[s % 3] if s != 65 else 2.2
        x[s] = x[s] * gain + (0.05 if s % 2 == 0 else -0.03)
    x[SILENT] = 0.0
    x = x.astype(np.float32)
    assert all(float(np.abs(x[s]).max()) > 1.2 for s in (0, 63, 65)) and not x[SILENT].any()
    if nonfinite:
        x[63, 100] = -np.inf   # in the first call
        x[65, 500] = np.nan    # in the second
        x[0, 3000] = np.inf    # in the third
    x.setflags(write=False)
    return x


def front_end(x: np.ndarray, clamp: bool, dc_hp: bool, oracle) -> np.ndarray:
    """One stream through the realtime front end, as the engine's calls see it (the state runs on across them)."""
    y = chain_oracle.sanitize(x, True) if clamp else np.array(x, dtype=np.float32)
    return oracle.prefilter(y) if dc_hp else y


_EXPECTED: dict = {}


def expected_rows(name: str, oracle) -> np.ndarray:
    """[len(READ), 1728 + 37 x 480] float32: the model input of the READ streams over the whole timeline behind 1728 zeros.
    Computed once per variant and shared; callers must not change it."""
    if name not in _EXPECTED:
        clamp, dc_hp, raw = VARIANTS[name]
        x = stimulus(clamp)
        sc = np.empty((len(READ), x.shape[1]), dtype=np.float32)
        for i, s in enumerate(READ):
            fe = front_end(x[s], clamp, dc_hp, oracle)
            if raw:
                sc[i] = R.raw_model_input(fe)
            else:
                sc[i] = np.array([oracle.scale_sample_for_model(float(v)) for v in fe], dtype=np.float32)
        y = R.biquad_hp_f32(sc, np.zeros((len(READ), 2), dtype=np.float32))
        rows = np.concatenate([np.zeros((len(READ), HISTORY), dtype=np.float32), y], axis=1)
        rows.setflags(write=False)
        _EXPECTED[name] = rows
    return _EXPECTED[name]
