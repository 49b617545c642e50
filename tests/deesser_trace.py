"""The oracle's de-esser stepped sample by sample through the ctypes mirror of its struct (`af_oracle_py.DeEsser`), and the
predicates of `afo_deesser_process_sample` recomputed from the recorded state: which branch every sample and band took.
CPU only; used by tests/test_deesser_stimulus.py (and for reading a device / oracle difference sample by sample)."""
from __future__ import annotations

import ctypes as C

import numpy as np

import af_oracle_py as O

STATE_DTYPE = np.dtype(O.DeEsser)


def new_deesser(fs: float, settings: dict):
    """An `afo_deesser` of the test's own, enabled and set up as `make_chain` sets the chain's up."""
    L = O.lib()
    d = O.DeEsser()
    L.afo_deesser_init(C.byref(d), float(fs))
    L.afo_deesser_set_enabled(C.byref(d), 1)
    O.deesser_apply(C.byref(d), O.settings_from_dict(settings))
    return d


def trace(x: np.ndarray, fs: float, settings: dict):
    """(output float32 [n], state after every sample [n] of STATE_DTYPE)."""
    d = new_deesser(fs, settings)
    step = O.lib().afo_deesser_process_sample
    p = C.byref(d)
    view = np.frombuffer(d, dtype=STATE_DTYPE, count=1)
    n = x.size
    state = np.empty(n, dtype=STATE_DTYPE)
    out = np.empty(n, dtype=np.float32)
    for i, v in enumerate(np.asarray(x, dtype=np.float32).tolist()):
        out[i] = step(p, v)
        state[i] = view[0]
    return out, state


def _db(v):
    return 20.0 * np.log10(np.maximum(v, 1e-10))


def _lerp(a, b, t):
    return a + (b - a) * t


def predicates(state: np.ndarray) -> dict:
    """Per sample and band ([n, 3] bool unless noted) what `afo_deesser_process_sample` decided, from the state after each sample
    (the envelopes are final before any decision; baseline / gain comparisons use the previous sample's state)."""
    env = state["bands"]["env"]                      # [n, 3]
    total = env.sum(axis=1, keepdims=True)
    top = env.max(axis=1, keepdims=True)
    side_db = _db(env)
    voice_db = _db(np.maximum(state["broadband_env"][:, None] - total * 0.6, 1e-8))
    ratio_db = np.maximum(side_db - voice_db, 0.0)
    narrowness = np.where(total > 1e-10, top / np.where(total > 0.0, total, 1.0), 0.0)
    ratio_conf = np.clip((ratio_db - 1.5) / 8.5, 0.0, 1.0)
    s0 = state[0]
    auto = bool(s0["auto_enabled"])
    max_red = float(s0["max_reduction_db"])
    amount = float(np.clip(s0["auto_amount"], 0.0, 1.0))
    p = {
        "zero_env": np.broadcast_to(total <= 1e-10, env.shape),
        "narrow_support_on": (ratio_db > 6.0) & (side_db > -45.0),
        "narrowness_low": np.broadcast_to((total > 1e-10) & (narrowness < 0.34), env.shape),
        "narrowness_high": np.broadcast_to(narrowness > 0.68, env.shape),
        "ratio_conf_low": ratio_conf <= 0.12,
    }
    p["narrow_support_off"] = ~p["narrow_support_on"]
    p["ratio_conf_high"] = ~p["ratio_conf_low"]
    confidence = state["bands"]["confidence"]
    baseline = state["bands"]["baseline_excess_db"]
    previous_baseline = np.vstack([np.zeros((1, 3)), baseline[:-1]])
    if auto:
        active = (voice_db > -55.0) | (side_db > -55.0)
        baseline_target = np.clip(ratio_db * 0.45, 0.0, 24.0)
        floor = float(np.clip(_lerp(0.28, 0.06, amount), 0.0, 0.95))
        cap = min(_lerp(0.8, 14.0, amount), max_red * 0.75)
        gain = np.clip((confidence - floor) / (1.0 - floor), 0.0, 1.0)
        raw = np.maximum(ratio_db - baseline - _lerp(8.0, 0.8, amount), 0.0) * _lerp(0.08, 1.9, amount) * gain
        target = np.clip(raw, 0.0, cap)
        p["voice_active_true"] = active
        p["voice_active_false"] = ~active
        p["baseline_decay"] = ~active & (previous_baseline > 1e-3)  # `baseline *= baseline_inactive` on a baseline that is not 0
        p["baseline_fall"] = active & (baseline_target < previous_baseline)
        p["baseline_rise"] = active & (baseline_target > previous_baseline)
        p["band_cap_under_budget"] = (raw >= cap) & (cap > 0.0) & (target.sum(axis=1, keepdims=True) <= max_red)
    else:
        threshold = float(s0["threshold_db"])
        ratio_threshold = float(np.clip((threshold + 60.0) * 0.10, 0.0, 6.0))
        over_level = side_db > threshold
        ratio_over = ratio_db - ratio_threshold
        gain = np.clip((confidence - 0.22) / (1.0 - 0.22), 0.0, 1.0)
        raw = (1.0 - 1.0 / float(s0["ratio"])) * np.minimum(side_db - threshold, ratio_over) * gain
        target = np.where(over_level & (ratio_over > 0.0), np.clip(raw, 0.0, max_red * 0.75), 0.0)
        p["manual_below_threshold"] = ~over_level
        p["manual_ratio_exit"] = over_level & (ratio_over <= 0.0)
        p["manual_active"] = over_level & (ratio_over > 0.0)
    target_sum = target.sum(axis=1, keepdims=True)
    p["budget_rescale"] = np.broadcast_to((target_sum > max_red) & (target_sum > 0.0), env.shape)
    gain_db = state["bands"]["dynamic_eq"]["gain_db"]
    previous_gain = np.vstack([np.zeros((1, 3)), gain_db[:-1]])
    wanted = -state["bands"]["reduction_db"]
    p["update"] = gain_db != previous_gain
    p["hold"] = (gain_db == previous_gain) & (wanted != gain_db)  # the reduction moved, by 0.001 dB or less: the gain stayed
    return p
