"""The de-esser's stimulus and cases (tests/test_deesser_stimulus.py on the oracle alone, tests/test_gpu_deesser_alone.py on the device).

`batch(case)` is a deterministic batch of 67 streams -- one full 64-lane group and a group of 3, so the tile edges are streams
0, 63, 64 and 66 -- built here from seeded `numpy` generators.  Every stream has a role (`roles()`), and the edge streams
carry full-scale ones:

  ess        voiced harmonic series alternating with 4.5-9 kHz noise bursts: baseline rise and fall, cap, budget rescale
  narrow     tone bursts centred inside the MIDDLE band of the case's layout: one band leads, the other two's dominance is small (the
             detectors are second-order, so even this gives a narrowness of only ~0.36; see tests/test_deesser_stimulus.py)
  wide       white / 2.5-14 kHz bursts: narrowness near 1/3 (below the 0.34 gate); a manual-mode reduction that stays under its cap
  ramp       voice with sibilance rising linearly from 0: slow crossings of every threshold, long runs of the 0.001 dB hold
  late       exact zeros for the first quarter, then `ess`: envelopes exactly 0 (the <= 1e-10 guards, the -200 dB floor)
  quiet      `ess` at -62 dBFS: `voice_active` false for the whole stream
  loud       voice under sibilance that exceeds +-1.0: the input clamp (where it is on), large reductions
  nonfinite  `ess` with NaN, +Inf and -Inf sprinkled in, some at call edges and some at control-block edges: the input scrub
  dip        voice under steady sibilance that drops to -70 dBFS from 0.2 to 0.85 of the stream: `voice_active` goes false while
             the baselines are not 0 (they decay by `baseline_inactive` per sample) and comes back
  dc         `ess` + 0.03, only with `dc=True` (the front-end case; otherwise these streams are further `ess` streams)
  twin       a bit-for-bit copy of another stream in the OTHER 64-lane group at a different lane (`TWINS`)

A case is a sample rate, a length, a call pattern and the `deesser_*` settings of `simulate_auto_eq_chain` (EQ, compressor and
limiter are switched off by the tests that run the de-esser alone)."""
from __future__ import annotations

import numpy as np

N_STREAMS = 67
SEED = 20
TWINS = {65: 7, 30: 64}  # copy: original -- group 0 lane 7 -> group 1 lane 1, group 1 lane 0 -> group 0 lane 30
_EDGE_ROLES = {0: "ess", 63: "loud", 64: "ess", 66: "narrow", 7: "nonfinite"}
_CYCLE = ("wide", "ramp", "late", "quiet", "dip", "narrow", "dc", "loud", "nonfinite", "ess")


def control_block(fs: float) -> int:
    return int(min(max(round(fs * 0.020), 1), 8192))


def _de(**kw) -> dict:
    return {"deesser_enabled": True, "compressor_enabled": False, "limiter_enabled": False, **{"deesser_" + k: v for k, v in kw.items()}}


def _calls(n: int, head=(7_001, 1, 2_880, 12_345)) -> tuple:
    """Ragged calls: one of 1 sample, one that is no multiple of 4, 64 or the control block, one longer than two stage windows."""
    assert n > sum(head)
    return tuple(head) + (n - sum(head),)


_SHORT, _LONG = 26_417, 49_003  # > 9 and > 17 stage windows of 2880 (the stage form keeps 16 parameter slots)
_B = dict(auto_enabled=True, auto_amount=0.85, max_reduction_db=6.0)
_CLAMP_EDGE = dict(auto_enabled=False, ratio=20.0, attack_ms=0.1, release_ms=5.0, max_reduction_db=8.0)
# name: (sample rate, samples, calls, settings)
CASES = {
    "A": (48_000, _SHORT, _calls(_SHORT), _de()),
    "B": (48_000, _LONG, _calls(_LONG), _de(**_B)),
    "C": (48_000, _SHORT, _calls(_SHORT), _de(auto_enabled=True, auto_amount=0.5, max_reduction_db=24.0)),
    "D": (48_000, _SHORT, _calls(_SHORT), _de(auto_enabled=False, threshold_db=-40.0, ratio=6.0, max_reduction_db=8.0)),
    "E-60": (48_000, _SHORT, _calls(_SHORT), _de(threshold_db=-60.0, **_CLAMP_EDGE)),
    "E-6": (48_000, _SHORT, _calls(_SHORT), _de(threshold_db=-6.0, **_CLAMP_EDGE)),
    "E-out": (48_000, _SHORT, _calls(_SHORT), _de(auto_enabled=False, threshold_db=-90.0, ratio=50.0, attack_ms=0.01, release_ms=1000.0,
                                                    auto_amount=1.5, max_reduction_db=30.0)),
    "F-max0": (48_000, _SHORT, _calls(_SHORT), _de(auto_enabled=True, max_reduction_db=0.0)),
    "F-ratio1": (48_000, _SHORT, _calls(_SHORT), _de(auto_enabled=False, ratio=1.0, threshold_db=-40.0)),
    # the first calls of G end inside the 72-sample crossfade that moving the cuts leaves pending on the nine filters
    "G-high": (48_000, _SHORT, _calls(_SHORT, (37, 1, 7_001, 12_345)), _de(low_cut_hz=12_000.0, high_cut_hz=12_200.0, **_B)),
    "G-full": (48_000, _SHORT, _calls(_SHORT, (37, 1, 7_001, 12_345)), _de(low_cut_hz=2_000.0, high_cut_hz=16_000.0, **_B)),
    # ... and G-moved's in a HOLD of the dynamic EQs' gain after an update cancelled their crossfade (attack 30 ms: the reduction creeps;
    # with B's 2 ms the gain is updated on every sample of the crossfade and a lost `cancelled` flag would not show)
    "G-moved": (48_000, _SHORT, _calls(_SHORT, (53, 1, 7_001, 12_345)), _de(low_cut_hz=3_500.0, high_cut_hz=9_000.0, attack_ms=30.0, **_B)),
    "H-44k1": (44_100, 45_113, _calls(45_113), _de(**_B)),   # > 17 windows of 2646
    "H-96k": (96_000, 52_811, _calls(52_811), _de(**_B)),    # 0.55 s: > 27 windows of 1920
}


def band_layout(settings: dict) -> tuple:
    """(low cut, lower split, upper split, high cut) after `set_low_cut_hz` then `set_high_cut_hz` on the defaults (deesser.rs:231-245,
    319-334)."""
    lo, hi = 4000.0, 11000.0
    lo = float(np.clip(settings.get("deesser_low_cut_hz", 4000.0), 2000.0, 12000.0))
    if hi <= lo + 200.0:
        hi = float(np.clip(lo + 200.0, 2200.0, 16000.0))
    hi = float(np.clip(settings.get("deesser_high_cut_hz", 11000.0), 2200.0, 16000.0))
    if hi <= lo + 200.0:
        lo = float(np.clip(hi - 200.0, 2000.0, 12000.0))
    span = max(hi - lo, 600.0)
    return lo, lo + span / 3.0, lo + span * 2.0 / 3.0, hi


def roles(dc: bool = False) -> list:
    out = []
    k = 0
    for s in range(N_STREAMS):
        if s in TWINS:
            out.append("twin")
        elif s in _EDGE_ROLES:
            out.append(_EDGE_ROLES[s])
        else:
            role = _CYCLE[k % len(_CYCLE)]
            k += 1
            out.append(role if (role != "dc" or dc) else "ess")
    return out


def role_streams(dc: bool = False) -> dict:
    """role: the stream that represents it (an edge stream where one carries the role)."""
    r = roles(dc)
    first = {}
    for s in (0, 63, 66, 7, *range(N_STREAMS)):
        if r[s] != "twin":
            first.setdefault(r[s], s)
    return first


# ------------------------------------------------------------------------------------------------------------ parts
def _voice(rng, n, fs):
    t = np.arange(n) / fs
    f0 = rng.uniform(95.0, 230.0)
    x = np.zeros(n)
    k = 1
    while k * f0 < 3400.0:
        x += np.sin(2.0 * np.pi * k * f0 * t + rng.uniform(0.0, 2.0 * np.pi)) / k
        k += 1
    x *= 0.6 + 0.4 * np.sin(2.0 * np.pi * rng.uniform(2.0, 4.5) * t + rng.uniform(0.0, 2.0 * np.pi))
    return x / np.abs(x).max()


def _band_noise(rng, n, fs, lo, hi):
    """White noise through a 255-tap Blackman-windowed band-pass (lo = None: white), peak 1."""
    taps = 255
    w = rng.standard_normal(n + taps - 1)
    if lo is not None:
        m = np.arange(taps) - (taps - 1) / 2.0
        hi = min(hi, 0.49 * fs)
        h = (2.0 * hi / fs) * np.sinc(2.0 * hi / fs * m) - (2.0 * lo / fs) * np.sinc(2.0 * lo / fs * m)
        w = np.convolve(w, h * np.blackman(taps), mode="valid")
    else:
        w = w[:n]
    return w / np.abs(w).max()


def _gate(rng, n, fs, period_s=0.110, on_s=0.045, edge_s=0.004):
    """A 0..1 burst envelope with raised-cosine edges."""
    t = (np.arange(n) / fs + rng.uniform(0.0, period_s)) % period_s
    up = np.clip(t / edge_s, 0.0, 1.0)
    down = np.clip((on_s - t) / edge_s, 0.0, 1.0)
    return 0.5 - 0.5 * np.cos(np.pi * np.minimum(up, down))


def _ess(rng, n, fs, voice=0.5, sibilance=0.55):
    g = _gate(rng, n, fs)
    return voice * _voice(rng, n, fs) * (1.0 - 0.85 * g) + sibilance * _band_noise(rng, n, fs, 4500.0, 9000.0) * g


def _stream(role, rng, n, fs, middle, full_scale, edges):
    if role in ("ess", "dc", "nonfinite"):
        x = _ess(rng, n, fs)
    elif role == "dip":  # (sibilance throughout: the ratio, and with it the baseline, is not 0 when the level drops)
        x = 0.15 * _voice(rng, n, fs) + 0.8 * _band_noise(rng, n, fs, 4500.0, 9000.0)
        t = np.arange(n) / n
        edge = 0.005 * fs / n
        inside = np.minimum(np.clip((t - 0.2) / edge, 0.0, 1.0), np.clip((0.85 - t) / edge, 0.0, 1.0))
        x = x / np.abs(x).max() * 0.95 * 10.0 ** (-70.0 / 20.0 * (0.5 - 0.5 * np.cos(np.pi * inside)))
        return x.astype(np.float32)
    elif role == "narrow":
        f = 0.5 * (middle[0] + middle[1]) + rng.uniform(-0.1, 0.1) * (middle[1] - middle[0])
        g = _gate(rng, n, fs, on_s=0.06)
        x = 0.08 * _voice(rng, n, fs) * (1.0 - g) + 0.9 * np.sin(2.0 * np.pi * f * np.arange(n) / fs) * g
    elif role == "wide":
        noise = _band_noise(rng, n, fs, None, None) if rng.integers(2) else _band_noise(rng, n, fs, 2500.0, 14000.0)
        x = 0.12 * _voice(rng, n, fs) + 0.7 * noise * _gate(rng, n, fs, on_s=0.06)
    elif role == "ramp":
        x = 0.35 * _voice(rng, n, fs) + 0.6 * _band_noise(rng, n, fs, 4500.0, 9000.0) * np.linspace(0.0, 1.0, n)
    elif role == "late":
        x = _ess(rng, n, fs)
        x[: n // 4] = 0.0
    elif role == "quiet":
        x = _ess(rng, n, fs)
        return (x / np.abs(x).max() * 10.0 ** (-62.0 / 20.0)).astype(np.float32)
    elif role == "loud":
        x = _ess(rng, n, fs, voice=0.5, sibilance=1.0)
        return (x / np.abs(x).max() * 1.6).astype(np.float32)
    else:
        raise ValueError(role)
    gain = 0.95 if full_scale else 10.0 ** (rng.uniform(-16.0, -2.0) / 20.0)
    x = (x / np.abs(x).max() * gain)
    if role == "dc":
        x = x + 0.03
    x = x.astype(np.float32)
    if role == "nonfinite":
        bad = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
        at = np.concatenate([edges, edges - 1, rng.integers(0, n, 24)])
        at = np.unique(at[(at >= 0) & (at < n)])
        x[at] = bad[np.arange(at.size) % 3]
    return x


def batch(case: str, dc: bool = False, seed: int = SEED) -> np.ndarray:
    """[67, n] float32 for `CASES[case]`."""
    fs, n, calls, settings = CASES[case]
    _, split_a, split_b, _ = band_layout(settings)
    cb = control_block(fs)
    call_edges = np.cumsum(calls)[:-1]
    edges = np.concatenate([call_edges[:3], cb * np.array([1, 7, 20, 33])])
    r = roles(dc)
    out = np.zeros((N_STREAMS, n), dtype=np.float32)
    for s in range(N_STREAMS):
        if s not in TWINS:
            out[s] = _stream(r[s], np.random.default_rng([seed, s]), n, fs, (split_a, split_b), s in (0, 63, 64, 66), edges)
    for copy, original in TWINS.items():
        out[copy] = out[original]
    return out
