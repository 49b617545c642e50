"""Deterministic synthetic inputs and waveform metrics shared by the CPU and GPU tests, smoke() and bench.py.

Nothing here is reference text and no reference file is read at run time.  Three kinds of content:

* the golden-KAT generator of `rust-core/src/audio/processor/tests.rs:1824-1851`, vectorised, and its per-stream variation
   -- this repository's own numpy formulation of the Rust test's arithmetic;
* DATA captured from the reference's evaluators by `tools/gen_golden.py` in the build container (tests/golden/*.json): the
  chain settings dicts and band lists they hand to `simulate_auto_eq_chain`, fingerprints of their stimuli, and the values
  their metric functions return on the oracle's output;
* this repository's own generators for those stimuli (held to the fingerprints by tests/test_golden_fixtures.py) and its
  own vectorised forms of the waveform metrics the reports define (held to the captured values by the same test).
"""
from __future__ import annotations

import copy
import json
import pathlib

import numpy as np

SAMPLE_RATE = 48_000
KAT_NOISE_STATE = 0x6A09E667F3BCC909
MASK64 = (1 << 64) - 1

_GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
LIMITER_FIXTURE = json.loads((_GOLDEN / "limiter_lookahead.json").read_text())
ALIASING_FIXTURE = json.loads((_GOLDEN / "dynamics_aliasing.json").read_text())


def kat_signal(n_blocks: int, noise_state: int = KAT_NOISE_STATE, f0: float = 180.0, phrase_hz: float = 1.7) -> np.ndarray:
    """Golden-KAT input (rust-core/src/audio/processor/tests.rs:1824-1851), vectorised.

    f0 / phrase_hz / noise_state generalise it per stream; the
    defaults are the KAT itself.  Tones sit at f0, 2*f0 and 15*f0 (180/360/2700 Hz).
    """
    n = n_blocks * 480
    idx = np.arange(n, dtype=np.float64)
    time = idx / 48000.0
    # LCG: state_{k} = a^k s0 + c (a^k-1)/(a-1)  -- iterate in uint64 blocks for speed
    a = np.uint64(6364136223846793005)
    c = np.uint64(1442695040888963407)
    states = np.empty(n, dtype=np.uint64)
    s = np.uint64(noise_state & MASK64)
    with np.errstate(over="ignore"):
        # jump table: process sequentially in chunks using vectorised affine powers
        chunk = 4096
        mul = np.empty(chunk, dtype=np.uint64)
        add = np.empty(chunk, dtype=np.uint64)
        m, d = np.uint64(1), np.uint64(0)
        for k in range(chunk):
            m = m * a
            d = d * a + c
            mul[k] = m
            add[k] = d
        for start in range(0, n, chunk):
            ln = min(chunk, n - start)
            states[start : start + ln] = mul[:ln] * s + add[:ln]
            s = states[start + ln - 1]
    noise = ((states >> np.uint64(40)).astype(np.uint32).astype(np.float64) / float((1 << 24) - 1) * 2.0 - 1.0) * 0.012
    phrase = 0.25 + 0.75 * np.abs(np.sin(2.0 * np.pi * phrase_hz * time))
    block_index = np.arange(n) // 480
    gate = (((block_index // 12) % 5) == 2).astype(np.float64)
    voiced = (
        0.30 * np.sin(2.0 * np.pi * f0 * time)
        + 0.14 * np.sin(2.0 * np.pi * (2.0 * f0) * time)
        + 0.08 * np.sin(2.0 * np.pi * (15.0 * f0) * time)
    )
    x = phrase * voiced + gate * 0.35 * np.sin(2.0 * np.pi * 7200.0 * time) + noise
    return x.astype(np.float32)


def stream_params(i: int) -> tuple[int, float, float]:
    """Per-stream variation of the KAT generator."""
    state = KAT_NOISE_STATE ^ ((i * 0x9E3779B97F4A7C15) & MASK64)
    f0 = 180.0 * 2.0 ** (((i % 25) - 12) / 24.0)
    phrase = 1.7 * (1.0 + 0.01 * (i % 7))
    return state, f0, phrase


def batch_signal(n_streams: int, n_blocks: int) -> np.ndarray:
    """S3 batch: [n_streams, n_blocks*480] f32, stream-major."""
    out = np.empty((n_streams, n_blocks * 480), dtype=np.float32)
    for i in range(n_streams):
        st, f0, ph = stream_params(i)
        out[i] = kat_signal(n_blocks, st, f0, ph)
    return out


# ------------------------------------------------------------------------------------------------------------------
# Chain configurations of the reference's evaluators: data (tests/golden/*.json), captured at their call into the operator.
def limiter_settings(lookahead_ms: float) -> dict:
    """The settings dict `evaluation/limiter-lookahead-report.json` was rendered with, for one of its lookaheads; other
    lookaheads take the 2 ms dict with `limiter_lookahead_ms` replaced (the evaluator's only per-lookahead key)."""
    table = LIMITER_FIXTURE["settings"]
    key = f"{float(lookahead_ms):g}"
    settings = copy.deepcopy(table[key] if key in table else table["2"])
    settings["limiter_lookahead_ms"] = float(lookahead_ms)
    return settings


LIMITER_BANDS = [tuple(band) for band in LIMITER_FIXTURE["bands"]]
ALIASING_CASES = tuple((name, carrier, modulation) for name, carrier, modulation in ALIASING_FIXTURE["cases"])
ALIASING_SETTINGS = dict(ALIASING_FIXTURE["settings"])
ALIASING_BANDS = [tuple(band) for band in ALIASING_FIXTURE["bands"]]

DEFAULT_TYPED_BANDS = [
    ("low_shelf", 80.0, 0.0, 1.41, 12, True),
    ("bell", 160.0, 0.0, 1.41, 12, True),
    ("bell", 320.0, 0.0, 1.41, 12, True),
    ("bell", 640.0, 0.0, 1.41, 12, True),
    ("bell", 1280.0, 0.0, 1.41, 12, True),
    ("bell", 2500.0, 0.0, 1.41, 12, True),
    ("bell", 5000.0, 0.0, 1.41, 12, True),
    ("bell", 8000.0, 0.0, 1.41, 12, True),
    ("bell", 12000.0, 0.0, 1.41, 12, True),
    ("high_shelf", 16000.0, 0.0, 1.41, 12, True),
]


# ------------------------------------------------------------------------------------------------------------------
# Stimuli of the two evaluators, regenerated from their descriptions (the reports' `configuration`
# blocks).  tests/test_golden_fixtures.py holds every one of them to the SHA-256 / head / tail / checkpoint fingerprints
# that tools/gen_golden.py took from the reference's own generators.
def _seconds(n: int, fs: int) -> np.ndarray:
    return np.arange(n) / fs


def _hann_burst_train(n: int, fs: int) -> np.ndarray:
    """25 ms Hann-windowed 6.5 kHz bursts at 1.35 x full scale, one every 190 ms from 0.25 s on (19 of them in 4 s)."""
    starts = ((0.25 + 0.19 * np.arange(19)) * fs).astype(np.int64)
    length = int(0.025 * fs)
    index = starts[:, None] + np.arange(length)[None, :]          # [burst][sample]: the bursts do not overlap
    carrier = np.sin(2.0 * np.pi * 6_500.0 * (index / fs))
    train = np.zeros(n, dtype=np.float64)
    train[index.ravel()] += ((1.35 * np.hanning(length))[None, :] * carrier).ravel()  # (added to silence: a window edge is +0.0, never -0.0)
    return train


def _impulse_train(n: int) -> np.ndarray:
    """+1.45 on every 997th sample, -1.35 on samples 499 mod 1553 (the negative train wins where they coincide)."""
    position = np.arange(n)
    return np.where(position % 1553 == 499, -1.35, np.where(position % 997 == 0, 1.45, 0.0))


def _clipped_two_tone_voice(n: int, fs: int) -> np.ndarray:
    """180 Hz + 2.3 kHz under a 2.1 Hz squared-sine swell, driven 25 % past full scale and hard-clipped."""
    t = _seconds(n, fs)
    tones = 0.72 * np.sin(2.0 * np.pi * 180.0 * t) + 0.46 * np.sin(2.0 * np.pi * 2_300.0 * t)
    swell = 0.45 + 0.55 * np.sin(2.0 * np.pi * 2.1 * t) ** 2
    return np.clip(tones * swell * 1.25, -1.0, 1.0)


def limiter_cases() -> dict[str, np.ndarray]:
    """The three controlled 4 s stimuli of `evaluation/limiter-lookahead-report.json` (float32)."""
    n = SAMPLE_RATE * 4
    made = {
        "controlled-sine-bursts": _hann_burst_train(n, SAMPLE_RATE),
        "controlled-impulses": _impulse_train(n),
        "controlled-clipped-voice": _clipped_two_tone_voice(n, SAMPLE_RATE),
    }
    return {name: made[name].astype(np.float32) for name in LIMITER_FIXTURE["stimuli"]}  # (the fixture's case order)


def aliasing_signal(sample_rate: int, carrier_hz: float, modulation_hz: float) -> np.ndarray:
    """One amplitude-modulated carrier of `evaluation/dynamics-aliasing-report.json`, 4 s at `sample_rate`: a squared-sine
    swell at `modulation_hz` plus a 1.5 ms exponential click every 173 ms, capped at 0.95."""
    n = int(4.0 * sample_rate)
    t = np.arange(n, dtype=np.float64) / sample_rate
    swell = 0.08 + 0.72 * np.square(0.5 + 0.5 * np.sin(2.0 * np.pi * modulation_hz * t))
    period = max(1, int(round(0.173 * sample_rate)))
    one_click = np.exp(-np.arange(period) / max(1.0, 0.0015 * sample_rate))  # the decay depends on the phase only: one period, repeated
    clicks = np.resize(one_click, n)
    level = np.clip(swell + 0.35 * clicks, 0.0, 0.95)
    return (level * np.sin(2.0 * np.pi * carrier_hz * t)).astype(np.float32)


def fingerprint_mismatch(x: np.ndarray, want: dict) -> str | None:
    """None when `x` is the stimulus `want` (a fingerprint written by tools/gen_golden.py) describes, else what differs."""
    import hashlib

    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.size != want["n"]:
        return f"length {x.size} != {want['n']}"
    if not np.array_equal(x[:64], np.asarray(want["head"], dtype=np.float32)):
        return "first 64 samples differ"
    if not np.array_equal(x[-64:], np.asarray(want["tail"], dtype=np.float32)):
        return "last 64 samples differ"
    for index, value in want["checkpoints"]:
        if x[index] != np.float32(value):
            return f"sample {index}: {x[index]!r} != {value!r}"
    if hashlib.sha256(x.astype("<f4").tobytes()).hexdigest() != want["sha256_f32le"]:
        return "SHA-256 over the float32 bytes differs"
    return None


# ------------------------------------------------------------------------------------------------------------------
# Waveform metrics of the limiter-lookahead report (`evaluation/limiter-lookahead-report.json`, "evaluation_contract"):
# this repository's vectorised forms.  tests/test_golden_fixtures.py checks them against the values the reference's own
# functions returned on the oracle's output (tests/golden/limiter_lookahead.json, "rows").
def _framed(x: np.ndarray, frame: int, hop: int) -> np.ndarray:
    return np.lib.stride_tricks.sliding_window_view(np.asarray(x, dtype=np.float64), frame)[::hop]


def gain_envelope_variation_db(reference: np.ndarray, aligned: np.ndarray) -> float:
    """Standard deviation (about the median) of the short-term gain output / input in dB: 2 ms frames at half overlap,
    frames whose input is below -40 dBFS left out."""
    frame = int(round(0.002 * SAMPLE_RATE))
    if reference.size < frame:
        return 0.0
    rms_in = np.sqrt(np.mean(np.square(_framed(reference, frame, frame // 2)), axis=1))
    rms_out = np.sqrt(np.mean(np.square(_framed(aligned[: reference.size], frame, frame // 2)), axis=1))
    audible = rms_in >= 10.0 ** (-40.0 / 20.0)
    if not audible.any():
        return 0.0
    gain_db = 20.0 * np.log10(np.maximum(rms_out[audible], 1e-12) / np.maximum(rms_in[audible], 1e-12))
    return float(np.std(gain_db - np.median(gain_db)))


def transient_indices(audio: np.ndarray, limit: int = 16) -> np.ndarray:
    """The `limit` steepest sample-to-sample steps that lie at least 6 ms apart, steepest first (ties: earliest), sorted."""
    audio = np.asarray(audio, dtype=np.float64)
    step = np.abs(np.diff(audio, prepend=0.0))
    guard = int(round(0.006 * SAMPLE_RATE))
    taken = np.zeros(audio.size, dtype=bool)   # samples closer than `guard` to a transient already picked
    picked = []
    for index in np.argsort(-step, kind="stable"):
        if taken[index]:
            continue
        picked.append(int(index))
        if len(picked) == limit:
            break
        taken[max(0, index - guard + 1) : index + guard] = True
    return np.asarray(sorted(picked), dtype=np.int64)


def transient_error_db(reference: np.ndarray, aligned: np.ndarray, indices: np.ndarray) -> float:
    """Median over the transients of the shape error in a +-4 ms window: the output minus its least-squares projection on
    the input, relative to the output, in dB (windows shorter than 8 samples are skipped; -240 dB when none is left)."""
    reference = np.asarray(reference, dtype=np.float64)
    aligned = np.asarray(aligned, dtype=np.float64)
    radius = int(round(0.004 * SAMPLE_RATE))
    floor = 1e-12
    shape_db = []
    for centre in np.asarray(indices, dtype=np.int64):
        lo, hi = max(0, int(centre) - radius), min(reference.size, int(centre) + radius + 1)
        if hi - lo < 8:
            continue
        x, y = reference[lo:hi], aligned[lo:hi]
        residual = y - (float(np.dot(x, y)) / max(float(np.dot(x, x)), floor)) * x
        rms = [float(np.sqrt(np.mean(np.square(v)))) for v in (residual, y)]
        shape_db.append(20.0 * np.log10(max(rms[0], floor) / max(rms[1], floor)))
    return float(np.median(shape_db)) if shape_db else -240.0


# Metrics of the dynamics-aliasing report (48 kHz render against a 192 kHz render brought down to 48 kHz).
def align_renders(reference: np.ndarray, candidate: np.ndarray, max_lag: int = 256) -> tuple[np.ndarray, np.ndarray, int]:
    """Shift `candidate` against `reference` by the lag (|lag| <= max_lag) of largest absolute cross-correlation over the
    first second, and cut both to their overlap."""
    probe = min(reference.size, candidate.size, SAMPLE_RATE)
    r = reference[:probe] - np.mean(reference[:probe])
    c = candidate[:probe] - np.mean(candidate[:probe])
    spectrum = np.fft.rfft(c, 2 * probe) * np.conj(np.fft.rfft(r, 2 * probe))
    xcorr = np.fft.irfft(spectrum, 2 * probe)  # xcorr[k] = sum_n c[n + k] r[n]; negative lags wrap to the end
    lags = np.arange(-max_lag, max_lag + 1)
    lag = int(lags[int(np.argmax(np.abs(xcorr[lags % (2 * probe)])))])
    if lag >= 0:
        count = min(reference.size, candidate.size - lag)
        return reference[:count], candidate[lag : lag + count], lag
    count = min(reference.size + lag, candidate.size)
    return reference[-lag : -lag + count], candidate[:count], lag


def relative_error_db(reference: np.ndarray, candidate: np.ndarray) -> float:
    rms = [float(np.sqrt(np.mean(np.square(v)))) for v in (candidate - reference, reference)]
    return float(20.0 * np.log10(max(rms[0], 1e-12) / max(rms[1], 1e-12)))


def folded_error_db(reference: np.ndarray, candidate: np.ndarray, carrier_hz: float, modulation_hz: float) -> float:
    """Energy of the (Hann-windowed) difference outside the sidebands carrier +- k x modulation, k <= 12 -- where only folded
    products can land -- relative to the reference's energy, in dB."""
    window = np.hanning(reference.size)
    frequency = np.fft.rfftfreq(reference.size, 1.0 / SAMPLE_RATE)
    centres = carrier_hz + modulation_hz * np.arange(-12, 13)
    centres = centres[(centres >= 0.0) & (centres <= SAMPLE_RATE / 2)]
    half_width = max(8.0, 0.12 * modulation_hz)
    expected = (np.abs(frequency[:, None] - centres[None, :]) <= half_width).any(axis=1)
    error_power = np.square(np.abs(np.fft.rfft((candidate - reference) * window)))
    reference_power = np.square(np.abs(np.fft.rfft(reference * window)))
    return float(10.0 * np.log10(max(float(error_power[~expected].sum()), 1e-24) / max(float(reference_power.sum()), 1e-24)))


def aliasing_case_metrics(base_output: np.ndarray, reference_output: np.ndarray, carrier_hz: float, modulation_hz: float) -> dict:
    """The waveform rows of one aliasing case from its two renders (48 kHz; 192 kHz), as the report defines them."""
    from scipy.signal import resample_poly

    down = resample_poly(np.asarray(reference_output, dtype=np.float64), 1, 4)
    reference, candidate, lag = align_renders(down, np.asarray(base_output, dtype=np.float64))
    trim = SAMPLE_RATE // 2
    if reference.size > 2 * trim:
        reference, candidate = reference[trim:-trim], candidate[trim:-trim]
    return {"alignment_lag_samples": lag, "relative_waveform_error_db": relative_error_db(reference, candidate),
            "folded_out_of_expected_error_db": folded_error_db(reference, candidate, carrier_hz, modulation_hz)}


# ------------------------------------------------------------------------------------------------------------------
# Mixed-lane stimulus for the chain kernels, whose lanes are streams: one wave holds 64 streams, and the limiter's
# division runs under a wave-wide branch (any lane over the ceiling).  Built so that waves split at the same sample.
LANE_MIX_GROUP = 64
LANE_MIX_UNDER_GROUP, LANE_MIX_OVER_GROUP = 1, 2  # group kinds by index; every other group is a mixed one


def lane_mix_kind(group: int) -> str:
    return {LANE_MIX_UNDER_GROUP: "under", LANE_MIX_OVER_GROUP: "over"}.get(group, "mixed")


def _lane_mix_roles() -> list[tuple[str, int]]:
    """The 64 lanes of a mixed group before the group's own permutation: (role, index within the role)."""
    counts = (("voiced", 37), ("loud_section", 12), ("square", 2), ("clipped", 2), ("impulses", 3), ("silent", 2),
              ("dc", 2), ("out_of_range", 2), ("non_finite", 2))
    roles = [(role, k) for role, count in counts for k in range(count)]
    assert len(roles) == LANE_MIX_GROUP
    return roles


def _edge_positions(n: int) -> np.ndarray:
    """Samples on both sides of 4-sample chunk, 480-sample control-block and 9600-sample window edges."""
    chunk = np.arange(4 * 97, n, 4 * 997)
    block = np.arange(480 * 7, n, 480 * 11)
    window = np.arange(9600, n, 9600)
    edges = np.concatenate([chunk, block, window])
    edges = np.concatenate([edges - 1, edges])
    return np.unique(edges[(edges >= 0) & (edges < n)])


def lane_mix_batch(n_streams: int, n_samples: int, seed: int = 0) -> np.ndarray:
    """[n_streams, n_samples] float32, deterministic in `seed`.  Every group of 64 streams is one of three kinds
    (`lane_mix_kind`): "mixed" groups hold voiced streams whose peak levels spread from -60 to +12 dBFS, voiced streams
    with a loud section starting at staggered offsets, full-scale squares and clipped two-tones (inter-sample overs),
    impulses at chunk / control-block / window edges, silence, DC offsets, +-4.0 samples and, in every eighth mixed group,
    NaN / +-Inf samples; in the "under" group every stream stays well under a -1.5 dBFS ceiling; in the "over" group every
    stream is loud (over the ceiling) during a span whose ends are staggered, so that the group's lanes are all under,
    some over and all over at different times.  Lanes are permuted differently in every group."""
    rng = np.random.default_rng(seed)
    n = int(n_samples)
    n_blocks = max(1, -(-n // 480))
    bases = []
    for i in range(16):  # voiced material, normalised to a peak of 1.0 (a gain in dB is then the peak level in dBFS)
        v = kat_signal(n_blocks, *stream_params(i)).astype(np.float64)[:n]
        bases.append(v / max(float(np.max(np.abs(v))), 1e-12))
    t = np.arange(n, dtype=np.float64)
    db = lambda g: 10.0 ** (np.asarray(g, dtype=np.float64) / 20.0)  # noqa: E731
    roles = _lane_mix_roles()
    edges = _edge_positions(n)
    out = np.empty((n_streams, n), dtype=np.float32)
    for g0 in range(0, n_streams, LANE_MIX_GROUP):
        group = g0 // LANE_MIX_GROUP
        kind = lane_mix_kind(group)
        lanes = min(LANE_MIX_GROUP, n_streams - g0)
        order = rng.permutation(LANE_MIX_GROUP)
        voiced_gain = rng.permutation(np.linspace(-60.0, 12.0, 37))
        offsets = rng.permutation(np.linspace(0.08, 0.72, 12)) * n + rng.integers(0, 480, 12)
        for lane in range(lanes):
            k_all = int(order[lane])
            base = bases[(k_all + 5 * group) % 16]
            if kind == "under":
                x = base * db(-60.0 + 54.0 * k_all / (LANE_MIX_GROUP - 1))  # -60 .. -6 dBFS
            elif kind == "over":
                start = (0.10 + 0.15 * k_all / LANE_MIX_GROUP) * n + 37 * k_all
                stop = (0.65 + 0.15 * ((k_all * 29) % LANE_MIX_GROUP) / LANE_MIX_GROUP) * n
                loud = (t >= start) & (t < stop)
                x = base * np.where(loud, db(6.0 + 6.0 * k_all / LANE_MIX_GROUP), db(-30.0 + 12.0 * k_all / LANE_MIX_GROUP))
            else:
                role, k = roles[k_all]
                if role == "voiced":
                    x = base * db(voiced_gain[k])
                elif role == "loud_section":
                    loud = (t >= offsets[k]) & (t < offsets[k] + n // 6)
                    x = base * np.where(loud, db(3.0 + k * 0.75), db(-24.0))
                elif role == "square":
                    x = np.where(np.sin(2.0 * np.pi * (997.0 + 2004.0 * k) * t / SAMPLE_RATE + 0.3 * group) >= 0.0, 1.0, -1.0)
                elif role == "clipped":
                    x = np.clip(0.9 * np.sin(2.0 * np.pi * (180.0 + 40.0 * k) * t / SAMPLE_RATE)
                                + 0.6 * np.sin(2.0 * np.pi * (2300.0 + 700.0 * k) * t / SAMPLE_RATE + group), -1.0, 1.0)
                elif role == "impulses":
                    x = base * db(-40.0)
                    x[edges] = np.where(np.arange(edges.size) % 2 == 0, 1.3, -0.95) * (1.0 - 0.2 * k)
                elif role == "silent":
                    x = np.zeros(n)
                elif role == "dc":
                    x = (0.5 if k == 0 else -0.95) + base * db(-26.0)
                elif role == "out_of_range":
                    x = base * db(-6.0)
                    x[(997 * (k + 1)) % 1553 :: 1553] = 4.0
                    x[(499 + 331 * k) % 2039 :: 2039] = -4.0
                else:  # non_finite
                    x = base * db(-3.0 * k)
                    if group % 8 == 0:
                        x = x.copy()
                        x[edges[k::9]] = np.nan
                        x[edges[3 + k :: 11]] = np.inf
                        x[edges[5 + k :: 13]] = -np.inf
            out[g0 + lane] = x
    return out


# ------------------------------------------------------------------------------------------------------------------
# Lane-role stimulus for the gated pre-pass (supp_prefilter_gate_kernel): every 64-stream group moves through 32-sample
# tiles, and each wave role maps rows differently (the load wave 32 rows per half-wave in batches of 16, F1 eight rows per
# half-wave, the state machine and the front end one lane per row).  Built so that the gate opens, closes and chatters on
# some rows of every eight-row octet and not on others in the same tile.
GATE_LANE_GROUP = 64
GATE_LANE_TILE = 32


def _gate_lane_roles() -> list[tuple[str, int]]:
    """The 64 lanes of a group before the group's own permutation: (role, index within the role)."""
    counts = (("flutter", 54), ("non_finite", 2), ("out_of_range", 2), ("dc", 2), ("noise", 2), ("silent", 1), ("steady", 1))
    roles = [(role, k) for role, count in counts for k in range(count)]
    assert len(roles) == GATE_LANE_GROUP
    return roles


def _gate_lane_envelope(rng: np.random.Generator, n: int, centre_db: float) -> np.ndarray:
    """Per-sample RMS level in dB: episodes of level flutter across `centre_db` (loud segments of 12-60 ms, quiet ones of
    65-140 ms that outlast the 50 ms hold, so that the 8 ms detector follows them and four transitions fall inside the
    500 ms chatter window), each followed either by a quiet gap of 0.25-0.5 s 34-55 dB under the centre (the 24 dB
    auto-relax floor's case: the relax still armed) or by a loud span.  Starts at a random point of its first episode."""
    fs = SAMPLE_RATE
    levels, lengths = [], []
    total = 0
    skip = int(rng.integers(0, int(0.4 * fs)))
    while total < n + skip:
        for i in range(int(rng.integers(6, 13))):  # the flutter (a quiet segment outlasts the 50 ms hold)
            loud = i % 2 == 0
            levels.append(centre_db + (rng.uniform(3.0, 18.0) if loud else -rng.uniform(6.0, 28.0)))
            lengths.append(int((rng.uniform(0.012, 0.06) if loud else rng.uniform(0.065, 0.14)) * fs))
        if rng.uniform() < 0.4:  # a quiet gap
            levels.append(centre_db - rng.uniform(34.0, 55.0))
            lengths.append(int(rng.uniform(0.25, 0.5) * fs))
        else:  # or a loud span
            levels.append(centre_db + rng.uniform(4.0, 20.0))
            lengths.append(int(rng.uniform(0.05, 0.4) * fs))
        total = int(np.sum(lengths))
    env = np.repeat(np.asarray(levels), np.asarray(lengths))
    return env[skip : skip + n]


def gate_lane_batch(n_streams: int, n_samples: int, seed: int = 0) -> np.ndarray:
    """[n_streams, n_samples] float32, deterministic in `seed`; a group's rows depend on (seed, group) only, so a batch's
    first streams do not depend on how many follow.  Lanes are permuted differently in every group of 64.  Most rows are
    a tone (120-900 Hz) under a level flutter around the -40 dB default threshold (a sixth of them around -60 and -20 dB,
    for the other threshold settings); a few carry NaN / +-Inf, samples beyond +-1.0 (up to +-4.0), a DC offset, white
    noise instead of the tone, digital silence, or a steady tone just over the threshold."""
    n = int(n_samples)
    t = np.arange(n, dtype=np.float64) / SAMPLE_RATE
    roles = _gate_lane_roles()
    out = np.empty((n_streams, n), dtype=np.float32)
    for g0 in range(0, n_streams, GATE_LANE_GROUP):
        group = g0 // GATE_LANE_GROUP
        rng = np.random.default_rng([int(seed), group])
        order = rng.permutation(GATE_LANE_GROUP)
        # every role's parameters are drawn for all 64 lanes, whether or not the group is complete
        params = []
        for role, k in roles:
            centre = -40.0 + rng.uniform(-2.0, 2.0)
            pick = rng.uniform()
            if role == "flutter" and pick < 1 / 12:
                centre -= 20.0
            elif role == "flutter" and pick < 1 / 6:
                centre += 20.0
            params.append(dict(centre=centre, f=rng.uniform(120.0, 900.0), phase=rng.uniform(0.0, 2.0 * np.pi),
                               env_seed=int(rng.integers(0, 2**63)), noise=rng.uniform(1e-6, 3e-5)))
        for lane in range(min(GATE_LANE_GROUP, n_streams - g0)):
            role, k = roles[int(order[lane])]
            p = params[int(order[lane])]
            r = np.random.default_rng(p["env_seed"])
            if role == "silent":
                out[g0 + lane] = 0.0
                continue
            if role == "steady":
                env = np.full(n, p["centre"] + 2.0)
            else:
                env = _gate_lane_envelope(r, n, p["centre"])
            amp = np.sqrt(2.0) * 10.0 ** (env / 20.0)
            if role == "noise":
                x = 10.0 ** (env / 20.0) * r.standard_normal(n)
            else:
                x = amp * np.sin(2.0 * np.pi * p["f"] * t + p["phase"]) + p["noise"] * r.standard_normal(n)
            if role == "dc":
                x = x + (0.3 if k == 0 else -0.6)
            elif role == "out_of_range":
                x = x.copy()
                x[int(r.integers(0, 977)) :: 977] = 4.0 if k == 0 else 1.5
                x[int(r.integers(0, 1231)) :: 1231] = -4.0 if k == 0 else -1.25
            elif role == "non_finite":
                x = x.copy()
                x[int(r.integers(0, 1409)) :: 1409] = np.nan
                x[int(r.integers(0, 2083)) :: 2083] = np.inf
                x[int(r.integers(0, 2801)) :: 2801] = -np.inf
            out[g0 + lane] = x
    return out
