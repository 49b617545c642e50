"""The production forms of the chain -- ONE token-ring launch per call following a ready counter, behind the systolic /
lane-per-stream EQ kernel (no suppressor) or behind the suppressor's pipeline -- against the oracle, on every stream of
the mixed-lane stimulus (`signals.lane_mix_batch`: waves whose lanes are over the limiter ceiling at the same sample as
lanes that are not).  Every case first asserts which form ran (kernel id, chain launches per call, launches per call).

Calls of 19 213, 24 000 and 20 411 samples: state crosses call boundaries that are not multiples of the 4-sample chunk,
the 480-sample control block or the 9600-sample EQ window, and the host path's stream stride (the call length) is
unaligned for two of the three calls.  The oracle is its block processor driven over the same calls
(tests/chain_oracle.py).  Without compressor libm in the sample path the audio must be bit-exact; with the compressor the
tolerances of tests/test_gpu_parity.py."""
import math

import numpy as np
import pytest

import chain_oracle as CO
import signals as S

pytestmark = pytest.mark.gpu

CALLS = (19_213, 24_000, 20_411)
# Auto-makeup's loudness window is 40 control blocks of block energies on the GPU, 19 200 samples in the oracle: the two
# agree only while every block is whole, so its cases run calls of whole control blocks (test_auto_makeup_ragged_calls).
ALIGNED_CALLS = (19_200, 24_000, 20_160)
SEED = 7
KERNEL_PHASED, KERNEL_STAGED = 2, 4

_STEEP_15 = list(S.DEFAULT_TYPED_BANDS)
_STEEP_15[0] = ("high_pass", 90.0, 0.0, 0.707, 48, True)      # 4 sections
_STEEP_15[9] = ("low_pass", 15000.0, 0.0, 0.707, 36, True)    # 3 sections: 15 in all (the two-wave EQ kernel splits 7 + 8)
_STEEP_15[4] = ("bell", 1000.0, 6.0, 2.0, 12, True)
_STEEP_16 = list(_STEEP_15)
_STEEP_16[9] = ("low_pass", 15000.0, 0.0, 0.707, 48, True)    # 16: the offload EQ's limit
_STEEP_17 = list(_STEEP_16)
_STEEP_17[1] = ("high_pass", 40.0, 0.0, 0.707, 24, True)      # 17: routed away from the offload EQ

_LIMITER_ONLY = dict(S.limiter_settings(2.0), compressor_enabled=False)
_AUTO_MAKEUP = dict(S.limiter_settings(2.0), compressor_auto_makeup_enabled=True, compressor_target_lufs=-16.0)
# name: (sample rate, settings, input clamp, tolerance: None = bit-exact, else (max abs, rms))
CONFIGS = {
    "limiter": (48_000, _LIMITER_ONLY, False, None),
    "compressor": (48_000, dict(S.limiter_settings(2.0), compressor_adaptive_release=True,
                                compressor_sidechain_highpass_enabled=True), False, (2e-7, 2e-8)),
    "automakeup": (48_000, _AUTO_MAKEUP, False, (5e-7, 5e-8)),
    "eq15": (48_000, dict(_LIMITER_ONLY, eq_bands_v2=_STEEP_15), False, None),
    "eq16": (48_000, dict(_LIMITER_ONLY, eq_bands_v2=_STEEP_16), False, None),
    "eq17": (48_000, dict(_LIMITER_ONLY, eq_bands_v2=_STEEP_17), False, None),
    "44k1": (44_100, _LIMITER_ONLY, False, None),
    "clamp": (48_000, _LIMITER_ONLY, True, None),
}
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name, (max_abs, rms, streams, first) in sorted(REPORT.items()):
        where = "" if first is None else f", first sample out of bounds {first}"
        print(f"chain-forms {name}: {streams} streams, worst max abs {max_abs:.3e}, worst rms {rms:.3e}{where}")


_AUDIO, _ORACLE = {}, {}


def _calls(config):
    return ALIGNED_CALLS if config == "automakeup" else CALLS


def _audio(n_streams):
    if n_streams not in _AUDIO:
        _AUDIO[n_streams] = S.lane_mix_batch(n_streams, sum(CALLS), SEED)
    return _AUDIO[n_streams]


def _oracle(config, n_streams, calls=None):
    """The oracle over the stimulus itself (no suppressor), once per module."""
    calls = calls or _calls(config)
    key = (config, n_streams, calls)
    if key not in _ORACLE:
        fs, settings, clamp, _ = CONFIGS[config]
        _ORACLE[key] = CO.run_batch(_audio(n_streams), fs, S.LIMITER_BANDS, settings, calls, clamp)
    return _ORACLE[key]


def _engine(n_streams, config, pinned, suppressor=False, chain=True):
    from mic_eq_mi import _lib
    from mic_eq_mi import mic_eq_core as core

    fs, settings, clamp, _ = CONFIGS[config]
    eng = core.Engine(float(fs), n_streams)
    if pinned:
        eng.set_kernel(_lib.KERNEL_PHASED)
        eng.set_ring_variant(16, 4)
    else:
        eng.set_kernel(_lib.KERNEL_AUTO)
        eng.set_ring_variant(0, 0)
    if chain:
        core.configure_auto_eq_chain(eng, float(fs), S.LIMITER_BANDS, settings)
    else:
        eng.set_eq_enabled(0)
        eng.set_compressor_enabled(0)
        eng.set_limiter_enabled(0)
        eng.set_control_block_samples(CO.control_block(fs))
    if clamp:
        eng.set_input_clamp_enabled(1)
    if suppressor:
        eng.set_prefilter_enabled(1, 1)
        eng.set_suppressor_enabled(1)
        eng.suppressor_set_trace_enabled(1)
    eng.set_timing_enabled(1)
    return eng


def _form(eng):
    return eng.last_kernel(), eng.last_chain_launch_ms()[2], eng.last_kernel_ms()[1]


def _run(eng, audio, device_stride_pad=None, calls=CALLS):
    """`calls` through `eng`: (output, rows [blocks, streams], forms per call, suppressor traces per call, samples each
    call returned)."""
    outs, rows, forms, traces, lengths = [], [], [], [], []
    at = 0
    for n in calls:
        x = audio[:, at : at + n]
        at += n
        if device_stride_pad is None:
            y = eng.process(x)
        else:  # device pointers through torch, rows `n + pad` apart
            import torch

            stride = n + device_stride_pad
            xin = torch.zeros((x.shape[0], stride), dtype=torch.float32, device="cuda")
            xin[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            yout = torch.full_like(xin, 7.0)
            eng.process_device(xin.data_ptr(), yout.data_ptr(), n, stride, 0, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert bool((yout[:, n:] == 7.0).all()), "the engine wrote past a row's samples"
            y = yout[:, :n].cpu().numpy()
        outs.append(y)
        lengths.append(y.shape[1])
        rows.append(eng.block_stats().copy())
        forms.append(_form(eng))
        traces.append(eng.suppressor_trace().copy())
    return np.concatenate(outs, axis=1), np.concatenate(rows, axis=0), forms, traces, lengths


def _eq_launches(n, fs):
    cb = CO.control_block(fs)
    window = cb * max(1, 9600 // cb)
    return 1 + 2 * math.ceil(n / window)  # the chain launch + per EQ window the EQ kernel and the counter's publish


def _assert_one_launch_behind_eq(forms, fs, calls=CALLS):
    for n, (kernel, chain, launches) in zip(calls, forms):
        assert (kernel, chain, launches) == (KERNEL_PHASED, 1, _eq_launches(n, fs)), (n, kernel, chain, launches)


def _assert_one_launch_behind_suppressor(forms):
    for kernel, chain, launches in forms:
        assert kernel == KERNEL_PHASED and chain == 1 and launches > 7, (kernel, chain, launches)


def _compare(name, config, got, got_rows, want, want_rows):
    tol = CONFIGS[config][3]
    assert got.shape == want.shape and got_rows.shape == want_rows.shape, (got.shape, want.shape, got_rows.shape, want_rows.shape)
    d = got.astype(np.float64) - want.astype(np.float64)
    max_abs = np.abs(d).max(axis=1)
    rms = np.sqrt(np.mean(d * d, axis=1))
    off = np.abs(d) > (tol[0] if tol else 0.0)
    first = int(np.argmax(off.any(axis=0))) if off.any() else None  # (the first sample where some stream is out of bounds)
    REPORT[name] = (float(max_abs.max()), float(rms.max()), got.shape[0], first)
    if tol is None:
        differ = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
        assert differ.size == 0, f"{name}: {differ.size} streams differ from the oracle (first {differ[:8].tolist()}, max abs " \
                                 f"{max_abs[differ].max():.3e})"
    else:
        bad = np.flatnonzero((max_abs > tol[0]) | (rms > tol[1]))
        assert bad.size == 0, f"{name}: streams {bad[:8].tolist()} exceed {tol}: max abs {max_abs.max():.3e}, rms {rms.max():.3e}"
    exact_events = tol is None
    for field in CO.ROW_FIELDS:
        a, b = got_rows[field], want_rows[field]
        if field == "true_peak_limited_events":
            if exact_events:
                where = np.argwhere(a.astype(np.uint64) != b)
                assert where.size == 0, f"{name}: true-peak events differ in {len(where)} rows (block, stream) {where[:4].tolist()}"
            continue
        a, b = a.astype(np.float64), b.astype(np.float64)
        rel = 2e-5 if exact_events else 1e-4
        err = np.abs(a - b) - rel * np.maximum(1.0, np.abs(b))
        where = np.argwhere(err > 0.0)
        assert where.size == 0, f"{name}: row field {field} differs in {len(where)} rows, first (block, stream) {where[:4].tolist()}"


# ----------------------------------------------------------------------------------------------------- no suppressor
@pytest.mark.parametrize("config", list(CONFIGS))
def test_one_launch_behind_eq_pinned(config):
    """ring-16x4 pinned, 130 streams (two groups and a group of 2 lanes + 62 padded ones)."""
    fs = CONFIGS[config][0]
    eng = _engine(130, config, pinned=True)
    try:
        got, rows, forms, _, _ = _run(eng, _audio(130), calls=_calls(config))
    finally:
        eng.close()
    if config == "eq17":  # more sections than the offload EQ takes: the EQ runs inside the one chain launch
        assert all(f == (KERNEL_PHASED, 1, 1) for f in forms), forms
    else:
        _assert_one_launch_behind_eq(forms, fs, _calls(config))
    want, want_rows = _oracle(config, 130)
    _compare(f"ring-16x4/130/{config}", config, got, rows, want, want_rows)
    if config == "automakeup":
        makeup = rows["compressor_makeup_gain_db"]
        assert float(np.abs(makeup).max()) > 1.0, "the auto-makeup gain never moved"


def test_one_launch_behind_eq_auto_large_batch():
    """AUTO at 3136 streams (past the stage pipeline's 3072): the production form without the suppressor."""
    n_streams = 3136
    eng = _engine(n_streams, "limiter", pinned=False)
    try:
        got, rows, forms, _, _ = _run(eng, _audio(n_streams))
    finally:
        eng.close()
    _assert_one_launch_behind_eq(forms, 48_000)
    want, want_rows = CO.run_batch(_audio(n_streams), 48_000, S.LIMITER_BANDS, _LIMITER_ONLY, CALLS)
    _compare(f"auto/{n_streams}/limiter", "limiter", got, rows, want, want_rows)


def test_stage_pipeline_auto_small_batch():
    eng = _engine(130, "limiter", pinned=False)
    try:
        got, rows, forms, _, _ = _run(eng, _audio(130))
    finally:
        eng.close()
    assert all(f[0] == KERNEL_STAGED and f[1] > 1 for f in forms), forms  # (a launch step per stage window)
    want, want_rows = _oracle("limiter", 130)
    _compare("auto/130/limiter (stage pipeline)", "limiter", got, rows, want, want_rows)


def test_one_launch_behind_eq_device_pointers_unaligned_stride():
    """process_device with rows n + 3 apart: the lane-per-stream EQ kernel does not take unaligned rows and the systolic
    kernel runs instead (af_eq_systolic.hip, launch_eq_systolic); nothing is written between the rows."""
    eng = _engine(130, "limiter", pinned=True)
    try:
        got, rows, forms, _, _ = _run(eng, _audio(130), device_stride_pad=3)
    finally:
        eng.close()
    _assert_one_launch_behind_eq(forms, 48_000)
    want, want_rows = _oracle("limiter", 130)
    _compare("ring-16x4/130/limiter (device, stride n+3)", "limiter", got, rows, want, want_rows)


@pytest.mark.xfail(strict=True, reason="auto-makeup's loudness window on the GPU is the last 40 control blocks' energies, which "
                                       "is the oracle's 19 200-sample window only while every block is whole; a call whose "
                                       "length is not a multiple of the control block ends in a short block")
def test_auto_makeup_ragged_calls():
    eng = _engine(130, "automakeup", pinned=True)
    try:
        got, rows, forms, _, _ = _run(eng, _audio(130))
    finally:
        eng.close()
    _assert_one_launch_behind_eq(forms, 48_000)
    want, want_rows = _oracle("automakeup", 130, CALLS)
    _compare("ring-16x4/130/automakeup (ragged calls)", "automakeup", got, rows, want, want_rows)


# --------------------------------------------------------------------------------------------- behind the suppressor
def _behind_suppressor(name, n_streams, config, pinned):
    audio = _audio(n_streams)
    front = _engine(n_streams, config, pinned, suppressor=True, chain=False)
    try:
        supp_out, _, _, supp_traces, lengths = _run(front, audio)
    finally:
        front.close()
    eng = _engine(n_streams, config, pinned, suppressor=True)
    try:
        got, rows, forms, traces, got_lengths = _run(eng, audio)
    finally:
        eng.close()
    assert got_lengths == lengths == [19_200, 24_000, 20_160], (got_lengths, lengths)
    for a, b in zip(traces, supp_traces):  # the same suppressor decisions: the chain's input is `supp_out` exactly
        assert a.shape == b.shape and np.array_equal(a, b)
    _assert_one_launch_behind_suppressor(forms)
    fs, settings, _, _ = CONFIGS[config]
    want, want_rows = CO.run_batch(supp_out, fs, S.LIMITER_BANDS, settings, lengths)
    _compare(name, config, got, rows, want, want_rows)


@pytest.mark.parametrize("config", ["limiter", "compressor"])
def test_one_launch_behind_suppressor_pinned(config):
    _behind_suppressor(f"suppressor+ring-16x4/130/{config}", 130, config, pinned=True)


def test_one_launch_behind_suppressor_auto_large_batch():
    """AUTO at 2112 streams (past the stage pipeline's 2048 behind the suppressor)."""
    _behind_suppressor("suppressor+auto/2112/limiter", 2112, "limiter", pinned=False)
