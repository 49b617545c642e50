"""Live control (af_engine_set_live_control): chain setters called between process calls against the oracle's block
processor retuned the same way (tests/retune_oracle.py), on every kernel family.

67 streams (one full wave and a ragged one of 3 lanes), 48 kHz, the loud per-stream KAT voices of
tests/live_control_cases.py -- the oracle's rows show the compressor, the limiter and the true-peak limiter reducing gain
in every block, so a silent chain cannot pass -- in calls of 960, 50, 30, 480, 7, 1000, 960 samples: the 72-sample
crossfade scheduled before call 1 is still running at the next boundary (22 samples left) and ends inside call 2, one call
has 7 samples, and the calls are no multiples of the 960-sample control block.  Tolerances are those of the existing parity
tests of each path: 2e-7 / 2e-8 (max abs / rms) behind the compressor (tests/test_gpu_parity.py), 5e-7 / 5e-8 with the
de-esser (tests/test_gpu_deesser.py), rms and worst sample 1e-5 behind the suppressor (tests/test_gpu_suppressor.py);
the block rows as tests/test_gpu_chain_forms.py compares them."""
import ctypes as C

import numpy as np
import pytest

import chain_oracle as CO
import live_control_cases as LC
import retune_oracle as RO

pytestmark = pytest.mark.gpu

COMP_TOL = (2e-7, 2e-8)
DEESSER_TOL = (5e-7, 5e-8)
KERNELS = {"auto": 0, "lane": 1, "phased": 2, "quad": 3, "staged": 4}
STATE_MESSAGE = "setter called after streaming started; call af_engine_reset first"
N_STREAMS = 67


def _engine(n_streams, kernel, live, deesser=None, suppressor=False, presets=None):
    from mic_eq_mi import mic_eq_core as core

    eng = core.Engine(float(LC.FS), n_streams)
    eng.set_kernel(KERNELS[kernel])
    eng.set_ring_variant(*((16, 4) if kernel == "phased" else (0, 0)))
    n_presets = max(presets) + 1 if presets else 1  # `presets`: the preset of each 64-stream group
    if presets:
        eng.set_preset_count(n_presets)
    for k in range(n_presets):
        if presets:
            eng.select_preset(k)
        core.configure_auto_eq_chain(eng, float(LC.FS), LC.BANDS, LC.SETTINGS)
        if deesser is not None:
            eng.set_deesser_enabled(1)
            eng.set_eq_before_deesser(int(deesser["eq_first"]))
            for name, args in deesser["setters"]:
                RO.apply_to_engine(eng, name, args)
    if presets:
        gp = np.asarray(presets, dtype=np.int32)
        core._lib.check(eng._lib.af_engine_assign_presets(eng._h, gp.ctypes.data_as(C.POINTER(C.c_int32)), len(presets)))
    if suppressor:
        eng.set_suppressor_enabled(1)
    if live is not None:
        eng.set_live_control(live)
    return eng


def _run(eng, audio, calls, schedule=None, preset=None):
    """`calls` through `eng`, the schedule's setters applied before their call: (output, rows [blocks, streams], launches
    per call, pending edits seen before each call)."""
    outs, rows, launches, pending = [], [], [], []
    at = 0
    for index, n in enumerate(calls):
        if preset is not None:
            eng.select_preset(preset)
        for name, args in (schedule or {}).get(index, ()):
            RO.apply_to_engine(eng, name, args)
        pending.append(eng.live_control_pending())
        outs.append(eng.process(audio[:, at : at + n]))
        at += n
        rows.append(eng.block_stats().copy())
        launches.append(eng.last_kernel_ms()[1])
    return np.concatenate(outs, axis=1), np.concatenate(rows, axis=0), launches, pending


def _compare(name, got, got_rows, want, want_rows, tol, deesser=False):
    assert got.shape == want.shape and got_rows.shape == want_rows.shape, (got.shape, want.shape, got_rows.shape, want_rows.shape)
    d = got.astype(np.float64) - want.astype(np.float64)
    max_abs = np.abs(d).max(axis=1)
    rms = np.sqrt(np.mean(d * d, axis=1))
    off = np.abs(d) > tol[0]
    first = int(np.argmax(off.any(axis=0))) if off.any() else None
    print(f"live-control {name}: worst max abs {max_abs.max():.3e}, worst rms {rms.max():.3e}, first sample out of bounds {first}")
    bad = np.flatnonzero((max_abs > tol[0]) | (rms > tol[1]))
    assert bad.size == 0, f"{name}: streams {bad[:8].tolist()} exceed {tol}: max abs {max_abs.max():.3e}, rms {rms.max():.3e}, first sample {first}"
    for field in CO.ROW_FIELDS + (("deesser_gain_reduction_db",) if deesser else ()):
        if field == "true_peak_limited_events":
            continue  # (a count of threshold crossings: exact only where the audio is, tests/test_gpu_chain_forms.py)
        a, b = got_rows[field].astype(np.float64), want_rows[field].astype(np.float64)
        err = np.abs(a - b) - 1e-4 * np.maximum(1.0, np.abs(b))
        where = np.argwhere(err > 0.0)
        assert where.size == 0, f"{name}: row field {field} differs in {len(where)} rows, first (block, stream) {where[:4].tolist()}"


_ORACLE = {}


def _oracle(key, n_streams, schedule, deesser=None, skip=LC.SKIP):
    if key not in _ORACLE:
        _ORACLE[key] = RO.run_batch(LC.audio(n_streams, skip=skip), LC.FS, LC.BANDS, LC.SETTINGS, LC.CALLS, schedule, deesser=deesser)
    return _ORACLE[key]


# ------------------------------------------------------------------------------------------------ 1. every kernel family
@pytest.mark.parametrize("kernel", ["lane", "phased", "quad", "staged", "auto"])
def test_schedule_on_every_kernel(kernel):
    want, want_rows = _oracle("main", N_STREAMS, LC.SCHEDULE)
    LC.assert_loud(want_rows)
    eng = _engine(N_STREAMS, kernel, live=True)
    try:
        got, rows, launches, pending = _run(eng, LC.audio(N_STREAMS), LC.CALLS, LC.SCHEDULE)
        used = eng.last_kernel()
    finally:
        eng.close()
    if kernel != "auto":
        assert used == KERNELS[kernel], used
    # calls 1-5 have setters pending (several setters of one boundary: one list), call 6 and call 0 none; the limiter's
    # and the ratio's are parameters only, so call 4 carries no state edit
    assert [p > 0 for p in pending] == [False, True, True, True, False, True, False], pending
    _compare(f"schedule/{kernel}", got, rows, want, want_rows, COMP_TOL)
    # the retune is heard: the same engine without the schedule is the unretuned oracle, far outside the tolerance
    plain, _ = _oracle("plain", N_STREAMS, None)
    assert float(np.abs(want.astype(np.float64) - plain).max()) > 1e-3


def test_forty_calls_each_behind_a_retune():
    """Forty calls of one control block, one EQ band's gain changed before each (before the first the engine has not started:
    that setter is configuration, the other 39 are live edits): every later call uploads the edit list and the parameter block
    of the crossfade it starts, so the 32 pinned staging slots are all used more than once."""
    calls = (960,) * 40
    schedule = {k: [("eq_set_band_gain", (3, 6.0 if k % 2 else -4.0 + 0.125 * k))] for k in range(40)}
    audio = LC.audio(N_STREAMS, n=sum(calls))
    want, want_rows = RO.run_batch(audio, LC.FS, LC.BANDS, LC.SETTINGS, calls, schedule)
    eng = _engine(N_STREAMS, "auto", live=True)
    try:
        got, rows, launches, pending = _run(eng, audio, calls, schedule)
    finally:
        eng.close()
    assert [p > 0 for p in pending] == [False] + [True] * 39, pending
    _compare("forty retunes", got, rows, want, want_rows, COMP_TOL)


# ------------------------------------------------------------------------------------------------ 2. the de-esser
_DEESSER_FORMS = [(False, "lane"), (False, "staged"), (True, "phased")]


def _deesser_run(eq_first, kernel, schedule, key):
    deesser = {"eq_first": eq_first, "setters": LC.DEESSER_SETTERS}
    want, want_rows = _oracle((key, eq_first), N_STREAMS, schedule, deesser, LC.SIBILANT_SKIP)
    LC.assert_loud(want_rows, true_peak_streams=60)
    assert float(want_rows["deesser_gain_reduction_db"].min()) > 0.5  # every stream is de-essed in every block
    eng = _engine(N_STREAMS, kernel, live=True, deesser=deesser)
    try:
        got, rows, _, _ = _run(eng, LC.audio(N_STREAMS, skip=LC.SIBILANT_SKIP), LC.CALLS, schedule)
        used = eng.last_kernel()
    finally:
        eng.close()
    assert used == KERNELS[kernel], used
    _compare(f"deesser/{key}/{'eq-first' if eq_first else 'default'}/{kernel}", got, rows, want, want_rows, DEESSER_TOL, deesser=True)


@pytest.mark.parametrize("eq_first,kernel", _DEESSER_FORMS)
def test_deesser_scalar_retune(eq_first, kernel):
    """The chain's schedule with the de-esser on, plus the de-esser's threshold, ratio, max reduction and auto amount."""
    _deesser_run(eq_first, kernel, LC.merged(LC.SCHEDULE, LC.DEESSER_SCALARS), "scalars")


@pytest.mark.parametrize("eq_first,kernel", _DEESSER_FORMS)
def test_deesser_cut_frequency_retune(eq_first, kernel):
    """... plus the cut frequencies before call 1: a crossfade on the nine de-esser filters, the dynamic EQs' from each stream's
    live coefficients to the new centre / Q at that stream's momentary gain (deesser.rs:64-73, 536-538)."""
    _deesser_run(eq_first, kernel, LC.merged(LC.SCHEDULE, LC.DEESSER_SCALARS, LC.DEESSER_CUTS), "cuts")


HELD_CALLS = (15_360, 200, 960)
HELD_SKIP = 23 * 480  # a sibilant burst in the first call; at its end the de-essing has decayed to ~0.1 dB


@pytest.mark.parametrize("kernel", ["lane", "staged"])
def test_deesser_cut_frequency_retune_while_the_gain_is_held(kernel):
    """The cut frequencies move while every stream's dynamic EQs sit at a small gain of their own that moves slowly (0.09-0.13 dB
    of de-essing, decaying by 4e-5 dB per sample: the 0.001 dB hold keeps the gain, and with it the crossfade, for some 25
    samples at a time).  The crossfade then runs from each stream's live coefficients towards the new centre and Q AT THAT
    STREAM'S GAIN; in the burst of the other cases the gain moves at every sample and cancels it at once."""
    deesser = {"eq_first": False, "setters": LC.DEESSER_SETTERS}
    audio = LC.audio(N_STREAMS, n=sum(HELD_CALLS), skip=HELD_SKIP)
    want, want_rows = RO.run_batch(audio, LC.FS, LC.BANDS, LC.SETTINGS, HELD_CALLS, LC.DEESSER_CUTS, deesser=deesser)
    plain, _ = RO.run_batch(audio, LC.FS, LC.BANDS, LC.SETTINGS, HELD_CALLS, None, deesser=deesser)
    boundary = want_rows["deesser_gain_reduction_db"][15:17]  # the last block of call 0, the block of call 1
    assert 0.05 < float(boundary.min()) and float(boundary.max()) < 0.2, (boundary.min(), boundary.max())
    heard = np.abs(want.astype(np.float64) - plain)[:, HELD_CALLS[0] : HELD_CALLS[0] + HELD_CALLS[1]].max(axis=1)
    assert float(heard.min()) > 10 * DEESSER_TOL[0], float(heard.min())  # the retune is heard inside the crossfade, on every stream
    eng = _engine(N_STREAMS, kernel, live=True, deesser=deesser)
    try:
        got, rows, _, _ = _run(eng, audio, HELD_CALLS, LC.DEESSER_CUTS)
        used = eng.last_kernel()
    finally:
        eng.close()
    assert used == KERNELS[kernel], used
    _compare(f"deesser/held/{kernel}", got, rows, want, want_rows, DEESSER_TOL, deesser=True)


# ------------------------------------------------------------------------------------------------ 3. behind the suppressor
SUPP_CALLS = (1000, 500, 1900, 480)          # what goes in; 960, 480, 1920, 480 come out (whole 480-sample frames)
SUPP_SCHEDULE = {
    1: [("eq_set_band_gain", (3, 6.0)), ("compressor_set_threshold", (-16.0,)), ("compressor_set_ratio", (3.0,))],
    2: [("eq_set_band_config", (7, ("notch", 4021.2060546875, 0.0, 2.0, 12, True))), ("compressor_set_release_time", (120.0,)),
        ("compressor_set_makeup_gain", (15.0,))],
}


@pytest.mark.parametrize("kernel", ["phased", "auto"])
def test_behind_the_suppressor(oracle, kernel):
    """Synthetic weights as in tests/test_gpu_suppressor.py.  The oracle chain runs on the oracle suppressor's output, retuned
    at the first sample the chain sees in each call.  Pinned, the token-ring kernel runs as ONE launch per call behind the
    systolic EQ."""
    audio = LC.audio(N_STREAMS, sum(SUPP_CALLS))
    lengths, pending = [], 0
    for n in SUPP_CALLS:
        lengths.append((pending + n) // 480 * 480)
        pending = pending + n - lengths[-1]
    assert lengths == [960, 480, 1920, 480]
    sup = np.stack([oracle.suppressor_process(audio[s], 1.0, 0x5EED) for s in range(N_STREAMS)])[:, : sum(lengths)]
    want, want_rows = RO.run_batch(sup, LC.FS, LC.BANDS, LC.SETTINGS, lengths, SUPP_SCHEDULE)
    plain, _ = RO.run_batch(sup, LC.FS, LC.BANDS, LC.SETTINGS, lengths, None)
    # the suppressor's output starts with its one-frame fade-in: the limiter works in every block, the compressor from the
    # third block on (every block behind the second retune)
    assert float(want_rows["limiter_peak_gain_reduction_db"].min()) > 0.0 and float(want_rows["compressor_gain_reduction_db"][2:].min()) > 0.0
    eng = _engine(N_STREAMS, kernel, live=True, suppressor=True)
    try:
        got, rows, _, _ = _run(eng, audio, SUPP_CALLS, SUPP_SCHEDULE)
        used = eng.last_kernel()
    finally:
        eng.close()
    assert got.shape == want.shape
    if kernel == "phased":
        assert used == KERNELS["phased"]
    d = got.astype(np.float64) - want.astype(np.float64)
    rms, worst = float(np.sqrt(np.mean(d * d))), float(np.abs(d).max())
    print(f"live-control suppressor/{kernel}: kernel {used}, rms {rms:.3e}, worst sample {worst:.3e}")
    assert rms <= 1e-5 and worst <= 1e-5, (rms, worst)
    assert float(np.abs(want.astype(np.float64) - plain).max()) > 1e-3  # (the unretuned chain is far outside that)
    assert np.abs(rows["compressor_gain_reduction_db"].astype(np.float64) - want_rows["compressor_gain_reduction_db"]).max() <= 1e-3


# ------------------------------------------------------------------------------------------------ 4. presets
def test_only_the_addressed_preset_is_retuned():
    """130 streams (groups of 64, 64 and 2), two presets assigned [0, 1, 0]; preset 1 is retuned."""
    n_streams, groups = 130, [0, 1, 0]
    audio = LC.audio(n_streams)
    want, want_rows = _oracle("main130", n_streams, LC.SCHEDULE)
    LC.assert_loud(want_rows)
    eng = _engine(n_streams, "phased", live=True, presets=groups)
    other = _engine(n_streams, "phased", live=True, presets=groups)
    try:
        got, rows, _, _ = _run(eng, audio, LC.CALLS, LC.SCHEDULE, preset=1)
        base, base_rows, _, _ = _run(other, audio, LC.CALLS)
    finally:
        eng.close()
        other.close()
    untouched = np.r_[0:64, 128:130]
    retuned = np.r_[64:128]
    assert np.array_equal(got[untouched].view(np.uint32), base[untouched].view(np.uint32))
    for field in rows.dtype.names:
        assert rows[field][:, untouched].tobytes() == base_rows[field][:, untouched].tobytes(), field
    _compare("presets/retuned", got[retuned], rows[:, retuned], want[retuned], want_rows[:, retuned], COMP_TOL)
    assert float(np.abs(got[retuned].astype(np.float64) - base[retuned]).max()) > 1e-3


# ------------------------------------------------------------------------------------------------ 5. the switch off
@pytest.mark.parametrize("live", [None, False])
def test_switch_off_refuses_as_before(live):
    audio = LC.audio(N_STREAMS)
    eng = _engine(N_STREAMS, "auto", live=live)
    try:
        eng.process(audio[:, :960])
        for name, args in [item for items in LC.SCHEDULE.values() for item in items] + LC.DEESSER_SETTERS:
            with pytest.raises(RuntimeError) as info:
                RO.apply_to_engine(eng, name, args)
            assert str(info.value) == STATE_MESSAGE, (name, str(info.value))
        with pytest.raises(RuntimeError, match="af_engine_reset"):
            eng.set_live_control(True)  # the switch is a configuration setter itself
        assert eng.live_control_pending() == 0
    finally:
        eng.close()


@pytest.mark.parametrize("kernel", ["auto", "phased", "lane"])
def test_switch_on_without_setters_changes_nothing(kernel):
    audio = LC.audio(N_STREAMS)
    runs = []
    for live in (False, True):
        eng = _engine(N_STREAMS, kernel, live=live)
        try:
            runs.append(_run(eng, audio, LC.CALLS))
        finally:
            eng.close()
    (off, off_rows, off_launches, _), (on, on_rows, on_launches, on_pending) = runs
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
    assert on_rows.tobytes() == off_rows.tobytes()
    assert on_launches == off_launches and min(off_launches) >= 1, (on_launches, off_launches)
    assert on_pending == [0] * len(LC.CALLS)


def test_a_retune_costs_one_launch_and_only_when_something_is_pending():
    audio = LC.audio(N_STREAMS)
    plain = _engine(N_STREAMS, "phased", live=True)
    tuned = _engine(N_STREAMS, "phased", live=True)
    try:
        _, _, base, _ = _run(plain, audio, LC.CALLS)
        _, _, launches, pending = _run(tuned, audio, LC.CALLS, LC.SCHEDULE)
    finally:
        plain.close()
        tuned.close()
    extra = [a - b for a, b in zip(launches, base)]
    assert extra == [1 if p else 0 for p in pending], (launches, base, pending)


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_stream_alone_and_reset_returns_to_configuration():
    from mic_eq_mi import _lib

    audio = LC.audio(N_STREAMS)
    want, want_rows = _oracle("plain", N_STREAMS, None)
    eng = _engine(N_STREAMS, "auto", live=True)
    fresh = _engine(N_STREAMS, "auto", live=True)
    try:
        first = eng.process(audio[:, :960])
        first_rows = eng.block_stats().copy()
        # configuration setters: they change which kernels, stages or buffers are resident
        for call in (lambda: eng.limiter_set_lookahead_ms(1.0), lambda: eng.set_compressor_enabled(0), lambda: eng.set_deesser_enabled(1),
                     lambda: eng.set_eq_before_deesser(1), lambda: eng.compressor_set_auto_makeup_enabled(1),
                     lambda: eng.set_control_block_samples(480), lambda: eng.eq_reset(), lambda: eng.set_live_control(False)):
            with pytest.raises(RuntimeError, match="configuration setter.*af_engine_reset"):
                call()
            assert eng.live_control_pending() == 0
        # arguments are validated before anything is recorded: the message is EqBandConfig::validate's
        bad = _lib.EqBandConfig(1, 30_000.0, 0.0, 1.0, 12, 1)
        assert eng._lib.af_eq_band_config_validate(C.byref(bad), 3, float(LC.FS)) == _lib.AF_ERR_INVALID_ARGUMENT
        message = _lib.last_error()
        assert "out of range" in message
        with pytest.raises(ValueError) as info:
            eng.eq_set_band_frequency(3, 30_000.0)
        assert str(info.value) == message
        for call in (lambda: eng.eq_set_band_gain(3, float("nan")), lambda: eng.eq_set_band_q(3, 0.0), lambda: eng.eq_set_band_gain(10, 1.0),
                     lambda: eng.eq_set_band_config_tuple(3, ("bell", 100.0, 40.0, 1.0, 12, True))):
            with pytest.raises(ValueError):
                call()
        # what cannot be patched in place
        with pytest.raises(NotImplementedError, match="sections"):
            eng.eq_set_band_config_tuple(0, ("high_pass", 90.0, 0.0, 0.707, 48, True))
        assert eng.live_control_pending() == 0
        rest, rest_rows, _, _ = _run(eng, audio[:, 960:], LC.CALLS[1:])
        got, rows = np.concatenate([first, rest], axis=1), np.concatenate([first_rows, rest_rows], axis=0)
        _compare("refusals", got, rows, want, want_rows, COMP_TOL)
        # reset: configuration mode again, the switch kept, and the same stream as a fresh engine
        eng.reset()
        eng.limiter_set_lookahead_ms(2.0)
        eng.set_compressor_enabled(1)
        again, again_rows, _, _ = _run(eng, audio, LC.CALLS, LC.SCHEDULE)
        new, new_rows, _, _ = _run(fresh, audio, LC.CALLS, LC.SCHEDULE)
        assert np.array_equal(again.view(np.uint32), new.view(np.uint32))
        assert again_rows.tobytes() == new_rows.tobytes()
    finally:
        eng.close()
        fresh.close()
