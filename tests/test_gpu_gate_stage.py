"""The noise gate as a stateful stage of the engine's realtime chain (dsp_loop.rs:1371-1435): front end -> gate ->
suppressor -> dynamics chain, against the oracle composed per stream (prefilter -> Gate -> suppressor_process ->
simulate_auto_eq_chain), with gate state carried across calls."""
import numpy as np
import pytest

import gate_oracle as GO
import signals as S

pytestmark = pytest.mark.gpu
FS = 48_000.0


@pytest.fixture(scope="module")
def core():
    import mic_eq_mi
    from mic_eq_mi import mic_eq_core

    assert mic_eq_mi.CORE_AVAILABLE, "HIP library missing: GPU tests never fall back to the CPU"
    return mic_eq_core


def gate_signal(n_streams: int, n: int, seed: int = 7) -> np.ndarray:
    """Speech-level tone bursts, pauses and a level flutter around -40 dB (200 ms period: the gate opens and closes four
    times inside the 500 ms chatter window).  Every stream is shifted and scaled differently."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    out = np.empty((n_streams, n), dtype=np.float32)
    for s in range(n_streams):
        f = 150.0 + 13.0 * (s % 17)
        tone = np.sin(2 * np.pi * f * t + 0.3 * s) + 0.3 * np.sin(2 * np.pi * 2.7 * f * t)
        ts = (t + 0.037 * s) % 2.0
        env = np.where(ts < 0.4, 0.25, 0.0008)                                    # talk, then a pause
        flutter = np.where(((ts - 0.8) % 0.2) < 0.1, 0.05, 0.003)                  # -30 / -54 dB flutter
        env = np.where((ts >= 0.8) & (ts < 1.6), flutter, env)
        env = env * (0.7 + 0.06 * (s % 9))
        out[s] = (env * tone + 1e-4 * rng.standard_normal(n)).astype(np.float32)
    return out


def oracle_gate(oracle, x, vad_mode=False):
    g = oracle.Gate(vad_mode=vad_mode)
    return g.process(x), g


def check_all_states(eng, want):
    """Every stream's gate state against the batched oracle's (tests/gate_oracle.py)."""
    st = eng.gate_state()
    gain = np.abs(st["current_gain"].astype(np.float64) - want["current_gain"].astype(np.float64))
    assert gain.max() <= 1e-6, (int(np.argmax(gain)), gain.max())
    for field in ("chatter_events", "is_open", "auto_relax_active"):
        assert np.array_equal(st[field], want[field]), (field, np.flatnonzero(st[field] != want[field])[:8])
    return st


def check_state(eng, gates, streams):
    st = eng.gate_state()
    for s, g in zip(streams, gates):
        assert abs(float(st["current_gain"][s]) - g.current_gain) <= 1e-6, (s, st["current_gain"][s], g.current_gain)
        assert int(st["chatter_events"][s]) == g.chatter_event_count, s
        assert bool(st["is_open"][s]) == g.is_open, s
        assert bool(st["auto_relax_active"][s]) == (g.s.auto_relax_remaining_samples > 0), s
    return st


@pytest.mark.parametrize("kernel", [0, 2])
def test_full_realtime_chain_with_the_gate(core, oracle, kernel):
    n_streams, frames_a, frames_b = 70, 130, 110
    n = (frames_a + frames_b) * 480 + 500
    x = gate_signal(n_streams, n)
    settings = S.limiter_settings(2.0)
    eng = core.Engine(FS, n_streams)
    core.configure_auto_eq_chain(eng, FS, S.LIMITER_BANDS, settings)
    eng.set_prefilter_enabled(1, 1)
    eng.set_suppressor_enabled(1)
    eng.set_kernel(kernel)
    eng.set_gate_enabled(1)
    a = eng.process(x[:, : frames_a * 480])
    b = eng.process(x[:, frames_a * 480 :])
    used = eng.last_kernel()
    got = np.concatenate([a, b], axis=1)
    assert got.shape[1] == (n // 480) * 480
    assert used == (4 if kernel == 0 else 2)
    m = got.shape[1]
    gates = []
    for s in (0, 1, 63, 64, 69):
        gated, g = oracle_gate(oracle, oracle.prefilter(x[s, :m]))
        gates.append(g)
        want = oracle.simulate_auto_eq_chain(oracle.suppressor_process(gated, 1.0), FS, S.LIMITER_BANDS,
                                             settings)["output_audio"]
        d = got[s].astype(np.float64) - np.asarray(want, dtype=np.float64)
        rms = float(np.sqrt(np.mean(d * d)))
        assert rms <= 1e-5, (s, rms)
    st = check_state(eng, gates, (0, 1, 63, 64, 69))
    eng.close()
    assert any(g.chatter_event_count > 0 for g in gates), "the stimulus never made the gate chatter"
    assert float(st["current_gain"].min()) < 0.5 or not all(st["is_open"])
    # every stream, through the batched oracle
    want, want_st = GO.run_batch(x, FS, (frames_a * 480, n - frames_a * 480), suppressor="wrapper",
                                 chain=(S.LIMITER_BANDS, settings))
    d = got.astype(np.float64) - want.astype(np.float64)
    rms, worst = np.sqrt(np.mean(d * d, axis=1)), np.abs(d).max(axis=1)
    print(f"gate stage + suppressor, kernel {kernel}: {n_streams} streams, worst rms {rms.max():.3e}, worst {worst.max():.3e}")
    assert rms.max() <= 1e-5, (int(np.argmax(rms)), rms.max())
    assert np.array_equal(st["chatter_events"], want_st["chatter_events"])
    assert np.abs(st["current_gain"].astype(np.float64) - want_st["current_gain"]).max() <= 1e-6
    assert np.array_equal(st["is_open"], want_st["is_open"])


def _dyn_engine(core, n_streams, kernel=0, presets=1):
    settings = S.limiter_settings(2.0)
    eng = core.Engine(FS, n_streams)
    if presets > 1:
        eng.set_preset_count(presets)
        for p in range(presets):
            eng.select_preset(p)
            core.configure_auto_eq_chain(eng, FS, S.LIMITER_BANDS, settings)
    else:
        core.configure_auto_eq_chain(eng, FS, S.LIMITER_BANDS, settings)
    eng.set_prefilter_enabled(1, 1)
    eng.set_kernel(kernel)
    eng.set_gate_enabled(1)
    return eng, settings


@pytest.mark.parametrize("kernel", [0, 1, 2, 3, 4])
def test_gate_without_the_suppressor(core, oracle, kernel):
    n_streams = 70
    x = gate_signal(n_streams, 48_000 + 333, seed=3)
    eng, settings = _dyn_engine(core, n_streams, kernel)
    got = np.concatenate([eng.process(x[:, :20_000]), eng.process(x[:, 20_000:])], axis=1)
    rows = eng.block_stats()
    gates = []
    worst = 0.0
    for s in (0, 1, 63, 64, 69):
        gated, g = oracle_gate(oracle, oracle.prefilter(x[s]))
        gates.append(g)
        want = oracle.simulate_auto_eq_chain(gated, FS, S.LIMITER_BANDS, settings)["output_audio"]
        worst = max(worst, float(np.max(np.abs(got[s].astype(np.float64) - np.asarray(want, dtype=np.float64)))))
        # the block input statistics describe the chain's input, the gated signal (control blocks of 960, per call)
        tail = gated[20_000:].astype(np.float64)
        blocks = -(-tail.size // 960)
        want_sq = np.array([np.sum(tail[b * 960 : (b + 1) * 960] ** 2) for b in range(blocks)])
        raw_sq = np.array([np.sum(x[s, 20_000:][b * 960 : (b + 1) * 960].astype(np.float64) ** 2) for b in range(blocks)])
        assert rows.shape[0] == blocks
        assert np.allclose(rows["input_square_sum"][:, s], want_sq, rtol=1e-5, atol=1e-12), s
        assert not np.allclose(want_sq, raw_sq, rtol=1e-2), "the gate never acted on this stream"
    check_state(eng, gates, (0, 1, 63, 64, 69))
    # every stream, through the batched oracle
    want, want_st = GO.run_batch(x, FS, (20_000, x.shape[1] - 20_000), chain=(S.LIMITER_BANDS, settings))
    check_all_states(eng, want_st)
    eng.close()
    every = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
    print(f"gate stage, kernel {kernel}: {n_streams} streams, worst max abs {every:.3e}")
    assert worst <= 1e-6, (kernel, worst)
    assert every <= 1e-6, (kernel, every)


def test_gate_without_the_suppressor_with_the_deesser(core, oracle):
    n_streams = 70
    n = 38_400
    t = np.arange(n) / FS
    # the golden KAT voice (it has sibilance the de-esser reduces), with pauses that close the gate
    x = np.stack([S.kat_signal(n // 480, *S.stream_params(s)) * np.where(((t + 0.05 * s) % 0.8) < 0.5, 1.0, 0.002)
                  for s in range(n_streams)]).astype(np.float32)
    settings = dict(S.limiter_settings(2.0), deesser_enabled=True, deesser_auto_amount=0.85, deesser_max_reduction_db=10.0)
    eng = core.Engine(FS, n_streams)
    core.configure_auto_eq_chain(eng, FS, S.LIMITER_BANDS, settings)
    eng.set_prefilter_enabled(1, 1)
    eng.set_gate_enabled(1)
    got = np.concatenate([eng.process(x[:, :19_200]), eng.process(x[:, 19_200:])], axis=1)
    rows = eng.block_stats()
    eng.close()
    assert float(rows["deesser_gain_reduction_db"].max()) > 0.5, "the de-esser never acted"
    for s in range(n_streams):
        gated, _ = oracle_gate(oracle, oracle.prefilter(x[s]))
        want = oracle.simulate_auto_eq_chain(gated, FS, S.LIMITER_BANDS, dict(settings))["output_audio"]
        assert float(np.max(np.abs(got[s].astype(np.float64) - np.asarray(want, dtype=np.float64)))) <= 1e-6, s


def test_gate_without_the_suppressor_two_presets(core, oracle):
    n_streams = 128
    x = gate_signal(n_streams, 30_000, seed=5)
    eng, settings = _dyn_engine(core, n_streams, 0, presets=2)
    got = eng.process(x)
    eng.close()
    for s in range(n_streams):
        gated, _ = oracle_gate(oracle, oracle.prefilter(x[s]))
        want = oracle.simulate_auto_eq_chain(gated, FS, S.LIMITER_BANDS, settings)["output_audio"]
        assert float(np.max(np.abs(got[s].astype(np.float64) - np.asarray(want, dtype=np.float64)))) <= 1e-6, s


def test_state_across_calls_is_bit_identical(core):
    n_streams, n = 4096, 96_000
    base = gate_signal(128, n, seed=11)  # 128 different streams, tiled and scaled per stream
    x = (np.tile(base, (n_streams // 128, 1)) * np.linspace(0.6, 1.4, n_streams, dtype=np.float32)[:, None]).astype(np.float32)
    del base

    def run(cuts, suppressor=False):
        eng = core.Engine(FS, n_streams)
        eng.set_prefilter_enabled(1, 1)
        eng.set_gate_enabled(1)
        if suppressor:
            eng.set_suppressor_enabled(1)
        parts, at = [], 0
        for c in list(cuts) + [n]:
            parts.append(eng.process(x[:, at:c]))
            at = c
        st = eng.gate_state()
        eng.close()
        return np.concatenate(parts, axis=1), st

    cuts = np.cumsum([1, 63, 64, 65, 4799])
    one, st1 = run([])
    split, st2 = run(cuts)
    assert np.array_equal(one, split)
    assert np.array_equal(st1["current_gain"], st2["current_gain"])
    assert np.array_equal(st1["chatter_events"], st2["chatter_events"])
    one_s, _ = run([], suppressor=True)
    split_s, _ = run(cuts, suppressor=True)
    assert np.array_equal(one_s, split_s)


def _tp_free_err(got, want):
    return float(np.max(np.abs(got.astype(np.float64) - np.asarray(want, dtype=np.float64))))


def _gate_only(core, n_streams):
    """The gate in front of the configured dynamics chain, no front end, no suppressor."""
    eng = core.Engine(FS, n_streams)
    core.configure_auto_eq_chain(eng, FS, S.LIMITER_BANDS, S.limiter_settings(2.0))
    eng.set_gate_enabled(1)
    return eng


def _chain(oracle, gated):
    return oracle.simulate_auto_eq_chain(gated, FS, S.LIMITER_BANDS, S.limiter_settings(2.0))["output_audio"]


def _coeff(ms):
    return float(np.exp(-1.0 / ((ms / 1000.0) * FS)))


def test_live_parameter_changes_match_the_oracle(core, oracle):
    n_streams, n1 = 65, 40_320
    x = gate_signal(n_streams, 2 * n1, seed=13)
    eng = _gate_only(core, n_streams)
    a = eng.process(x[:, :n1])
    eng.gate_set_threshold(-35.0)
    eng.gate_set_attack_time(3.0)
    eng.gate_set_release_time(250.0)
    b = eng.process(x[:, n1:])
    eng.close()
    for s in range(n_streams):
        g = oracle.Gate()
        first = g.process(x[s, :n1])
        g.s.threshold_db = -35.0
        g.s.attack_coeff = _coeff(3.0)
        g.s.release_coeff = _coeff(250.0)
        want = _chain(oracle, np.concatenate([first, g.process(x[s, n1:])]))
        assert _tp_free_err(np.concatenate([a[s], b[s]]), want) <= 1e-6, s


def relax_signal(n_streams: int, n: int) -> np.ndarray:
    """Per 2 s: 0.8 s of level flutter around the threshold (a chatter event arms the 700 ms auto-relax), then near
    silence (~ -95 dB, more than 32 dB under the threshold) while the relax counter still runs."""
    t = np.arange(n) / FS
    out = np.empty((n_streams, n), dtype=np.float32)
    rng = np.random.default_rng(31)
    for s in range(n_streams):
        ts = (t + 0.011 * s) % 2.0
        env = np.where(ts < 0.8, np.where((ts % 0.2) < 0.1, 0.05, 0.003), 2e-5)
        out[s] = (env * np.sin(2 * np.pi * (170.0 + 9.0 * s) * t) + 1e-5 * rng.standard_normal(n)).astype(np.float32)
    return out


@pytest.mark.parametrize("mode", [0, 1])
def test_modes_and_the_auto_relax_floor(core, oracle, mode):
    """The first call ends at 0.95 s, in stream 0's near silence while its auto-relax (armed by the chatter event of the
    flutter) still runs: there mode 1's target is the 24 dB floor and mode 0's the 36 dB one, so the gains differ by far
    more than the 1e-6 the device is held to."""
    n_streams, n1 = 64, 45_600
    x = relax_signal(n_streams, 144_000)
    eng = _gate_only(core, n_streams)
    eng.gate_set_mode(mode)
    a = eng.process(x[:, :n1])
    gates = [oracle.Gate(vad_mode=mode != 0) for _ in range(n_streams)]  # every stream
    firsts = [g.process(x[s, :n1]) for g, s in zip(gates, range(n_streams))]
    st = check_state(eng, gates, range(n_streams))
    other = oracle.Gate(vad_mode=mode == 0)
    other.process(x[0, :n1])
    assert (gates[0].s.auto_relax_remaining_samples > 0) == (mode == 1)
    assert abs(gates[0].current_gain - other.current_gain) > 1e-2, "the 24 dB floor was not reached with the relax armed"
    if mode == 1:
        assert st["auto_relax_active"][0] and st["current_gain"][0] > 10 ** (-24.5 / 20)
    else:
        assert not st["auto_relax_active"].any()
    b = eng.process(x[:, n1:])
    for g, first, s in zip(gates, firsts, range(n_streams)):
        want = _chain(oracle, np.concatenate([first, g.process(x[s, n1:])]))
        assert _tp_free_err(np.concatenate([a[s], b[s]]), want) <= 1e-6, s
    st = check_state(eng, gates, range(n_streams))
    assert st["chatter_events"].max() > 1
    eng.close()


def test_mode_zero_clears_the_auto_relax_at_once(core, oracle):
    import ctypes as C

    n_streams, n1 = 64, 45_600  # the first call ends 0.15 s after the flutter: the relax is armed
    x = relax_signal(n_streams, 2 * n1)
    eng = _gate_only(core, n_streams)
    eng.gate_set_mode(1)
    a = eng.process(x[:, :n1])
    assert eng.gate_state()["auto_relax_active"][0]
    eng.gate_set_mode(0)
    assert not eng.gate_state()["auto_relax_active"].any()
    b = eng.process(x[:, n1:])
    eng.close()
    g = oracle.Gate(vad_mode=True)
    first = g.process(x[0, :n1])
    oracle.lib().afo_gate_set_vad_mode(C.byref(g.s), 0)
    want = _chain(oracle, np.concatenate([first, g.process(x[0, n1:])]))
    assert _tp_free_err(np.concatenate([a[0], b[0]]), want) <= 1e-6


def test_disable_freezes_and_reset_restores(core, oracle):
    n_streams, n = 64, 28_800
    x = gate_signal(n_streams, 3 * n, seed=19)
    eng = _gate_only(core, n_streams)
    a = eng.process(x[:, :n])
    eng.set_gate_enabled(0)
    b = eng.process(x[:, n : 2 * n])
    eng.set_gate_enabled(1)
    c = eng.process(x[:, 2 * n :])
    for s in range(n_streams):
        g = oracle.Gate()
        gated = np.concatenate([g.process(x[s, :n]), x[s, n : 2 * n], g.process(x[s, 2 * n :])])  # skipped in the middle
        want = _chain(oracle, gated)
        assert _tp_free_err(np.concatenate([a[s], b[s], c[s]]), want) <= 1e-6, s
    eng.reset()
    after = eng.process(x[:, :n])
    st = eng.gate_state()
    eng.close()
    fresh = _gate_only(core, n_streams)
    first = fresh.process(x[:, :n])
    st_f = fresh.gate_state()
    fresh.close()
    assert np.array_equal(after, first)
    assert np.array_equal(st["current_gain"], st_f["current_gain"])


def test_disable_with_the_front_end_on_the_stage_pipeline(core, oracle):
    """AUTO at 70 streams takes the stage pipeline, chosen at the first call with the gate on (the front end in the
    pre-pass).  The disabled call must still get the DC block and the high-pass: prefilter -> chain for that call."""
    n_streams, n = 70, 19_200
    x = gate_signal(n_streams, 3 * n, seed=37)
    eng, settings = _dyn_engine(core, n_streams, 0)
    a = eng.process(x[:, :n])
    assert eng.last_kernel() == 4
    eng.set_gate_enabled(0)
    b = eng.process(x[:, n : 2 * n])
    eng.set_gate_enabled(1)
    c = eng.process(x[:, 2 * n :])
    eng.close()
    for s in range(n_streams):
        pre = oracle.prefilter(x[s])
        g = oracle.Gate()
        gated = np.concatenate([g.process(pre[:n]), pre[n : 2 * n], g.process(pre[2 * n :])])
        want = oracle.simulate_auto_eq_chain(gated, FS, S.LIMITER_BANDS, settings)["output_audio"]
        assert _tp_free_err(np.concatenate([a[s], b[s], c[s]]), want) <= 1e-6, s


def test_gate_off_is_untouched(core):
    n_streams = 70
    x = gate_signal(n_streams, 110 * 480, seed=23)
    settings = S.limiter_settings(2.0)

    def run(touch):
        eng = core.Engine(FS, n_streams)
        core.configure_auto_eq_chain(eng, FS, S.LIMITER_BANDS, settings)
        eng.set_prefilter_enabled(1, 1)
        eng.set_suppressor_enabled(1)
        eng.set_kernel(2)
        if touch:
            eng.gate_set_threshold(-20.0)
            eng.gate_set_attack_time(1.0)
            eng.gate_set_release_time(20.0)
            eng.gate_set_mode(1)
            eng.set_gate_enabled(1)
            eng.set_gate_enabled(0)
        out = eng.process(x)
        eng.close()
        return out

    assert np.array_equal(run(False), run(True))


def test_time_major_with_the_gate_is_refused(core):
    eng = core.Engine(FS, 4)
    eng.set_gate_enabled(1)
    with pytest.raises(NotImplementedError, match="gate"):
        eng.process(np.zeros((480, 4), np.float32), layout=1)
    eng.close()
