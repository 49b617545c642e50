"""The VAD-fused gate modes on the device, through the C ABI, against the restatement (tests/vad_gate_oracle.py): the
reference's eleven gate tests (gate.rs:1109-1295) run on the engine -- the eleventh, a pure function in the reference, through
the gain it asks for --, and the committed stimulus (tests/vad_gate_stimulus.py)
over 70 streams, two unequal calls with state carried, per-stream evidence, with and without the suppressor and the chain.
Tolerances are the project's existing ones: gated audio <= 2e-7 abs, current_gain <= 1e-6, RMS <= 1e-5 behind the suppressor
and the chain; fused score and smoothed probability <= 1e-6; discrete results equal (a stream may leave the discrete
comparison only if the restatement reports an rms_db within 1e-4 dB of a bin edge or of the level threshold: compute_rms_db
ends in an f32 log10, and the device's and the host's may differ in the last bit)."""
import numpy as np
import pytest

import gate_oracle as GO
import signals as S
import vad_gate_oracle as V
import vad_gate_stimulus as ST

pytestmark = pytest.mark.gpu
FS = ST.FS
F32 = np.float32


@pytest.fixture(scope="module")
def core():
    import mic_eq_mi
    from mic_eq_mi import mic_eq_core

    assert mic_eq_mi.CORE_AVAILABLE, "HIP library missing: GPU tests never fall back to the CPU"
    return mic_eq_core


def bare_engine(core, n_streams, block, *, prefilter=False, kernel=0, suppressor=False, chain=None):
    eng = core.Engine(FS, n_streams)
    if chain is None:
        eng.set_eq_enabled(0)
        eng.set_compressor_enabled(0)
        eng.set_limiter_enabled(0)
    else:
        core.configure_auto_eq_chain(eng, FS, *chain)
    eng.set_prefilter_enabled(int(prefilter), int(prefilter))
    eng.set_control_block_samples(block)
    if suppressor:
        eng.set_suppressor_enabled(1)
    eng.set_kernel(kernel)
    eng.set_gate_enabled(1)
    return eng


def apply(eng, p, ctl):
    eng.gate_set_threshold(p["threshold_db"])
    eng.gate_set_attack_time(p["attack_ms"])
    eng.gate_set_release_time(p["release_ms"])
    eng.gate_set_mode(p["mode"])
    eng.gate_set_vad_auto_gate_enabled(int(ctl is not None))
    if ctl is not None:
        eng.gate_set_vad_threshold(ctl["vad_threshold"])
        eng.gate_set_hold_time(ctl["hold_ms"])
        eng.gate_set_margin(ctl["margin_db"])
        eng.gate_set_auto_threshold(int(ctl["auto_threshold"]))


def amp_db(db):
    return F32(np.power(F32(10.0), F32(db) / F32(20.0), dtype=np.float32))


# ---- the eleven reference tests: (attack, release, vad_threshold, mode, hold or None, [(probability, available, block)])
def _blk(v, n):
    return np.full(n, v, dtype=np.float32)


def _click():
    c = _blk(0.0, 512)
    c[0] = 0.8
    return c


REFERENCE_CASES = {
    "assisted_uses_level_when_unavailable": (1.0, 20.0, 0.5, 1, None, [(0.0, False, _blk(0.1, 3000))],
                                             lambda r: r["gain"] > 0.5),
    "only_closes_when_unavailable": (1.0, 20.0, 0.5, 2, None, [(0.0, False, _blk(0.1, 3000))], lambda r: r["gain"] < 0.2),
    "assisted_opens_for_strong_evidence": (1.0, 20.0, 0.5, 1, None, [(0.9, True, _blk(0.1, 3000))],
                                           lambda r: r["score"] >= V.FUSED_GATE_OPEN_SCORE and r["gain"] > 0.5),
    "assisted_vad_open_below_level_threshold": (1.0, 20.0, 0.4, 1, None, [(0.45, True, _blk(amp_db(-42.0), 3000))],
                                                lambda r: r["gain"] > 0.35),
    "only_honors_vad_threshold": (1.0, 20.0, 0.4, 2, None, [(0.45, True, _blk(0.1, 3000))], lambda r: r["gain"] > 0.5),
    "assisted_resists_weak_noise": (1.0, 20.0, 0.5, 1, None, [(0.1, True, _blk(0.0005, 3000))],
                                    lambda r: r["score"] <= V.FUSED_GATE_CLOSE_SCORE and r["gain"] < 0.3),
    "opens_on_rising_probability": (1.0, 20.0, 0.5, 1, 0.0, [(0.42, True, _blk(amp_db(-46.0), 2000))],
                                    lambda r: r["state"] == V.OPEN and r["gain"] > 0.25),
    "preserves_ambiguous_trailing_speech": (1.0, 20.0, 0.5, 1, 0.0,
                                            [(0.90, True, _blk(0.08, 2000)), (0.41, True, _blk(amp_db(-45.0), 2000))],
                                            lambda r: r["state"] != V.CLOSED and r["gain"] > r["gains"][0] * 0.45),
    "rejects_short_click": (1.0, 20.0, 0.5, 1, 0.0, [(0.05, True, _click())], lambda r: r["state"] == V.CLOSED and r["gain"] < 0.2),
    # (the reference builds this gate with a 5 ms release; the engine's live control clamps the release to [10, 1000] ms as the
    # realtime processor does, audio/processor.rs:77-82, so the device form runs the shortest release the ABI can set)
    "chatter_triggers_auto_relax": (1.0, 10.0, 0.5, 2, 0.0,
                                    [(0.95, True, _blk(0.1, 256)), (0.0, True, _blk(0.0, 256))] * 5,
                                    lambda r: r["events"] > 0 and r["relax"]),
}


@pytest.mark.parametrize("name", sorted(REFERENCE_CASES))
def test_reference_gate_tests_on_the_device(core, name):
    attack, release, vad_threshold, mode, hold, steps, verdict = REFERENCE_CASES[name]
    n_streams, block = 3, steps[0][2].size
    eng = bare_engine(core, n_streams, block)
    ctl = dict(V.DEFAULT_CONTROLLER, vad_threshold=vad_threshold, hold_ms=200.0 if hold is None else hold)
    apply(eng, dict(threshold_db=-40.0, attack_ms=attack, release_ms=release, mode=mode), ctl)
    g = V.VadGate(-40.0, attack, release, FS)
    g.set_vad_auto_gate(vad_threshold)
    g.set_gate_mode(mode)
    if hold is not None:
        g.set_hold_time(hold)
    gains = []
    for prob, avail, buf in steps:
        eng.gate_set_vad_evidence(np.array([prob], np.float32), np.array([avail]))
        got = eng.process(np.tile(buf, (n_streams, 1)))
        g.set_external_vad_probability(prob, avail)
        want = g.process_block_inplace(buf.copy())
        step_st, step_vs, step_want = eng.gate_state(), eng.gate_vad_state(), g.report()
        gains.append(float(step_st["current_gain"][0]))
        where = (name, len(gains), gains[-1], step_want.current_gain, int(step_vs["gate_state"][0]), step_want.gate_state,
                 bool(step_vs["held_open"][0]), step_want.held_open, bool(step_st["auto_relax_active"][0]),
                 step_want.auto_relax_active, float(step_vs["probability"][0]), step_want.vad_smoothed_probability)
        assert abs(gains[-1] - step_want.current_gain) <= 1e-6, where  # (a block of zeros does not show its gain in the audio)
        assert int(step_vs["gate_state"][0]) == step_want.gate_state, where
        assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2e-7, where
    st, vs = eng.gate_state(), eng.gate_vad_state()
    eng.close()
    r = dict(gain=float(st["current_gain"][1]), gains=gains, score=F32(vs["fused_score"][1]), state=int(vs["gate_state"][1]),
             events=int(st["chatter_events"][1]), relax=bool(st["auto_relax_active"][1]))
    print(name, r)
    assert verdict(r), r
    want = g.report()
    assert abs(r["gain"] - want.current_gain) <= 1e-6 and r["state"] == want.gate_state
    assert abs(float(r["score"]) - want.fused_gate_score) <= 1e-6
    assert abs(float(vs["probability"][2]) - want.vad_smoothed_probability) <= 1e-6
    assert r["events"] == want.chatter_event_count and r["relax"] == bool(want.auto_relax_active)
    assert bool(vs["held_open"][0]) == bool(want.held_open) and vs["noise_floor_db"][0] == F32(want.noise_floor)


def test_continuous_reduction_on_the_device(core):
    """gate.rs:1280-1295 through its effect.  The reference evaluates continuous_vad_gain_reduction_db(VadOnly, p, available,
    not held, 0.5) at p = 0.10 / 0.40 / 0.90: monotone, zero at 0.90, at most 36 dB x 0.45 at 0.10.  On the engine the function
    is only reachable through the gain it asks for: after one block of speech (p = 0.95) the hold time keeps the fused gate
    open for 200 ms while six 25 ms blocks carry the posterior p; the level is high throughout, so the posterior reduction
    alone sets the target (held with p >= 0.3 caps the closure at 0.8, which at p = 0.40, closure 0.5, does not bind)."""
    finals = {}
    for q in (0.10, 0.40, 0.90):
        eng = bare_engine(core, 2, 1200)
        apply(eng, dict(threshold_db=-40.0, attack_ms=1.0, release_ms=20.0, mode=2), dict(V.DEFAULT_CONTROLLER, vad_threshold=0.5))
        g = V.VadGate(-40.0, 1.0, 20.0, FS)
        g.set_vad_auto_gate(0.5)
        g.set_gate_mode(2)
        for p in (0.95,) + (q,) * 6:
            eng.gate_set_vad_evidence(np.array([p], np.float32), np.array([True]))
            got = eng.process(np.tile(_blk(0.1, 1200), (2, 1)))
            g.set_external_vad_probability(p, True)
            want = g.process_block_inplace(_blk(0.1, 1200))
            assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2e-7
        st, vs, r = eng.gate_state(), eng.gate_vad_state(), g.report()
        eng.close()
        assert vs["held_open"].all() and r.held_open and int(vs["gate_state"][0]) == r.gate_state == V.OPEN
        assert abs(float(st["current_gain"][0]) - r.current_gain) <= 1e-6
        finals[q] = float(st["current_gain"][1])
    print("continuous reduction, gains:", finals)
    low, uncertain, high = finals[0.10], finals[0.40], finals[0.90]
    assert low < uncertain < high                  # the reduction is monotone in the posterior
    assert abs(high - 1.0) < 1.0e-6                # and zero at the speech end
    assert low >= V.db_to_linear(-V.EXPANDER_RANGE_DB * V.VAD_ONLY_CONTINUOUS_SCALE) - 1e-6


def compare(eng, got, want, want_st, label, *, audio_tol=None, rms_tol=None):
    st, vs = eng.gate_state(), eng.gate_vad_state()
    d = got.astype(np.float64) - want.astype(np.float64)
    worst, rms = np.abs(d).max(axis=1), np.sqrt(np.mean(d * d, axis=1))
    out = ST.excluded(want_st)
    keep = ~out
    print(f"{label}: worst abs {worst.max():.3e}, worst rms {rms.max():.3e}, {int(out.sum())} of {out.size} streams left out "
          f"of the discrete comparison")
    assert out.sum() <= ST.EDGE_CAP * out.size
    # continuous results: every stream
    if audio_tol is not None:
        assert worst.max() <= audio_tol, (int(np.argmax(worst)), worst.max())
    if rms_tol is not None:
        assert rms.max() <= rms_tol, (int(np.argmax(rms)), rms.max())
    for key, src in (("current_gain", st), ("fused_score", vs), ("probability", vs)):
        e = np.abs(src[key].astype(np.float64) - want_st[key].astype(np.float64))
        assert e.max() <= 1e-6, (key, int(np.argmax(e)), e.max())
    # discrete results: every stream the restatement does not report at an edge
    for key, ref, src in (("chatter_events", "chatter_events", st), ("is_open", "is_open", st),
                          ("auto_relax_active", "auto_relax_active", st), ("gate_state", "gate_state", vs),
                          ("held_open", "held_open", vs)):
        a, b = np.asarray(src[key])[keep], np.asarray(want_st[ref])[keep]
        assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), (key, np.flatnonzero(a != b)[:8])
    # the noise floor is a sum of slews towards bin centres: the same bins in the same order give the same f32
    assert np.array_equal(vs["noise_floor_db"][keep], want_st["noise_floor_db"][keep].astype(np.float32))
    rel = np.abs(vs["noise_floor_reliability"].astype(np.float64) - want_st["noise_floor_reliability"].astype(np.float64))[keep]
    assert rel.max() <= 1e-6
    # every block of the last call: the held-open decision and the noise floor (hence its histogram bin) behind it
    want_held = np.asarray(want_st["block_held_open"]).T
    dec = eng.gate_vad_decisions(want_held.shape[0])
    assert np.array_equal(dec["held_open"][:, keep], want_held[:, keep]), np.argwhere(dec["held_open"] != want_held)[:8]
    assert np.array_equal(dec["noise_floor_db"][:, keep], np.asarray(want_st["block_noise_floor"], dtype=np.float32).T[:, keep])
    return keep


def run_engine(eng, x, calls, ev):
    outs, at = [], 0
    for c, e in zip(calls, ev):
        if e is not None:
            eng.gate_set_vad_evidence(e[0], e[1])
        outs.append(eng.process(x[:, at : at + c]))
        at += c
    return np.concatenate(outs, axis=1)


@pytest.mark.parametrize("config,kernel", [("assisted_auto_hold200", 0), ("only_manual_hold0", 2), ("assisted_auto_hold0", 2),
                                           ("only_auto_hold200", 0)])
def test_fused_gate_without_the_suppressor(core, config, kernel):
    mode, ctl = ST.CONFIGS[config]
    x, ev = ST.audio(), ST.evidence()
    eng = bare_engine(core, ST.N_STREAMS, ST.BLOCK, prefilter=True, kernel=kernel)
    apply(eng, ST.gate_params(mode), ctl)
    got = run_engine(eng, x, ST.CALLS, ev)
    want, want_st = V.run_batch(x, FS, ST.CALLS, ST.gate_params(mode), ctl, ev, ST.BLOCK)
    keep = compare(eng, got, want, want_st, f"fused gate {config} kernel {kernel}", audio_tol=2e-7)
    assert keep[[63, 64, 69]].all()
    # af_engine_reset, then the same input: the same output bit for bit
    eng.reset()
    apply(eng, ST.gate_params(mode), ctl)
    again = run_engine(eng, x, ST.CALLS, ev)
    eng.close()
    assert np.array_equal(got, again)


def test_ten_calls_of_growing_evidence(core):
    """Ten calls, each one control block longer than the one before (2 .. 11 blocks of evidence per stream): every call's
    evidence is larger than any staged before it, so the staging slots are reallocated call after call.  Then ten calls of
    two blocks, which fit: the eight slots are reused in turn."""
    mode, ctl = ST.CONFIGS["assisted_auto_hold200"]
    calls = tuple(ST.BLOCK * k + 250 for k in range(1, 11)) + (ST.BLOCK + 250,) * 10  # (each ends inside a control block)
    x = ST.audio(n=sum(calls))
    ev = ST.evidence(calls=calls)
    assert [e[0].shape[0] for e in ev] == list(range(2, 12)) + [2] * 10
    eng = bare_engine(core, ST.N_STREAMS, ST.BLOCK, prefilter=True)
    apply(eng, ST.gate_params(mode), ctl)
    got = run_engine(eng, x, calls, ev)
    want, want_st = V.run_batch(x, FS, calls, ST.gate_params(mode), ctl, ev, ST.BLOCK)
    compare(eng, got, want, want_st, "fused gate, ten calls of growing evidence", audio_tol=2e-7)
    eng.close()


@pytest.mark.parametrize("config,kernel", [("assisted_auto_hold0", 0), ("only_auto_hold200", 2)])
def test_fused_gate_behind_the_suppressor(core, config, kernel):
    mode, ctl = ST.CONFIGS[config]
    calls = (48_000 + 250, 36_000 + 333)  # 25 frames hold 24 control blocks of 500: windows of whole blocks
    x = ST.audio(n=sum(calls))
    out_calls = GO.output_calls(calls, "wrapper")
    ev = ST.evidence(calls=out_calls)
    eng = bare_engine(core, ST.N_STREAMS, ST.BLOCK, prefilter=True, kernel=kernel, suppressor=True)
    apply(eng, ST.gate_params(mode), ctl)
    got = run_engine(eng, x, calls, ev)
    want, want_st = V.run_batch(x, FS, calls, ST.gate_params(mode), ctl, ev, ST.BLOCK, suppressor="wrapper")
    compare(eng, got, want, want_st, f"fused gate + suppressor {config} kernel {kernel}", rms_tol=1e-5)
    eng.close()


def test_fused_gate_with_the_dynamics_chain(core):
    mode, ctl = ST.CONFIGS["assisted_auto_hold200"]
    calls = (30_000, 18_500)
    x = ST.audio(n=sum(calls))
    ev = ST.evidence(calls=calls)
    chain = (S.LIMITER_BANDS, S.limiter_settings(2.0))
    eng = bare_engine(core, ST.N_STREAMS, ST.BLOCK, prefilter=True, chain=chain)
    apply(eng, ST.gate_params(mode), ctl)
    got = run_engine(eng, x, calls, ev)
    want, want_st = V.run_batch(x, FS, calls, ST.gate_params(mode), ctl, ev, ST.BLOCK, chain=chain)
    compare(eng, got, want, want_st, "fused gate + dynamics chain", rms_tol=1e-5)
    eng.close()


def test_mode_changes_and_reattach_between_calls(core):
    """1 -> 0 -> 2 across calls, then a detach and a re-attach (a fresh controller): state carried as the reference carries it."""
    calls = (20_000, 15_000, 20_500, 12_000, 18_000)
    x = ST.audio(n=sum(calls))
    ev = ST.evidence(calls=calls)
    ctl = dict(V.DEFAULT_CONTROLLER, hold_ms=40.0)
    modes = (1, 0, 2, 2, 1)
    ctls = (ctl, ctl, ctl, None, ctl)
    params = [ST.gate_params(m) for m in modes]
    eng = bare_engine(core, ST.N_STREAMS, ST.BLOCK, prefilter=True)
    outs, at = [], 0
    for c, p, cc, e in zip(calls, params, ctls, ev):
        apply(eng, p, cc)
        if p["mode"] != 0 and cc is not None:
            eng.gate_set_vad_evidence(e[0], e[1])
        outs.append(eng.process(x[:, at : at + c]))
        at += c
    got = np.concatenate(outs, axis=1)
    want, want_st = V.run_batch(x, FS, calls, params, list(ctls), ev, ST.BLOCK)
    compare(eng, got, want, want_st, "mode changes and re-attach", audio_tol=2e-7)
    eng.close()


@pytest.mark.parametrize("mode,attached", [(0, True), (1, False), (2, False)])
def test_unfused_combinations_are_the_parent_path(core, mode, attached):
    """Controller attached with mode 0, or detached with mode 1 / 2: the expander path, as before this feature."""
    calls = (20_000, 13_333)
    x = ST.audio(n=sum(calls))
    eng = bare_engine(core, ST.N_STREAMS, ST.BLOCK, prefilter=True)
    p = ST.gate_params(mode)
    apply(eng, p, dict(V.DEFAULT_CONTROLLER) if attached else None)
    got = run_engine(eng, x, calls, [None, None])
    want, want_st = GO.run_batch(x, FS, calls, p)
    st, vs = eng.gate_state(), eng.gate_vad_state()
    eng.close()
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2e-7
    assert np.abs(st["current_gain"].astype(np.float64) - want_st["current_gain"]).max() <= 1e-6
    for key in ("chatter_events", "is_open", "auto_relax_active"):
        assert np.array_equal(st[key], want_st[key]), key
    assert (vs["gate_state"] == 0).all() and (vs["noise_floor_db"] == F32(-60.0)).all()


def test_evidence_of_the_wrong_length_is_refused_before_anything_is_touched(core):
    """Like the auto-makeup evidence: the refused call leaves af_engine_pending_input and the gate as they were, and the
    stream continues as if the call had not been made."""
    n_streams = 4
    x = ST.audio(n_streams=n_streams, n=3 * 480 + 500)
    ctl = dict(V.DEFAULT_CONTROLLER)
    eng = bare_engine(core, n_streams, ST.BLOCK, prefilter=True, suppressor=True)
    apply(eng, ST.gate_params(1), ctl)
    first = eng.process(x[:, :500])  # one frame completes, 20 samples wait
    assert first.shape[1] == 480 and eng.pending_input() == 20
    before = (eng.gate_state(), eng.gate_vad_state())
    eng.gate_set_vad_evidence(np.full(5, 0.9, np.float32), np.ones(5, bool))  # the call completes 3 frames: 3 blocks of 500
    with pytest.raises(Exception):
        eng.process(x[:, 500:])
    assert eng.pending_input() == 20
    after = (eng.gate_state(), eng.gate_vad_state())
    for b, a in zip(before, after):
        for key in b:
            assert np.array_equal(b[key], a[key]), key
    ev = (np.full(3, 0.9, np.float32), np.ones(3, bool))
    eng.gate_set_vad_evidence(*ev)
    second = eng.process(x[:, 500:])
    eng.close()
    calls = (500, 3 * 480)
    want, _ = V.run_batch(x, FS, calls, ST.gate_params(1), ctl, [None, ev], ST.BLOCK, suppressor="wrapper")
    got = np.concatenate([first, second], axis=1)
    d = got.astype(np.float64) - want.astype(np.float64)
    assert np.sqrt(np.mean(d * d, axis=1)).max() <= 1e-5
