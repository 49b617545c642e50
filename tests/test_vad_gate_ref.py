"""The reference's own unit tests of the VAD-fused gate, restated one for one on tests/ref/vad_gate_ref.c (the Rust cannot be
compiled here, so this is what holds the restatement to the reference): the eleven gate tests at gate.rs:1109-1295 and the
controller's tests at vad/tests.rs:8-14, 22-146, 472-495.  Same constructor arguments, block lengths and assertions.  Where
the reference constructs VadAutoGate::new, this constructs without_backend (the fields start equal, vad.rs:628-690; the
tests call process_with_probability directly and never touch a Silero session).  The remaining tests of vad/tests.rs are
Silero's resampler and model contract: not restated."""
import numpy as np

import vad_gate_oracle as V

F32 = np.float32


def amp_db(db):  # 10f32.powf(db / 20.0)
    return F32(np.power(F32(10.0), F32(db) / F32(20.0), dtype=np.float32))


def gate(attack=1.0, release=20.0, vad_threshold=0.5, mode=V.VAD_ASSISTED):
    g = V.VadGate(-40.0, attack, release, 48_000.0)
    g.set_vad_auto_gate(vad_threshold)
    g.set_gate_mode(mode)
    return g


def block(value, n):
    return np.full(n, value, dtype=np.float32)


# ---- gate.rs:1109-1295
def test_vad_assisted_uses_level_when_external_probability_unavailable():
    g = gate()
    g.set_external_vad_probability(0.0, False)
    g.process_block_inplace(block(0.1, 3000))
    assert g.current_gain() > 0.5
    assert not g.is_vad_available()


def test_vad_only_closes_when_external_probability_unavailable():
    g = gate(mode=V.VAD_ONLY)
    g.set_external_vad_probability(0.0, False)
    g.process_block_inplace(block(0.1, 3000))
    assert g.current_gain() < 0.2
    assert not g.is_vad_available()


def test_vad_assisted_fused_score_opens_for_strong_evidence():
    g = gate()
    g.set_external_vad_probability(0.9, True)
    g.process_block_inplace(block(0.1, 3000))
    assert g.fused_gate_score() >= V.FUSED_GATE_OPEN_SCORE
    assert g.current_gain() > 0.5


def test_vad_assisted_uses_vad_open_decision_below_level_threshold():
    g = gate(vad_threshold=0.4)
    g.set_external_vad_probability(0.45, True)
    g.process_block_inplace(block(amp_db(-42.0), 3000))
    assert g.current_gain() > 0.35


def test_vad_only_honors_configured_vad_threshold():
    g = gate(vad_threshold=0.4, mode=V.VAD_ONLY)
    g.set_external_vad_probability(0.45, True)
    g.process_block_inplace(block(0.1, 3000))
    assert g.current_gain() > 0.5


def test_vad_assisted_fused_score_resists_weak_noise():
    g = gate()
    g.set_external_vad_probability(0.1, True)
    g.process_block_inplace(block(0.0005, 3000))
    assert g.fused_gate_score() <= V.FUSED_GATE_CLOSE_SCORE
    assert g.current_gain() < 0.3


def test_vad_state_machine_opens_on_rising_probability():
    g = gate()
    g.set_hold_time(0.0)
    g.set_external_vad_probability(0.42, True)
    g.process_block_inplace(block(amp_db(-46.0), 2000))
    assert g.gate_state() == V.OPEN
    assert g.current_gain() > 0.25


def test_vad_state_machine_preserves_ambiguous_trailing_speech():
    g = gate()
    g.set_hold_time(0.0)
    g.set_external_vad_probability(0.90, True)
    g.process_block_inplace(block(0.08, 2000))
    open_gain = g.current_gain()
    g.set_external_vad_probability(0.41, True)
    g.process_block_inplace(block(amp_db(-45.0), 2000))
    assert g.gate_state() != V.CLOSED
    assert g.current_gain() > open_gain * 0.45, (open_gain, g.current_gain())


def test_vad_state_machine_rejects_short_click_with_low_probability():
    g = gate()
    g.set_hold_time(0.0)
    g.set_external_vad_probability(0.05, True)
    click = block(0.0, 512)
    click[0] = 0.8
    g.process_block_inplace(click)
    assert g.gate_state() == V.CLOSED
    assert g.current_gain() < 0.2


def test_vad_chatter_triggers_auto_relax():
    g = gate(release=5.0, mode=V.VAD_ONLY)
    g.set_hold_time(0.0)
    for _ in range(5):
        g.set_external_vad_probability(0.95, True)
        g.process_block_inplace(block(0.1, 256))
        g.set_external_vad_probability(0.0, True)
        g.process_block_inplace(block(0.0, 256))
    assert g.chatter_event_count() > 0
    assert g.auto_relax_active()


def test_continuous_vad_reduction_is_monotone_and_flat_at_speech_endpoints():
    g = V.VadGate(-40.0, 1.0, 20.0, 48_000.0)
    low = g.continuous_vad_gain_reduction_db(V.VAD_ONLY, 0.10, True, False, 0.50)
    uncertain = g.continuous_vad_gain_reduction_db(V.VAD_ONLY, 0.40, True, False, 0.50)
    high = g.continuous_vad_gain_reduction_db(V.VAD_ONLY, 0.90, True, False, 0.50)
    assert low > uncertain
    assert uncertain > high
    assert abs(high) < 1.0e-9
    assert low <= V.EXPANDER_RANGE_DB * V.VAD_ONLY_CONTINUOUS_SCALE


# ---- gate.rs:1009-1017, the one threshold-path test that reaches into apply_gain (the fused path shares it)
def test_noise_gate_force_close_transitions_are_smoothed():
    g = V.VadGate(-40.0, 10.0, 100.0, 48_000.0)
    g.set_current_gain(1.0)
    floor_gain = V.db_to_linear(-V.EXPANDER_RANGE_DB)
    g.apply_gain(0.5, V.EXPANDER_RANGE_DB)
    assert g.current_gain_f64() > floor_gain + 1e-3


# ---- vad/tests.rs:8-14
def test_rms_computation():
    assert V.compute_rms_db(np.zeros(1000, np.float32)) < -100.0
    assert abs(V.compute_rms_db(np.ones(1000, np.float32)) - 0.0) < 0.1


# ---- vad/tests.rs:22-46
def test_hold_time_persists_gate_after_speech_drop():
    g = V.controller(48000, 0.5)
    g.set_gate_mode(V.VAD_ONLY)
    g.set_hold_time(100.0)
    frame = block(0.01, 480)
    assert g.ctl_process_with_probability(frame, 0.9)
    for _ in range(5):
        assert g.ctl_process_with_probability(frame, 0.0)
    final_state = True
    for _ in range(6):
        final_state = g.ctl_process_with_probability(frame, 0.0)
    assert not final_state


# ---- vad/tests.rs:48-68
def test_debounce_blocks_short_reopen_glitch():
    g = V.controller(48000, 0.5)
    g.set_gate_mode(V.VAD_ONLY)
    g.set_hold_time(0.0)
    frame = block(0.01, 480)
    assert g.ctl_process_with_probability(frame, 0.9)
    assert not g.ctl_process_with_probability(frame, 0.0)
    assert not g.ctl_process_with_probability(frame, 0.9)
    for _ in range(5):
        g.ctl_process_with_probability(frame, 0.0)
    assert g.ctl_process_with_probability(frame, 0.9)


# ---- vad/tests.rs:70-88
def test_auto_threshold_adapts_toward_background_level():
    g = V.controller(48000, 0.5)
    g.set_gate_mode(V.VAD_ASSISTED)
    g.set_auto_threshold(True)
    initial_floor = g.noise_floor()
    frame = block(amp_db(-45.0), 480)
    for _ in range(250):
        g.ctl_process_with_probability(frame, 0.1)
    assert g.noise_floor() > initial_floor + F32(4.0)
    assert g.noise_floor() < -40.0


# ---- vad/tests.rs:90-108
def test_auto_threshold_ignores_high_confidence_speech_frames():
    g = V.controller(48_000, 0.5)
    g.set_gate_mode(V.VAD_ASSISTED)
    g.set_auto_threshold(True)
    initial_floor = g.noise_floor()
    frame = block(amp_db(-25.0), 480)
    for _ in range(300):
        g.ctl_process_with_probability(frame, 0.9)
    assert abs(g.noise_floor() - initial_floor) < 0.25, "high-confidence speech should not pollute noise floor"


# ---- vad/tests.rs:110-146
def test_auto_threshold_slew_limits_per_frame():
    g = V.controller(48_000, 0.5)
    g.set_gate_mode(V.VAD_ASSISTED)
    g.set_auto_threshold(True)
    quiet, loud = block(amp_db(-70.0), 480), block(amp_db(-35.0), 480)
    for _ in range(V.HISTORY_FRAMES):
        g.ctl_process_with_probability(quiet, 0.1)
    before_rise = g.noise_floor()
    g.ctl_process_with_probability(loud, 0.1)
    after_rise = g.noise_floor()
    assert after_rise - before_rise <= V.UP_SLEW + F32(1e-6), "rise slew exceeded per-frame limit"
    g.reset_controller()
    g.set_auto_threshold(True)
    for _ in range(V.HISTORY_FRAMES):
        g.ctl_process_with_probability(loud, 0.1)
    before_fall = g.noise_floor()
    g.ctl_process_with_probability(quiet, 0.1)
    after_fall = g.noise_floor()
    assert before_fall - after_fall <= V.DOWN_SLEW + F32(1e-6), "fall slew exceeded per-frame limit"


# ---- vad/tests.rs:472-481
def test_noise_floor_reliability_requires_mature_history():
    g = V.controller(48_000, 0.4)
    for _ in range(V.HISTORY_FRAMES // 4):
        g.ctl_push_noise_floor_sample(-52.0)
    expected = F32(V.HISTORY_FRAMES // 4) / F32(V.HISTORY_FRAMES)
    assert abs(g.noise_floor_reliability() - expected) < 1.0e-6


# ---- vad/tests.rs:483-494
def test_noise_floor_reliability_rejects_nonstationary_history():
    stationary, varying = V.controller(48_000, 0.4), V.controller(48_000, 0.4)
    for index in range(V.HISTORY_FRAMES):
        stationary.ctl_push_noise_floor_sample(-52.0 + float(index % 2))
        varying.ctl_push_noise_floor_sample(-72.0 + float(index % 30))
    assert stationary.noise_floor_reliability() > 0.95
    assert varying.noise_floor_reliability() < 0.10


# ---- gate.rs:659, 743-745, 814-817: ThresholdOnly with the controller attached is the per-sample expander and the controller
# is not stepped; selecting ThresholdOnly puts gate_state back to Closed
def test_threshold_only_with_controller_attached_is_the_expander():
    import af_oracle_py as O

    rng = np.random.default_rng(3)
    x = (rng.standard_normal(6000) * 0.05 * (np.arange(6000) % 2000 < 900)).astype(np.float32)
    g = gate(attack=10.0, release=100.0, mode=V.THRESHOLD_ONLY)
    g.set_external_vad_probability(0.9, True)
    got = g.process_block_inplace(x.copy())
    want = O.Gate(-40.0, 10.0, 100.0, 48_000.0).process(x)
    assert np.array_equal(got, want)
    assert g.report().history_len == 0 and g.noise_floor() == F32(-60.0)
    g.set_gate_mode(V.VAD_ONLY)
    g.process_block_inplace(block(0.1, 512))
    assert g.gate_state() != V.CLOSED
    g.set_gate_mode(V.THRESHOLD_ONLY)
    assert g.gate_state() == V.CLOSED
