"""The committed stimulus of the VAD-fused gate tests, on the restatement alone: it must exercise what the device test
compares (all five gate states, opening by probability below the level threshold, chatter with auto-relax, a full
noise-floor history, a floor that moves both ways) and keep the streams that may leave the discrete comparison
(rms_db within 1e-4 dB of a bin edge or of the level threshold) under the 2 % cap."""
import numpy as np
import pytest

import vad_gate_oracle as V
import vad_gate_stimulus as ST


@pytest.fixture(scope="module")
def runs():
    x = ST.audio()
    ev = ST.evidence()
    res = {}
    for name, (mode, ctl) in ST.CONFIGS.items():
        first, st_first = V.run_batch(x, ST.FS, ST.CALLS[:1], ST.gate_params(mode), ctl, ev[:1], ST.BLOCK)
        out, st = V.run_batch(x, ST.FS, ST.CALLS, ST.gate_params(mode), ctl, ev, ST.BLOCK)
        res[name] = (out, st, st_first)
    return res


def test_edge_exclusions_stay_under_the_cap(runs):
    for name, (_, st, _) in runs.items():
        n = int(ST.excluded(st).sum())
        print(f"{name}: {n} of {ST.N_STREAMS} streams within {ST.EDGE_DB} dB of an edge")
        assert n <= ST.EDGE_CAP * ST.N_STREAMS, name
    modes = {ST.CONFIGS[name][0] for name, (_, st, _) in runs.items() if not ST.excluded(st).all()}
    assert modes == {V.VAD_ASSISTED, V.VAD_ONLY}


def test_every_reachable_state_is_visited(runs):
    """Closed, Opening, Open and Uncertain in every configuration.  The fifth state, Releasing, cannot be entered by the
    reference's own rules: it needs `releasing_sustain` without `sustain`, i.e. current_gain > 0.20 with vad_uncertain or
    auto_relax (gate.rs:427-428) -- but vad_uncertain alone is `sustain` in both modes, auto_relax with current_gain > 0.12 is
    `sustain` in VadOnly (:423-425), and current_gain > 0.12 alone is `sustain` in VadAssisted (level_uncertain, :400,
    417-422).  So no stimulus visits it, and this test asserts exactly that of the restatement."""
    for name, (_, st, _) in runs.items():
        seen = int(np.bitwise_or.reduce(st["visited_states"].astype(np.int64)))
        assert seen == 0b01111, (name, bin(seen))


def test_probability_opens_below_the_level_threshold(runs):
    for name, (_, st, _) in runs.items():
        assert int(st["vad_opened_below_level"].max()) > 0, name


def test_chatter_with_auto_relax(runs):
    events = sum(int(st["chatter_events"].sum()) for _, st, _ in runs.values())
    relax = any(bool(st["auto_relax_active"].any()) or bool(first["auto_relax_active"].any()) for _, st, first in runs.values())
    assert events > 0 and relax


def test_history_fills_and_the_floor_moves_both_ways(runs):
    _, st, first = runs["assisted_auto_hold200"]
    assert int(st["history_len"].max()) == V.HISTORY_FRAMES
    up = first["noise_floor_db"] > np.float32(-60.0)
    down = st["noise_floor_db"] < first["noise_floor_db"]
    assert (up & down).any(), (first["noise_floor_db"][:8], st["noise_floor_db"][:8])
    assert len(np.unique(st["floor_bin"])) > 1


def test_the_gate_actually_gates(runs):
    for name, (out, st, _) in runs.items():
        assert float(st["current_gain"].min()) < 0.5 < float(st["current_gain"].max()), name
