"""The de-esser's stimulus (tests/deesser_stimulus.py) reaches the branches its cases are meant to cover -- on the ORACLE alone:
the oracle's de-esser is stepped sample by sample over the stream that represents each role, through the ctypes mirror of
`afo_deesser`, and the predicates of `afo_deesser_process_sample` are recomputed from the recorded state
(tests/deesser_trace.py).  A branch counts when it is taken on at least 500 (sample, band) pairs of one stream; every sample of
the stream is counted, none is picked.

Which case covers what.  Every case that reduces: gain update and 0.001 dB hold, narrow_support on and off, ratio_conf on both
sides of 0.12, the zero-envelope guard, narrowness below the 0.34 gate, one stream over 1 dB.  The auto cases: voice_active
true and false, baseline rising and falling, and decaying from a value that is not 0 while the voice is inactive.  B, D (and
B's parameters in G and H): the budget rescale.  C: the per-band `auto_cap` binding while the sum stays under the budget.  D and
E: the three manual-mode exits.  F: nothing moves at all.
Narrowness ABOVE 0.68 is asserted for G-full only: the detectors are second-order filters an octave and less apart, so with the
default cuts the largest band holds at most ~0.63 of the three envelopes' sum whatever the input (measured here: 0.628; a tone
at a band's centre gives 0.36); with the cuts at 2 and 16 kHz the voice's harmonics sit under all three high-passes and the
lowest band reaches 0.85."""
import ctypes as C

import numpy as np
import pytest

import af_oracle_py as O
import chain_oracle as CO
import deesser_stimulus as DS
import deesser_trace as DT
import signals as S

MIN_SAMPLES = 500
_REDUCING = ("update", "hold", "narrow_support_on", "narrow_support_off", "ratio_conf_low", "ratio_conf_high", "zero_env",
             "narrowness_low")
_AUTO = ("voice_active_true", "voice_active_false", "baseline_rise", "baseline_fall", "baseline_decay")
_MANUAL = ("manual_below_threshold", "manual_ratio_exit", "manual_active")
COVERS = {
    "A": _REDUCING + _AUTO,
    "B": _REDUCING + _AUTO + ("budget_rescale",),
    "C": _REDUCING + _AUTO + ("band_cap_under_budget",),
    "D": _REDUCING + _MANUAL + ("budget_rescale",),
    "E-60": _REDUCING + _MANUAL,
    "E-6": ("update", "hold", "manual_below_threshold", "manual_active"),
    "E-out": _REDUCING + _MANUAL + ("budget_rescale",),
    "F-max0": _AUTO,
    "F-ratio1": _MANUAL,
    "G-high": ("update", "hold", "budget_rescale") + _AUTO[:-1],  # (three bands at 12 kHz: only the `narrow` tone there gives a ratio)
    "G-full": _REDUCING[:-1] + _AUTO + ("budget_rescale", "narrowness_high"),
    "G-moved": _REDUCING + _AUTO + ("budget_rescale",),
    "H-44k1": _REDUCING + _AUTO + ("budget_rescale",),
    "H-96k": _REDUCING + _AUTO + ("budget_rescale",),
}
_OVER_1_DB = [c for c in DS.CASES if c not in ("E-6", "F-max0", "F-ratio1")]  # (E-6: only a full-scale tone passes -6 dB, by 0.4 dB)


def test_struct_mirror_matches_the_oracle():
    L = O.lib()
    assert C.sizeof(O.Biquad) == L.afo_biquad_sizeof()
    assert C.sizeof(O.DeEsserBand) == L.afo_deesser_band_sizeof()
    assert C.sizeof(O.DeEsser) == L.afo_deesser_sizeof()
    d = DT.new_deesser(44_100.0, DS.CASES["E-out"][3])  # every value outside its clamp
    assert (d.enabled, d.auto_enabled, d.sample_rate) == (1, 0, 44_100.0)
    assert (d.auto_amount, d.threshold_db, d.ratio, d.max_reduction_db) == (1.0, -60.0, 20.0, 24.0)
    assert d.attack_coeff == L.afo_time_constant_to_coeff(0.1, 44_100.0)
    assert d.release_coeff == L.afo_time_constant_to_coeff(500.0, 44_100.0)
    d = DT.new_deesser(48_000.0, DS.CASES["G-moved"][3])
    assert (d.low_cut_hz, d.high_cut_hz) == (3500.0, 9000.0)
    low, split_a, split_b, high = DS.band_layout(DS.CASES["G-moved"][3])
    assert [(b.low_hz, b.high_hz) for b in d.bands] == [(low, split_a), (split_a, split_b), (split_b, high)]
    for b in d.bands:  # the cuts moved after construction: a 72-sample crossfade pends on all nine filters
        for f in (b.detector_hp, b.detector_lp, b.dynamic_eq):
            assert (f.xf_total, f.xf_remaining, f.sample_rate, f.enabled) == (72, 72, 48_000.0, 1)
        assert (b.detector_hp.frequency, b.detector_lp.frequency) == (b.low_hz, b.high_hz)
        assert b.dynamic_eq.frequency == np.sqrt(b.low_hz * b.high_hz) and b.dynamic_eq.gain_db == 0.0
    # the chain's own de-esser through the same mirror
    chain = CO.make_chain(48_000.0, S.LIMITER_BANDS, DS.CASES["D"][3], eq_enabled=False)
    inner = O.DeEsser.from_address(chain.deesser)
    assert (inner.enabled, inner.auto_enabled, inner.threshold_db, inner.ratio, inner.max_reduction_db) == (1, 0, -40.0, 6.0, 8.0)


@pytest.mark.parametrize("case", list(DS.CASES))
def test_layout_matches_the_oracle(case):
    fs, _, _, settings = DS.CASES[case]
    d = DT.new_deesser(fs, settings)
    low, split_a, split_b, high = DS.band_layout(settings)
    assert [(b.low_hz, b.high_hz) for b in d.bands] == [(low, split_a), (split_a, split_b), (split_b, high)]


def test_roles_and_twins():
    roles = DS.roles()
    assert len(roles) == DS.N_STREAMS == 67
    assert set(roles) == {"ess", "narrow", "wide", "ramp", "late", "quiet", "dip", "loud", "nonfinite", "twin"}
    assert "dc" in DS.roles(dc=True)
    x = DS.batch("A")
    assert x.dtype == np.float32 and x.shape == (67, DS.CASES["A"][1])
    assert x.tobytes() == DS.batch("A").tobytes()  # deterministic
    for copy, original in DS.TWINS.items():
        assert copy // 64 != original // 64 and copy % 64 != original % 64
        assert x[copy].tobytes() == x[original].tobytes()
    for s in (0, 63, 64, 66):  # the tile edges carry full-scale roles
        assert float(np.nanmax(np.abs(x[s][np.isfinite(x[s])]))) >= 0.94, s
    assert float(np.abs(x[63]).max()) > 1.0  # `loud` exceeds +-1.0
    late = DS.role_streams()["late"]
    assert not x[late, : x.shape[1] // 4].any() and x[late, x.shape[1] // 4 :].any()
    quiet = DS.role_streams()["quiet"]
    assert abs(20.0 * np.log10(np.abs(x[quiet]).max()) + 62.0) < 1e-3
    bad = x[DS.role_streams()["nonfinite"]]
    fs, n, calls, _ = DS.CASES["A"]
    assert np.isnan(bad).any() and (bad == np.inf).any() and (bad == -np.inf).any()
    assert not np.isfinite(bad[calls[0] - 1]) and not np.isfinite(bad[calls[0]]) and not np.isfinite(bad[DS.control_block(fs)])
    assert float(DS.batch("A", dc=True)[DS.role_streams(dc=True)["dc"]].mean()) > 0.02


@pytest.mark.parametrize("case", list(DS.CASES))
def test_case_reaches_its_branches_on_the_oracle(case):
    fs, n, calls, settings = DS.CASES[case]
    audio = DS.batch(case)
    counts, max_reduction = {}, {}
    for role, s in DS.role_streams().items():
        x = CO.sanitize(audio[s], False)
        out, state = DT.trace(x, fs, settings)
        taken_by = DT.predicates(state)
        for name, taken in taken_by.items():
            counts[name] = max(counts.get(name, 0), int(taken.sum()))
        max_reduction[role] = float(state["current_reduction_db"].max())
        if case.startswith("F") or (case == "D" and role == "quiet"):  # on but inert: nothing moves, not even the dynamic EQs' gain
            assert max_reduction[role] == 0.0 and not state["bands"]["reduction_db"].any(), (case, role)
            assert not state["bands"]["dynamic_eq"]["gain_db"].any()
            assert out.tobytes() == x.tobytes(), (case, role)
        if role == "quiet" and bool(settings.get("deesser_auto_enabled", True)):
            assert not taken_by["voice_active_true"].any()  # inactive for the whole stream
        if case == "D" and role == "wide":  # a manual reduction that acts and stays under its cap (0.75 x max)
            assert 1.0 < max_reduction[role] < 0.75 * 8.0
        if case == "C":  # the sum of the three capped bands never reaches the 24 dB budget
            assert max_reduction[role] <= 3 * 7.4 + 1e-9 and not taken_by["budget_rescale"].any()
    print(f"de-esser stimulus {case}: " + ", ".join(f"{k} {v}" for k, v in sorted(counts.items())))
    print(f"de-esser stimulus {case}: max reduction " + ", ".join(f"{k} {v:.3f}" for k, v in max_reduction.items()))
    missing = {name: counts.get(name, 0) for name in COVERS[case] if counts.get(name, 0) < MIN_SAMPLES}
    assert not missing, f"case {case}: branches taken on fewer than {MIN_SAMPLES} samples of every role stream: {missing}"
    if case in _OVER_1_DB:
        assert max(max_reduction.values()) > 1.0, max_reduction


@pytest.mark.parametrize("eq_first", [False, True])
@pytest.mark.parametrize("case", ["B", "D", "E-out", "G-moved"])
def test_chain_replay_equals_the_simulation_with_the_deesser(case, eq_first):
    """`chain_oracle.make_chain` sets the de-esser up as `afo_simulate_auto_eq_chain` does: one call through the replay gives the
    simulation's output bit for bit, in both stage orders, and the largest block reduction is the simulation's figure."""
    deesser = {k: v for k, v in DS.CASES[case][3].items() if k.startswith("deesser_")}
    settings = dict(S.limiter_settings(2.0), eq_before_deesser=eq_first, **deesser)
    x = np.ascontiguousarray(DS.batch(case)[0][:12_345])
    got, rows = CO.run_calls(x, 48_000, S.LIMITER_BANDS, settings, (x.size,))
    want = O.simulate_auto_eq_chain(x, 48_000, S.LIMITER_BANDS, dict(settings, return_output_audio=True))
    assert got.tobytes() == want["output_audio"].tobytes()
    assert float(rows["deesser_gain_reduction_db"].max()) == want["deesser_gain_reduction_db"] > 1.0
