"""The mixdown stimulus reaches every branch of the phase-safe mixdown on the restatement alone (no GPU): a batch that did
not would let the GPU comparison pass without testing them.  If a branch is not reached, the stimulus is what changes."""
import numpy as np

import mixdown_oracle as MO
import mixdown_stimulus as S


def _counters():
    return S.reference(2, MO.PHASE_SAFE_MONO)[2]


def test_batch_shape_and_sequence():
    x = S.batch()
    assert x.shape == (67, S.N_FRAMES, 2) and x.dtype == np.float32
    assert S.CALLBACKS[:10] == (1, 2, 3, 5, 16, 17, 128, 480, 1000, 8192 + 5)
    assert np.isfinite(x).all()
    # every stream has material of its own
    assert len({x[s].tobytes() for s in range(67)}) == 67
    # the families the comparison relies on are all there
    assert {"coherent", "antiphase", "frac", "anti_delay", "noise", "hyst_reuse", "hyst_clear", "silence", "tiny", "negzero",
            "tie"} <= set(S.FAMILIES)
    assert {f"delay+{d}" for d in range(1, 9)} <= set(S.FAMILIES)
    assert np.signbit(x[S.FAMILIES.index("negzero")]).any()
    assert float(np.abs(x[[s for s, f in enumerate(S.FAMILIES) if f == "tiny"]]).min(axis=(1, 2)).max()) < 1e-3


def test_all_four_strategies_in_at_least_three_streams_each():
    cnt = _counters()
    for key in ("strategy_none", "strategy_flip", "strategy_fractional", "strategy_fallback"):
        assert sum(1 for c in cnt if c[key] > 0) >= 3, key


def test_every_branch_is_taken():
    cnt = _counters()
    total = {k: sum(c[k] for c in cnt) for k in MO.COUNTERS}
    for key in ("warm_up", "lagrange_clamp", "best_delay_edge", "delayed_none_short", "delayed_none_denom", "stereo_none",
                "hysteresis_reused", "hysteresis_cleared", "tie", "parabola_missing"):
        assert total[key] >= 1, (key, total)


def test_neighbouring_streams_decide_differently():
    _, diags, _ = S.reference(2, MO.PHASE_SAFE_MONO)
    d = diags[8]  # after the 1000-frame callback
    differs = sum(1 for s in range(66) if (d["strategy"][s], d["estimated_delay"][s]) != (d["strategy"][s + 1], d["estimated_delay"][s + 1]))
    assert differs >= 50


def test_the_tie_goes_to_the_first_lag():
    _, diags, _ = S.reference(2, MO.PHASE_SAFE_MONO)
    s = [i for i, f in enumerate(S._FAMILY) if f == ("tie", 1)][0]
    # lags -6, -2, 2 and 6 tie at exactly 1.0; the parabola moves the estimate by less than half a frame
    assert diags[8]["strategy"][s] == MO.FRACTIONAL_DELAY and abs(diags[8]["estimated_delay"][s] + 6.0) < 0.5


def test_average_and_phase_safe_average_differ_in_the_sign_of_zero():
    s = [i for i, f in enumerate(S._FAMILY) if f == ("negzero", 0)][0]
    avg = S.reference(2, MO.AVERAGE)[0][6][s]
    safe = S.reference(2, MO.PHASE_SAFE_MONO)[0][6][s]
    assert not np.signbit(avg).any() and np.signbit(safe).all() and np.all(avg == 0) and np.all(safe == 0)


def test_lagrange_clamp_beyond_its_bounds():
    h = np.random.default_rng(5).standard_normal(16).astype(np.float32)
    assert MO.lagrange_sample(h, 0.5) == MO.lagrange_sample(h, 2.0) == h[2]
    assert MO.lagrange_sample(h, 20.0) == MO.lagrange_sample(h, 13.0) == h[13]
