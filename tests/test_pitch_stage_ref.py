"""The float64 reference of the pitch path (tests/pitch_stage_ref.py) and its stimulus (tests/pitch_stage_stimulus.py), held
against the CPU restatement's taps in both evaluation orders.  No GPU.

This validates the reference (an independent f64 statement of pitch_downsample, pitch_search and remove_doubling has to
agree with the f32 restatement cell by cell), yields the yardsticks the GPU test uses (the restatement's own distance from
f64 on the same cells: tests/test_gpu_pitch_stages.py takes 4 x order 0's), and proves the stimulus: every edge of the
arithmetic that the GPU test relies on is reached on the f64 results, and the restatement alone needs at most 0.5 % excused
cells per stage.  A stimulus that misses an edge fails here.

Measured (order 0 | order 1): whitened buffer, max |d| / buffer peak 5.5e-4 | 5.4e-3 (the worst cell is a `sub` stream: two
spectral lines, which LPC-4 whitens with a prediction gain that multiplies the autocorrelation's f32 rounding; voiced cells
sit near 1e-5); call-end gain 1.9e-7 | 1.1e-6; comparison operands 5.6e-7 | 2.3e-6 relative, so tau = 2.2e-6 | 9.2e-6;
excused cells 0 of 1403 (search) and 0 of 1333 (tracker) in either order.
"""
import numpy as np
import pytest

import pitch_stage_ref as P
import pitch_stage_stimulus as T

ORDERS = (0, 1)
RESTATEMENT_CAP = 0.005  # the restatement alone; the device's cap is 1 %


def _search_status(r: dict) -> np.ndarray:
    return np.concatenate([part["check"]["status"].ravel() for part in r["search"].values()])


def _search_infos(r: dict, key) -> list:
    return r["search"][key]["check"]["info"]


@pytest.mark.parametrize("order", ORDERS)
def test_reference_agrees_with_the_restatement(order):
    """No cell out of the replay's reach, the excused share within the cap, the tracker state consistent at every call end."""
    r = T.restatement(order)
    search, tracker = _search_status(r), r["engine"]["check"]["status"]
    print(f"order {order}: tau {r['tau']:.3e} (operands {r['operand_distance']:.3e}) | buffer {r['buffer_worst']:.3e} -> bound "
          f"{r['buffer_bound']:.3e} | gain {r['gain_worst']:.3e} -> bound {r['gain_bound']:.3e} | excused: search "
          f"{int(np.sum(search == 1))}/{search.size}, tracker {int(np.sum(tracker == 1))}/{tracker.size}")
    assert search.size == sum(T.SEARCH_FRAMES) * len(T.SEARCH_STREAMS) + T.N_FRAMES * len(T.READ_STREAMS)
    assert tracker.shape == (T.N_FRAMES, len(T.READ_STREAMS))
    assert not np.any(search == 2), np.argwhere(search == 2)[:8]
    assert not np.any(tracker == 2), np.argwhere(tracker == 2)[:8]
    assert P.excused_share(search) <= RESTATEMENT_CAP and P.excused_share(tracker) <= RESTATEMENT_CAP
    assert r["engine"]["check"]["period_wrong"] == []
    # the yardsticks are f32 rounding, not a disagreement of the two statements (the buffer: a running sum of 864 terms is
    # good to ~1e-4 in the autocorrelation, and the whitening filter's prediction gain of 30-40 dB multiplies that)
    assert r["operand_distance"] <= 64 * P.F32_EPS and r["gain_worst"] <= 64 * P.F32_EPS and r["buffer_worst"] <= 1e-2


@pytest.mark.parametrize("order", ORDERS)
def test_all_zero_buffers_are_exact(order):
    r = T.restatement(order)
    col = [i for i, s in enumerate(T.READ_STREAMS) if T.ROLES.get(s) == "zeros"]
    assert len(col) == 2
    assert not np.any(r["engine"]["pitch_ds"][:, col].view(np.uint32) & 0x7FFFFFFF) and np.all(r["engine"]["buffer_err"][:, col] == 0.0)
    for n in T.SEARCH_FRAMES:
        assert not np.any(r["search"][n]["ds"][:, 0].view(np.uint32) & 0x7FFFFFFF)
        assert np.all(r["search"][n]["index"][:, :2] == 768)  # zeros, and the lone impulse: no positive correlation


def test_every_edge_is_reached_on_the_f64_results():
    """On the strict f64 results of the cells the GPU test reads (order 0's buffers; order 1 sees the same edges)."""
    for order in ORDERS:
        r = T.restatement(order)
        col = {s: i for i, s in enumerate(T.READ_STREAMS)}
        info = r["engine"]["check"]["info"]
        frames = range(T.N_FRAMES)
        # ac[0] == 0: the all-zero buffer
        assert P.pitch_downsample(T.pitch_buffer(T.model_spans(), col[6], 5))[1]["ac0_zero"]
        assert not P.pitch_downsample(T.pitch_buffer(T.model_spans(), col[0], 5))[1]["ac0_zero"]
        # T0 >= maxperiod clamped to 383 (the search returned 768), on a live stream too
        clamped = [(f, s) for (f, s), v in info.items() if v["clamped_t0"]]
        assert any(T.ROLES.get(T.READ_STREAMS[s]) in ("sweep_up", "sweep_down") for f, s in clamped), "T0 clamp on a voiced frame"
        # the final index clamped to 60
        assert sum(v["clamped_final"] for v in info.values()) >= 2
        assert int(r["engine"]["pitch_index"].min()) == 60 and int(r["engine"]["pitch_index"].max()) >= 760
        # the loop's break at the first candidate under the minimum period: as early as k = 4 (the search's shortest period
        # is 182, so T0 >= 91 and k = 2, 3 always run) and as late as k = 13
        assert all(v["past_min"] for v in info.values())
        assert any(v["T0"] < 118 for v in info.values()) and any(v["T0"] >= 12 * 30 for v in info.values())
        # all three arms of `cont`
        for arm in ("full", "half", "none"):
            assert sum(arm in v["arms"] for v in info.values()) >= 10, arm
        # remove_doubling does remove: the final period is a sub-multiple of the search's on some frames
        assert sum(v["T"] != v["T0"] for v in info.values()) >= 20
        # best0 at 0 and at the last lag (no interpolation offset), two coarse candidates within +-2, on the synthetic spans
        for n in T.SEARCH_FRAMES:
            infos = _search_infos(r, n)
            by = lambda stream: [infos[f * len(T.SEARCH_STREAMS) + T.SEARCH_STREAMS.index(stream)] for f in range(n)]  # noqa: E731
            assert any(i["coarse"][0] == 0 and i["fine"][0] == 0 and i["best0_at_edge"] for i in by("lag0")), n
            assert all(i["fine"][0] == 293 and i["best0_at_edge"] and 146 in i["coarse"] for i in by("lag146")), n
            assert all(abs(i["coarse"][0] - i["coarse"][1]) == 1 and i["candidates_overlap"] for i in by("twin")), n
        assert any(i["coarse"][0] == 146 for n in T.SEARCH_FRAMES for i in _search_infos(r, n))
        # an interpolation offset of either sign occurs, and none
        offsets = {i["offset"] for k in r["search"] for i in _search_infos(r, k)}
        assert offsets == {-1, 0, 1}
        # the history of the drain stream empties over four frames, and its buffer is not zero after them (the high-pass tail)
        d = col[22]
        peaks = [float(np.max(np.abs(T.pitch_buffer(T.model_spans(), d, f)[:P.PBUF - 4 * T.FRAME]))) for f in frames]
        assert peaks[T.DRAIN_FRAME + 2] > 1000.0 and peaks[T.DRAIN_FRAME + 4] < 1000.0
        # the late stream: two silent frames first
        assert r["engine"]["silence"][:2, col[38]].all() and not r["engine"]["silence"][3:, col[38]].any()
        # every second_check entry that can run (k = 3 .. 12) decides the gain of its own stream: with the entry changed the
        # f64 gain moves by far more than the device's bound, at every call end
        ends = np.cumsum(T.CALLS) - 1
        e = r["engine"]
        for k in range(3, 13):
            s = col[next(stream for stream, role in T.ROLES.items() if role == f"sub{k}")]
            changed = list(P.SECOND_CHECK)
            changed[k] += 1
            for f in ends[3:]:
                buf, prev, gain = e["pitch_ds"][f, s], int(e["pitch_index"][f - 1, s]), float(e["pitch_gain"][f - 1, s])
                search = P.pitch_search(buf)[0]
                right = P.remove_doubling(buf, search, prev, gain)
                wrong = P.remove_doubling(buf, search, prev, gain, second_check=tuple(changed))
                assert right[2]["accepted"] == k and right[0] == int(e["pitch_index"][f, s]), (k, int(f))
                assert wrong[0] != right[0] or abs(wrong[1] - right[1]) > 50 * T.restatement(0)["gain_bound"], (k, int(f))
        assert all((2 * 383 + k) // (2 * k) < 30 for k in (13, 14, 15))  # these entries cannot run
    # frame counts that leave 1, 2 and 3 live waves in the search's four-frame workgroup
    assert {n % 4 for n in T.CALLS} >= {1, 2, 3} and {n % 4 for n in T.SEARCH_FRAMES} >= {0, 1, 2, 3}


def test_the_replay_excuses_ties_and_nothing_else():
    """The tolerant replay on a buffer with a real near-tie reaches both outcomes; a result no near-tie leads to is refused."""
    r = T.restatement(0)
    ds = r["search"][4]["ds"][0, T.SEARCH_STREAMS.index("twin")].astype(np.float64)
    index, info = P.pitch_search(ds)
    assert P.replay(lambda D: P.pitch_search(ds, D), index, r["tau"], key=lambda q: q[0])[0] == "equal"
    for wrong in (index + 1, index - 1, index + 2, 768, 2 * index):
        assert P.replay(lambda D: P.pitch_search(ds, D), wrong, r["tau"], key=lambda q: q[0])[0] == "fail", wrong
    # with a tolerance as wide as the gap between the offset rule's two sides, the other side becomes reachable
    a, b, c = info["abc"]
    assert info["offset"] == 0  # both rules refuse; index = 768 - 2 best + offset, so the first rule's other side is index + 1
    wide = 1.01 * abs(c - (0.7 * b + 0.3 * a)) / max(abs(c), abs(0.7 * b + 0.3 * a))
    assert wide > 100 * r["tau"]
    state, _ = P.replay(lambda D: P.pitch_search(ds, D), index + 1, wide, key=lambda q: q[0])
    assert state == "excused", (state, index, wide)
    # the tracker: a wrong final index one lag off, a wrong carried gain that flips a decision
    e = r["engine"]
    f, s = next((f, s) for (f, s), v in e["check"]["info"].items() if "full" in v["arms"] and v["T"] != v["T0"] and f > 0)
    buf, prev, gain = e["pitch_ds"][f, s], int(e["pitch_index"][f - 1, s]), float(e["pitch_gain"][f - 1, s])
    fn = lambda g: (lambda D: P.remove_doubling(buf, P.pitch_search(buf, D)[0], prev, g, D))  # noqa: E731
    final = int(e["pitch_index"][f, s])
    assert P.replay(fn(gain), final, r["tau"], key=lambda q: q[0])[0] == "equal"
    assert P.replay(fn(gain), final + 2, r["tau"], key=lambda q: q[0])[0] == "fail"


def test_published_quirks_are_reproduced():
    """The `else if T1 < 2 minperiod` arm can never run (T1 < 2 minperiod implies T1 < 3 minperiod): the threshold under
    2 minperiod is the .85 / .4 one, not the .9 / .5 one -- reproduced, not repaired."""
    rng = np.random.default_rng(5)
    t = np.arange(P.HALF)
    ds = np.sin(2 * np.pi * t / 50.0) + 0.25 * np.sin(2 * np.pi * t / 100.0 + 1.0)  # period 50, a weak component at 100
    index, gain, info = P.remove_doubling(ds, 200, 0, 0.0)
    assert info["T0"] == 100 and not info["clamped_t0"] and info["arms"] == {"none"}
    # k = 2: T1 = 50 lies in [minperiod, 2 minperiod); g1 is held against max(.4, .85 g0) -- which it passes -- where
    # max(.5, .9 g0) would have refused it
    x = ds[384:864]
    corr = lambda lag: float(np.dot(x, ds[384 - lag:864 - lag]))  # noqa: E731
    xx = corr(0)
    yy = lambda lag: xx + sum(ds[384 - i] ** 2 - ds[864 - i] ** 2 for i in range(1, lag + 1))  # noqa: E731
    g0 = corr(100) / np.sqrt(1 + xx * yy(100))
    g1 = 0.5 * (corr(50) + corr(150)) / np.sqrt(1 + xx * 0.5 * (yy(50) + yy(150)))
    assert max(0.4, 0.85 * g0) < g1 <= max(0.5, 0.9 * g0), (g0, g1)
    assert info["T"] == 50 and index == 100 and abs(gain - g1) < 1e-12
    # the decimation's first sample has no left neighbour
    x = rng.standard_normal(P.PBUF)
    d = P.decimate(x)
    assert d[0] == 0.5 * (0.5 * x[1] + x[0]) and d[1] == 0.5 * (0.5 * (x[1] + x[3]) + x[2])
    # Levinson's early exit: a pure tone is predicted to under .001 of ac[0] by order 2, orders 3 and 4 stay zero
    lpc = P.lpc4(np.cos(2 * np.pi * np.arange(5) / 40.0))  # the exact autocorrelation of a tone
    assert lpc[0] != 0 and lpc[1] != 0 and lpc[2] == 0 and lpc[3] == 0
