"""What makes the GPU comparison of tests/test_gpu_latency_calibration.py meaningful: on the recordings of
tests/latency_stimulus.py (the cases and the batch of 70) every decision of analyze_latency clears its threshold by far more than
the arithmetic of any implementation moves a score, so equal discrete results are a property of the code and not of luck.

* score against threshold, at least 1e-4 relative: `>= max x bias` for every index up to and including the chosen one, the 0.035
  skip of a burst, and the 0.07 / 0.90 / 0.82 / 0.32 / 6.0 ms rules of the verdict;
* the parabola: |denom| >= 1e-6 and |raw offset| not within 1e-4 relative of the clip at 0.5;
* the integer roundings of expected_lag -+ local_radius: not within 1e-6 of a half-integer, unless the whole-probe parabola is
  saturated (exactly -+0.5), where the value is exactly k + 0.5 and round-half-even decides the same everywhere;
* the PHAT maximum inside each used window exceeds the runner-up by 1e-6 relative.
Digital silence is exempt: every sum is exactly 0 in any arithmetic."""
import numpy as np
import pytest

import latency_oracle as LO
import latency_stimulus as LS

SCORE_MARGIN = 1e-4
PHAT_MARGIN = 1e-6


@pytest.fixture(scope="module")
def traces():
    out = {}
    for name, (rate, _, akw) in LS.CASES.items():
        trace = {}
        LO.analyze_latency(LS.probe(rate), LS.recording(name), rate, trace=trace, **akw)
        out[name] = trace
    recorded, lengths, akw = LS.batch()
    for s in range(LS.BATCH):
        trace = {}
        if np.any(recorded[s, : lengths[s]]):
            LO.analyze_latency(LS.probe(), recorded[s, : lengths[s]], 48_000, trace=trace, max_search_ms=akw["max_search_ms"][s])
        out[f"stream {s}"] = trace
    return out


def picks(trace):
    if "full_pick" in trace:
        yield "full", trace["full_pick"]
        for entry in trace["bursts"]:
            if "pick" in entry:
                yield f"burst {entry['offset']}", entry["pick"]


def test_the_stimulus_reaches_every_branch(traces):
    ran = [name for name, trace in traces.items() if "full_pick" in trace and name not in LS.EXACT]
    assert len(ran) >= 50
    assert any(trace.get("fallback") for trace in traces.values())                          # no burst is used: :397-422
    assert any(0 < sum(e["used"] for e in trace["bursts"]) < 4 for trace in traces.values() if "bursts" in trace)  # a skipped burst
    raws = [pick["raw_offset"] for name in ran for _, pick in picks(traces[name]) if pick["raw_offset"] is not None]
    assert any(abs(r) < 0.5 for r in raws) and any(abs(r) > 0.5 for r in raws)             # the clip both idle and saturated
    assert any(0.05 < abs(traces[name]["full_pick"]["raw_offset"]) < 0.45 for name in ran)  # "fractional": a parabola at work


def test_every_score_decision_clears_its_threshold(traces):
    smallest = np.inf
    for name, trace in traces.items():
        if name in LS.EXACT or "full_pick" not in trace:
            continue
        for where, pick in picks(trace):
            smallest = min(smallest, pick["threshold_clearance"])
            assert pick["threshold_clearance"] >= SCORE_MARGIN, (name, where, pick["threshold_clearance"])
            if where != "full":
                d = abs(pick["peak_score"] - 0.035) / 0.035
                smallest = min(smallest, d)
                assert d >= SCORE_MARGIN, (name, where, pick["peak_score"])
        for rule, (value, threshold) in trace["rules"].items():
            d = abs(value - threshold) / threshold
            smallest = min(smallest, d)
            assert d >= SCORE_MARGIN, (name, rule, value)
    print(f"smallest relative distance of a score from its threshold: {smallest:.3e}")


def test_parabolas_and_roundings_are_well_conditioned(traces):
    for name, trace in traces.items():
        if name in LS.EXACT or "full_pick" not in trace:
            continue
        used = {"full"} | {f"burst {e['offset']}" for e in trace["bursts"] if e["used"]}
        for where, pick in picks(trace):
            if pick["denom"] is None or where not in used:
                continue  # the peak is at an end of its window: no parabola; a skipped burst: its lag is never read
            assert abs(pick["denom"]) >= 1e-6, (name, where, pick["denom"])
            assert abs(abs(pick["raw_offset"]) - 0.5) >= 1e-4 * 0.5, (name, where, pick["raw_offset"])
        raw = trace["full_pick"]["raw_offset"]
        saturated = raw is not None and abs(raw) >= 0.5
        for entry in trace["bursts"]:
            for value in entry["rounding"]:
                distance = abs(value - np.floor(value) - 0.5)
                if saturated:
                    assert distance == 0.0, (name, entry["offset"], value)
                else:
                    assert distance >= 1e-6, (name, entry["offset"], value)


def test_phat_maximum_is_clear_of_the_runner_up(traces):
    checked = 0
    for name, trace in traces.items():
        if name in LS.EXACT or "bursts" not in trace:
            continue
        for entry in trace["bursts"]:
            if "phat_abs" in entry and entry["phat_abs"].size > 1:
                top = np.sort(entry["phat_abs"])[-2:]
                assert top[1] - top[0] >= PHAT_MARGIN * top[1], (name, entry["offset"], top)
                checked += 1
    assert checked >= 200
