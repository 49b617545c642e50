#!/usr/bin/env python3
"""Build-container-only: generate tests/golden/compressor_search.npz by IMPORTING the reference's own
_calibrate_compressor_threshold (python/mic_eq/analysis/voice_setup.py:742-1079) and running it on the captures of
tests/compressor_search_stimulus.py, with its simulate_candidate_chain answered by this repository's CPU oracle
(oracle.af_oracle_py.simulate_auto_eq_chain behind the reference's own _bands_from_settings / _flatten_chain_settings, the result
marked "rust" as the native binding's is).

What is written is data, never reference text: per capture every simulated candidate in order (the last one is the winner's
verification), the objective of every evaluated candidate (+inf: hard-rejected), and the values of the two returned dicts.
The module's `sorted` is shadowed by a recording one to see the objectives, which the function keeps to itself.

The generator asserts that the outcome classes the tests rely on occur, and that no decision of the search is closer than a
relative 1e-4 (1e-3 dB for the two level cuts) to flipping; it prints the smallest margin it found.

    python tools/gen_golden_compressor_search.py      (needs the reference checkout; AF_REFERENCE overrides its place)
"""
from __future__ import annotations

import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
REFERENCE = pathlib.Path(os.environ.get("AF_REFERENCE", "/root/reference"))


def main() -> None:
    if not (REFERENCE / "python" / "mic_eq").is_dir():
        raise SystemExit("tools/gen_golden_compressor_search.py runs in the build container only (the reference is not here)")
    sys.path.insert(0, str(REFERENCE / "python"))
    for p in (ROOT / "tests", ROOT / "oracle"):
        sys.path.insert(0, str(p))
    from mic_eq.analysis import voice_setup as V
    from mic_eq.analysis.auto_eq_parts import headroom as H

    import af_oracle_py as oracle
    import compressor_search_stimulus as CS

    calls: list = []
    sorts: list = []

    def simulate(audio, sample_rate, eq_settings, chain_settings=None):
        flat = H._flatten_chain_settings(chain_settings)
        result = dict(oracle.simulate_auto_eq_chain(np.ascontiguousarray(audio, dtype=np.float32), float(sample_rate),
                                                    H._bands_from_settings(eq_settings), flat))
        result["simulation_backend"] = "rust"
        calls.append((dict(chain_settings["compressor"]), result))
        return result

    def recording_sorted(items, **kwargs):
        out = sorted(items, **kwargs)
        sorts.append([(item[0], dict(item[2])) for item in out])
        return out

    V.simulate_candidate_chain = simulate
    V.sorted = recording_sorted
    audio = CS.captures()
    out: dict = {}
    smallest = np.inf
    seen = set()
    for c, (name, level, deesser, compressor, (p95, median, cap)) in enumerate(CS.CASES):
        calls.clear()
        sorts.clear()
        calibrated, diagnostics = V._calibrate_compressor_threshold(
            speech_audio=audio[c], sample_rate=CS.FS, eq_settings=CS.EQ_SETTINGS, deesser_settings=dict(deesser),
            compressor_settings=dict(compressor), target_p95_db=p95, target_median_db=median, peak_cap_db=cap)
        feasible_run = diagnostics["backend"] == "rust"
        evaluations = calls[:-1] if feasible_run else list(calls)
        values = np.array([[settings[k] for k in CS.CONTROLS] for settings, _ in evaluations])
        scores = np.full(len(evaluations), np.inf)
        for score, v in sorts[-1]:
            hit = [i for i, row in enumerate(values) if all(row[j] == v[k] for j, k in enumerate(CS.CONTROLS))]
            assert hit, (name, v)  # (candidates that clamp to the same values are simulated alike and score alike)
            scores[hit] = score
        assert len(evaluations) == diagnostics["iterations"] - (1 if feasible_run else 0)
        # ---- margins of every decision
        for settings, sim in evaluations:  # the hard rejections, :862-867
            smallest = min(smallest, abs(sim["output_true_peak_db"] - (sim["limiter_effective_ceiling_db"] + 0.10)) / 1e-3 * 1e-4,
                           abs(sim["compressor_gain_reduction_db"] - (cap + 1.0e-6)) / 1e-3 * 1e-4)
            assert not sim["non_finite_output"]
        finite = np.unique(scores[np.isfinite(scores)])  # (candidates that clamp to the same values score alike: no decision)
        if finite.size > 1:  # what decides feasible[0] (and with it the final expanded candidate)
            smallest = min(smallest, (finite[1] - finite[0]) / max(abs(finite[0]), 1e-12))
        if feasible_run:
            first = np.unique(scores[:50][np.isfinite(scores[:50])])  # phase 1: feasible[0] and the second seed
            for a, b in zip(first[:3], first[1:4]):
                smallest = min(smallest, (b - a) / max(abs(a), 1e-12))
            threshold_only, expanded = diagnostics["threshold_only_objective"], diagnostics["expanded_candidate_objective"]
            if np.isfinite(threshold_only):  # the tie-break, :989-992
                required = max(0.001, 0.01 * threshold_only)
                smallest = min(smallest, abs((threshold_only - expanded) - required) / max(required, 1e-12))
            winner = [i for i, row in enumerate(values) if all(row[j] == calibrated[k] for j, k in enumerate(CS.CONTROLS))]
            assert winner  # (the first of equal candidates: both sorts are stable)
            verification = calls[-1][1]
            assert all(verification[k] == evaluations[winner[0]][1][k] for k in verification if k not in ("candidate_runtime_ms", "output_audio"))
            incumbent_like = all(abs(values[winner[0]][j] - np.clip(compressor[k], *V._COMPRESSOR_SEARCH_BOUNDS[k])) <= 1e-6
                                 for j, k in enumerate(CS.CONTROLS) if j > 0)
            if diagnostics["expanded_search_selected"]:
                seen.add("expanded_local_step" if winner[0] >= 50 else "expanded_halton" if winner[0] >= 34 else "expanded_threshold")
                assert (name == "halton") == (34 <= winner[0] < 50), (name, winner[0])  # a phase-1 Halton point over its own +- steps
            elif expanded < threshold_only:
                seen.add("threshold_only_kept")
            assert diagnostics["expanded_search_selected"] != incumbent_like
            out[f"{c}/winner"] = np.int32(winner[0])
        else:
            seen.add("no_feasible")
            assert len(evaluations) == 50 and calibrated == compressor
            out[f"{c}/winner"] = np.int32(-1)
        if len(evaluations) == 65 and name == "grid_point":  # the incumbent's threshold is one of the 33: one duplicate
            seen.add("grid_point_duplicate")
        out[f"{c}/evaluated"] = values
        out[f"{c}/scores"] = scores
        out[f"{c}/calibrated"] = np.array([calibrated[k] for k in CS.CONTROLS])
        out[f"{c}/numbers"] = np.array([diagnostics.get(k, 0.0) for k in CS.DIAGNOSTIC_NUMBERS], dtype=np.float64)
        out[f"{c}/flags"] = np.array([feasible_run, bool(diagnostics.get("expanded_search_selected", False)),
                                      bool(diagnostics.get("peak_cap_passed", False)), diagnostics["iterations"],
                                      diagnostics.get("candidate_count", 0)], dtype=np.int32)
        out[f"{c}/keys"] = np.array(sorted(diagnostics), dtype="U64")
        print(f"{name}: margin so far {smallest:.3e}; {len(evaluations)} evaluations, backend {diagnostics['backend']}, winner {int(out[f'{c}/winner'])}, "
              f"expanded {diagnostics.get('expanded_search_selected')}, calibrated {out[f'{c}/calibrated'].tolist()}")
    wanted = {"expanded_local_step", "expanded_halton", "threshold_only_kept", "no_feasible", "grid_point_duplicate"}
    assert seen >= wanted, wanted - seen
    out["classes"] = np.array(sorted(seen), dtype="U32")
    assert any(c[3]["auto_makeup_enabled"] for c in CS.CASES) and not all(c[3]["auto_makeup_enabled"] for c in CS.CASES)
    assert any(not (lo <= c[3][k] <= hi) for c in CS.CASES for k, (lo, hi) in V._COMPRESSOR_SEARCH_BOUNDS.items())
    print(f"smallest decision margin: {smallest:.3e} (relative; the level cuts scaled so that 1e-3 dB reads 1e-4)")
    assert smallest >= 1e-4, smallest
    out["smallest_margin"] = np.float64(smallest)
    import hashlib

    out["audio_sha256"] = np.array(hashlib.sha256(audio.astype("<f4").tobytes()).hexdigest())
    np.savez_compressed(CS.FIXTURE, **out)
    print(f"wrote {CS.FIXTURE} ({CS.FIXTURE.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
