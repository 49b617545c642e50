#!/usr/bin/env python3
"""Build-container-only: generate tests/golden/headroom_validation.npz by IMPORTING the reference's own
apply_headroom_validation (python/mic_eq/analysis/auto_eq_parts/headroom.py:292-354) and running it on the captures, Auto-EQ
settings and chain settings of tests/headroom_stimulus.py.  Its _native_simulate (:99-118) is answered by this repository's CPU
oracle, as the native binding answers it in the reference; everything else is the reference's own code.

What is written is data, never reference text: per capture the selected scale, the flags, the status, the scaled gains, the
confidences and validation_gain_scale (NaN where the result has no such key); the numeric keys of ``before`` and ``after``;
and, per (capture, scale) the reference evaluated, the three quantities its safety test reads, with the distance of each from
its threshold.

    python tools/gen_golden_headroom.py      (needs the reference checkout; AF_REFERENCE overrides its place)
"""
from __future__ import annotations

import hashlib
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
REFERENCE = pathlib.Path(os.environ.get("AF_REFERENCE", "/root/reference"))
DECISIVE = ("pre_limiter_true_peak_headroom_db", "limiter_gain_reduction_db", "true_peak_limiter_gain_reduction_db")
OPTIONAL = ("validation_gain_scale", "validation_confidence", "analysis_confidence")


def main() -> None:
    if not (REFERENCE / "python" / "mic_eq").is_dir():
        raise SystemExit("tools/gen_golden_headroom.py runs in the build container only (the reference is not here)")
    sys.path.insert(0, str(REFERENCE / "python"))
    sys.path.insert(0, str(ROOT / "tests"))
    sys.path.insert(0, str(ROOT / "oracle"))
    from mic_eq.analysis.auto_eq_parts import headroom as H

    import af_oracle_py as oracle
    import headroom_stimulus as HS

    evaluated: list = []

    def native(audio_data, sample_rate, bands, flat_settings):
        result = dict(oracle.simulate_auto_eq_chain(np.ascontiguousarray(audio_data, dtype=np.float32), float(sample_rate), bands, flat_settings))
        result.pop("output_audio", None)
        evaluated.append(result)
        return result

    real = H._native_simulate
    H._native_simulate = native
    audio = HS.captures()
    C, S = HS.N_CAPTURES, len(HS.SCALES)
    assert tuple(H.HEADROOM_SCALES) == HS.SCALES
    decisive = np.full((C, S, 3), np.nan)  # NaN: the reference stopped before this scale
    results = []
    try:
        for c in range(C):
            evaluated.clear()
            r = H.apply_headroom_validation(audio[c], HS.FS, HS.eq_settings(c), HS.chain_settings(c))
            results.append(r)
            for k, sim in enumerate(evaluated):
                decisive[c, k] = [float(sim[key]) for key in DECISIVE]
            v = r["headroom_validation"]
            assert v["before"] is evaluated[0] or v["before"] == evaluated[0]
            print(f"  capture {c}: scale {v['gain_scale']} {v['status']} after {len(evaluated)} renders")
        wrong = H.apply_headroom_validation(audio[0], HS.FS, dict(HS.eq_settings(0), band_gains=[1.0] * 9), None)
        assert "headroom_validation" not in wrong and wrong["band_gains"] == [1.0] * 9
    finally:
        H._native_simulate = real
    numeric = sorted(key for key, value in results[0]["headroom_validation"]["before"].items()
                     if isinstance(value, (int, float)) and not isinstance(value, bool) and key != "candidate_runtime_ms")
    margins = np.abs(decisive - np.array([H.HEADROOM_TARGET_DB, H.LIMITER_GAIN_REDUCTION_WARN_DB, H.TRUE_PEAK_GAIN_REDUCTION_WARN_DB]))
    out = {
        "sha256": np.frombuffer(hashlib.sha256(audio.tobytes()).digest(), dtype=np.uint8),
        "gain_scale": np.array([r["headroom_validation"]["gain_scale"] for r in results], dtype=np.float64),
        "status": np.array([r["headroom_validation"]["status"] for r in results]),
        "flags": np.array([[r["headroom_validation"][key] for key in ("safe", "authoritative", "advisory", "meets_advisory_thresholds")]
                           + [r["headroom_safe"], r["headroom_advisory"]] for r in results], dtype=np.int32),
        "headroom_gain_scale": np.array([r["headroom_gain_scale"] for r in results], dtype=np.float64),
        "band_gains": np.array([r["band_gains"] for r in results], dtype=np.float64),
        "optional": np.array([[r.get(key, np.nan) for key in OPTIONAL] for r in results], dtype=np.float64),
        "keys": np.array(["|".join(sorted(r)) for r in results]),
        "numeric_keys": np.array(numeric),
        "before": np.array([[float(r["headroom_validation"]["before"][key]) for key in numeric] for r in results], dtype=np.float64),
        "after": np.array([[float(r["headroom_validation"]["after"][key]) for key in numeric] for r in results], dtype=np.float64),
        "non_finite_output": np.array([[int(r["headroom_validation"][side]["non_finite_output"]) for side in ("before", "after")]
                                       for r in results], dtype=np.int32),
        "decisive": decisive, "margins": margins,
    }
    print(f"  smallest decision margin {np.nanmin(margins):.3e} dB at (capture, scale, quantity) "
          f"{np.unravel_index(int(np.nanargmin(margins)), margins.shape)}")
    target = ROOT / "tests" / "golden" / "headroom_validation.npz"
    np.savez_compressed(target, **out)
    print(f"wrote {target} ({target.stat().st_size} bytes, {len(out)} entries)")


if __name__ == "__main__":
    main()
