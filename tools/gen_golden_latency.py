#!/usr/bin/env python3
"""Build-container-only: generate tests/golden/latency_calibration.npz by IMPORTING the reference's own
python/mic_eq/analysis/latency_calibration.py (it needs scipy) and running it on the recordings of tests/latency_stimulus.py.

What is written is data, never reference text: the reference's probe at the four rates (float32), every field of its result
per case and per stream of the batch, and, for two cases, the lags and normalised scores of its whole-probe search (decimated
for the long one) and of its burst windows, with the GCC-PHAT correlation inside those windows.  The non-finite case is this
project's addition: the reference is not run on it.

    python tools/gen_golden_latency.py      (needs the reference checkout; AF_REFERENCE overrides its place)
"""
from __future__ import annotations

import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
REFERENCE = pathlib.Path(os.environ.get("AF_REFERENCE", "/root/reference"))
DECIMATE = 16


def main() -> None:
    if not (REFERENCE / "python" / "mic_eq" / "analysis").is_dir():
        raise SystemExit("tools/gen_golden_latency.py runs in the build container only (the reference is not here)")
    import importlib.util

    # the module alone: the package's __init__ pulls in the UI
    spec = importlib.util.spec_from_file_location("reference_latency_calibration",
                                                  REFERENCE / "python" / "mic_eq" / "analysis" / "latency_calibration.py")
    R = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = R
    spec.loader.exec_module(R)
    sys.path.insert(0, str(ROOT / "tests"))
    import latency_oracle as LO
    import latency_stimulus as LS

    out = {}
    for rate in LS.RATES:
        out[f"probe_{rate}"] = R.generate_probe_signal(rate, LS.PROBE_MS[rate])
        assert out[f"probe_{rate}"].dtype == np.float32

    def fields(result):
        return {name: getattr(result, name) for name in LO.FIELDS}

    def store(prefix, rows):
        for name in LO.FIELDS:
            values = [row[name] for row in rows]
            if name == "directional_latency_ms":
                assert all(v is None for v in values)
                continue
            if name in ("message", "route_kind", "compensation_basis"):
                out[f"{prefix}{name}"] = np.array(values)
            elif name in ("success", "peak_sample_offset", "repetition_count"):
                out[f"{prefix}{name}"] = np.array(values, dtype=np.int64)
            else:
                out[f"{prefix}{name}"] = np.array(values, dtype=np.float64)

    names = list(LS.CASES)
    rows = []
    for name in names:
        rate, _, akw = LS.CASES[name]
        if name == "non_finite":
            rows.append(LO._failed(LO.NON_FINITE_MESSAGE))
            continue
        r = R.analyze_latency(LS.probe(rate), LS.recording(name), rate, **akw)
        rows.append(fields(r))
        print(f"  {name:16s} {r.success!s:5s} {r.measured_round_trip_ms:9.4f} ms  conf {r.confidence:.4f}  reps {r.repetition_count}  "
              f"amb {r.ambiguity_score:.4f}  {r.message}")
    out["names"] = np.array(names)
    store("case_", rows)

    recorded, lengths, akw = LS.batch()
    rows = []
    for s in range(LS.BATCH):
        x = recorded[s, : lengths[s]]
        if not np.all(np.isfinite(x)):
            rows.append(LO._failed(LO.NON_FINITE_MESSAGE))
        else:
            rows.append(fields(R.analyze_latency(LS.probe(), x, 48_000, max_search_ms=akw["max_search_ms"][s])))
    store("batch_", rows)

    # the score arrays: the reference's own functions on what analyze_latency passes them
    for name in LS.SCORE_CASES:
        rate, _, akw = LS.CASES[name]
        ref, rec = R._normalize_audio(LS.probe(rate)), R._normalize_audio(LS.recording(name))
        min_lag, max_lag = int(5.0 / 1000.0 * rate), int(500.0 / 1000.0 * rate)
        lags, scores = R._normalized_correlation_scores(rec, ref, min_lag=min_lag, max_lag=max_lag)
        step = DECIMATE if lags.size > 2000 else 1
        out[f"scores_{name}_full_lags"], out[f"scores_{name}_full"] = lags[::step], scores[::step]
        coarse = R._pick_peak(lags, scores, direct_path_bias=0.985)[0]
        burst, offsets = R._coded_probe_components(rate, ref.size)
        radius = max(int(round(rate * 0.010)), burst.size)
        n = 1
        while n < rec.size + burst.size:
            n <<= 1
        cross = np.fft.rfft(rec, n=n) * np.conj(np.fft.rfft(burst, n=n))
        cross /= np.maximum(np.abs(cross), 1e-12)
        corr = np.fft.irfft(cross, n=n)
        for k, offset in enumerate(offsets):
            lo = max(min_lag + offset, int(round(coarse + offset - radius)))
            hi = min(max_lag + offset, int(round(coarse + offset + radius)))
            blags, bscores = R._normalized_correlation_scores(rec, burst, min_lag=lo, max_lag=hi)
            out[f"scores_{name}_burst{k}_lags"], out[f"scores_{name}_burst{k}"] = blags, bscores
            out[f"scores_{name}_phat{k}"] = corr[blags] if blags.size and blags.min() >= 0 else np.empty(0)
    target = ROOT / "tests" / "golden" / "latency_calibration.npz"
    np.savez_compressed(target, **out)
    print(f"wrote {target} ({target.stat().st_size} bytes, {len(out)} entries)")


if __name__ == "__main__":
    main()
