"""Cost of the latency calibration: LatencyCalibration.analyze on --streams recordings of 0.7 s at 48 kHz (the probe delayed into
a -60 dBFS floor, each stream its own delay and seed).  Reported, not gated.

One line per batch size and process: wall ms per call and last_kernel_ms with its passes (condition: mean and energy prefix;
probe: whole-probe scores and pick; bursts: burst scores and picks; phat: the GCC-PHAT transforms and windows), the median and the
spread over --steps calls after one discarded call.  The whole-probe score kernel's f64 rate is lags x probe length x 2 flop per
stream over the "probe" span (which holds its pick too), against the chip's f64 vector peak of DESIGN 4.3 (78.6 TFLOP/s).
A last line times tests/latency_oracle.py, the NumPy restatement, on one thread of this host for scale.

    python tools/bench_latency_calibration.py [--streams 1024,4096] [--steps 5] [--processes 3]
"""
from __future__ import annotations

import argparse
import json
import pathlib
import statistics
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "audio-forge_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

FS, N = 48_000, 33_600
F64_PEAK_TFLOPS = 78.6


def recordings(count):
    import numpy as np

    import latency_stimulus as LS

    base = np.stack([LS.record(FS, N, seed=500 + s, delay=500 + 311 * s) for s in range(64)])
    return np.ascontiguousarray(np.tile(base, ((count + 63) // 64, 1))[:count])


def run(args) -> None:
    import mic_eq_mi
    import latency_stimulus as LS

    probe = LS.probe()
    for count in args.streams:
        recorded = recordings(count)
        lc = mic_eq_mi.LatencyCalibration(FS, probe, count, N)
        wall, total, passes, ok = [], [], [], 0
        for step in range(args.steps + 1):
            started = time.perf_counter()
            results = lc.analyze(recorded)
            if step:  # the first repetition is discarded
                wall.append((time.perf_counter() - started) * 1e3)
                ms, parts = lc.last_kernel_ms(passes=True)
                total.append(ms)
                passes.append(parts)
            ok = sum(r.success for r in results)
        lags = min(int(0.5 * FS), N - probe.size) - int(0.005 * FS) + 1
        probe_ms = statistics.median(p["probe"] for p in passes)
        print(json.dumps({
            "bench": "latency_calibration", "streams": count, "samples": N, "succeeded": ok,
            "wall_ms_per_call": [round(v, 1) for v in wall], "kernel_ms": [round(v, 2) for v in total],
            "kernel_ms_median": round(statistics.median(total), 2),
            "pass_ms_median": {k: round(statistics.median(p[k] for p in passes), 3) for k in passes[0]},
            "pass_ms_min_max": {k: [round(min(p[k] for p in passes), 3), round(max(p[k] for p in passes), 3)] for k in passes[0]},
            "us_per_stream": round(1e3 * statistics.median(total) / count, 2),
            "probe_score_tflops": round(2.0 * lags * probe.size * count / (probe_ms * 1e-3) / 1e12, 2),
            "probe_score_fraction_of_f64_peak": round(2.0 * lags * probe.size * count / (probe_ms * 1e-3) / 1e12 / F64_PEAK_TFLOPS, 3)}), flush=True)
        lc.close()


def oracle_line() -> None:
    import latency_oracle as LO
    import latency_stimulus as LS

    probe, recorded = LS.probe(), recordings(4)
    times = []
    for x in list(recorded) * 2:
        started = time.perf_counter()
        LO.analyze_latency(probe, x, FS)
        times.append((time.perf_counter() - started) * 1e3)
    print(json.dumps({"bench": "latency_oracle_one_thread", "samples": N, "ms_per_recording_median": round(statistics.median(times[1:]), 1),
                      "ms_min_max": [round(min(times[1:]), 1), round(max(times[1:]), 1)]}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=lambda v: [int(x) for x in v.split(",")], default=[1024, 4096])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        run(args)
        return
    for _ in range(args.processes):  # a fresh process each: code-object load and first allocations are in the discarded call
        subprocess.run([sys.executable, __file__, "--child", "--streams", ",".join(map(str, args.streams)), f"--steps={args.steps}"], check=True)
    oracle_line()


if __name__ == "__main__":
    main()
