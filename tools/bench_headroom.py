"""Cost of the EQ headroom validation: apply_headroom_validation_batch on --captures captures of --seconds at 48 kHz, each with
its own ten-band EQ, through the seven gain scales.  Reported, not gated.

Two lines per process.  "sweep": route "sweep" (one front-end engine run, the per-lane EQ over captures x 7 lanes, the compressor
sweep and its fold): wall ms per call and the kernel ms of lane EQ, sweep and fold.  "engine": the same call on route "engine",
simulate_auto_eq_chain_batch once per scale with one preset per capture (a 64-stream group each), which is the only way to make
the sweep without the per-lane EQ; it runs on --engine-captures captures (a preset per capture costs 64 streams of host and
device memory: 256 captures of 10 s are 31 GB of packed input per scale), and ms_per_capture is what to compare.
--processes child processes one after the other, each --steps + 1 calls with the first discarded.

The captures are synthetic (noise under an on/off envelope at mixed levels, so that every scale is selected somewhere).

    python tools/bench_headroom.py [--captures 256] [--engine-captures 32] [--seconds 10] [--steps 3] [--processes 3]
"""
from __future__ import annotations

import argparse
import json
import pathlib
import subprocess
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "audio-forge_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

FS = 48_000
FREQS = [80.0, 160.0, 320.0, 640.0, 1280.0, 2500.0, 5000.0, 8000.0, 12000.0, 16000.0]


def run(args) -> None:
    import numpy as np

    from mic_eq_mi import headroom as H

    B, n = args.captures, int(args.seconds * FS)
    rng = np.random.default_rng(41)
    t = np.arange(n, dtype=np.float32) / FS
    audio = np.empty((B, n), dtype=np.float32)
    for s in range(B):
        envelope = (np.sin(2 * np.pi * (rng.uniform(0.5, 0.9) * t + rng.uniform())) > 0.3).astype(np.float32)
        audio[s] = rng.standard_normal(n, dtype=np.float32) * (rng.uniform(0.02, 0.4) * envelope + 0.002)
    eq = [{"band_freqs": FREQS, "band_gains": rng.uniform(-3.0, 6.0, 10).tolist(), "band_qs": rng.uniform(0.7, 2.0, 10).tolist()}
          for _ in range(B)]
    chain = {"compressor": {"threshold_db": -24.0, "ratio": 3.0, "makeup_gain_db": 3.0}}
    for route, count in (("sweep", B), ("engine", min(B, args.engine_captures))):
        wall, kernels, results = [], [], None
        for step in range(args.steps + 1):
            timing: dict = {}
            started = time.perf_counter()
            results = H.apply_headroom_validation_batch(audio[:count], FS, eq[:count], chain, route=route, timing=timing)
            if step:  # the first repetition is discarded
                wall.append((time.perf_counter() - started) * 1e3)
                kernels.append({k: round(v, 2) for k, v in timing.items()})
        scales = [r["headroom_gain_scale"] for r in results]
        line = {"bench": "headroom_validation", "route": route, "captures": count, "seconds": args.seconds, "lanes": count * len(H.HEADROOM_SCALES),
                "ms_per_call": [round(v, 1) for v in wall], "ms_per_capture": round(min(wall) / count, 2),
                "selected_scales": {str(s): scales.count(s) for s in H.HEADROOM_SCALES}, "unsafe": sum(not r["headroom_safe"] for r in results)}
        if route == "sweep":
            line["kernel_ms"] = kernels
        print(json.dumps(line), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=256)
    ap.add_argument("--engine-captures", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        run(args)
        return
    for _ in range(args.processes):  # a fresh process each: code-object load and first allocations are in the discarded call
        forward = [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("captures", "engine_captures", "seconds", "steps")]
        subprocess.run([sys.executable, __file__, "--child", *forward], check=True)


if __name__ == "__main__":
    main()
