#!/usr/bin/env python3
"""Cost of the per-stream lifecycle calls: restart, export and import of 1, 64 and 4096 streams of a running
4096-stream engine, for the dynamics chain (1.8 KB per blob) and for the full chain with suppressor and gate (12 KB).

    python tools/bench_stream_lifecycle.py [--streams 4096] [--reps 7] [--step-timeout 120]

Every (configuration, list size) pair is one GPU step: a child process of its own under its own time limit, one JSON line
each.  A step that fails or runs out of time ends the run: nothing further is started on the device.  Times are wall clock
around the call plus `Engine.synchronize()` (so the launch, the copies and the host-side transposition all count); `issue_ms`
is the time until the call itself returned (restart and import do not wait for the device)."""
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
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

CONFIGS = ("dynamics", "suppressor-gate")
SIZES = (1, 64, 4096)


def child(config: str, n_list: int, n_streams: int, reps: int) -> dict:
    import numpy as np

    import stream_lifecycle_cases as SL

    eng = SL.engine(config, n_streams=n_streams)
    try:
        rng = np.random.default_rng(7)
        eng.process((0.5 * rng.standard_normal((n_streams, SL.CALL))).astype(np.float32))
        listed = list(range(min(n_list, n_streams)))
        out = {"config": config, "engine_streams": n_streams, "listed": len(listed), "blob_bytes": eng.stream_state_size(), "reps": reps}
        blobs = eng.export_stream_state(listed)  # (also warms the staging buffers)
        for name, call in (("export", lambda: eng.export_stream_state(listed)), ("import", lambda: eng.import_stream_state(listed, blobs)),
                           ("restart", lambda: eng.restart_streams(listed))):
            total, issue = [], []
            for _ in range(reps + 1):
                eng.synchronize()
                t0 = time.perf_counter()
                call()
                t1 = time.perf_counter()
                eng.synchronize()
                t2 = time.perf_counter()
                issue.append((t1 - t0) * 1e3)
                total.append((t2 - t0) * 1e3)
            out[name] = {"ms": round(statistics.median(total[1:]), 4), "min_ms": round(min(total[1:]), 4), "max_ms": round(max(total[1:]), 4),
                         "issue_ms": round(statistics.median(issue[1:]), 4)}
        return out
    finally:
        eng.close()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-timeout", type=float, default=120.0, help="seconds per GPU step")
    ap.add_argument("--child", nargs=2, metavar=("CONFIG", "N"), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child(args.child[0], int(args.child[1]), args.streams, args.reps)), flush=True)
        return 0
    for config in CONFIGS:
        for n in SIZES:
            cmd = [sys.executable, str(pathlib.Path(__file__).resolve()), "--streams", str(args.streams), "--reps", str(args.reps),
                   "--child", config, str(n)]
            try:
                done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print(json.dumps({"config": config, "listed": n, "error": f"no result within {args.step_timeout} s"}), flush=True)
                return 1
            if done.returncode != 0:
                print(json.dumps({"config": config, "listed": n, "error": done.stderr.strip().splitlines()[-1:]}), flush=True)
                return 1
            print(done.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
