"""Cost of the compressor calibration search: --captures compressor inputs of --seconds at 48 kHz resident on the device, searched
through af_compressor_search_run (three sweeps: at most 50 and 16 candidates per capture, then the winners' verification).
Reported, not gated.  --processes child processes one after the other, each --steps + 1 calls with the first discarded; one
JSON line per process: wall ms per call (the host's candidate lists, parameter mirrors and objectives included), the kernels'
ms per phase (sweep and fold), the sweep's nanoseconds per sample and lane (all lanes of a phase run side by side: kernel time
over samples, and the same over samples x lanes), lanes per phase, and the chain time the search replaces when every one of the
evaluations x captures simulations is a chain run of its own at --chain-ms-per-step (the README's measured full-chain step of
4096 streams x 10 s).

The captures are synthetic (noise under an on/off envelope), their input rows are computed from them: the de-esser and EQ pass
that makes a real compressor input is the existing engine's and is measured by bench.py.

    python tools/bench_compressor_search.py [--captures 4096] [--seconds 10] [--steps 3] [--processes 3]
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

FS, BLOCK = 48_000, 960


def run(args) -> None:
    import numpy as np
    import torch

    from mic_eq_mi import compressor_search as cs
    from mic_eq_mi import mic_eq_core as core

    B, n = args.captures, int(args.seconds * FS)
    blocks = -(-n // BLOCK)
    g = torch.Generator(device="cuda").manual_seed(31)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / FS
    audio = torch.empty(B, n, device="cuda")
    rows = np.zeros((blocks, B), dtype=core.STATS_DTYPE)
    for s0 in range(0, B, 256):  # in slices: the generator's temporaries stay small
        b = min(256, B - s0)
        rate = 0.5 + 0.4 * torch.rand(b, 1, device="cuda", generator=g)
        phase = torch.rand(b, 1, device="cuda", generator=g)
        level = 0.05 + 0.25 * torch.rand(b, 1, device="cuda", generator=g)
        envelope = (torch.sin(2 * torch.pi * (rate * t + phase)) > 0.3).float()
        audio[s0:s0 + b] = torch.randn(b, n, device="cuda", generator=g) * (level * envelope + 0.002)
        padded = torch.nn.functional.pad(audio[s0:s0 + b].double(), (0, blocks * BLOCK - n)).reshape(b, blocks, BLOCK)
        rows["input_square_sum"][:, s0:s0 + b] = (padded * padded).sum(dim=2).T.cpu().numpy()
        rows["input_sample_peak"][:, s0:s0 + b] = padded.abs().amax(dim=2).float().T.cpu().numpy()
    torch.cuda.synchronize()
    settings = [cs._search_settings({"threshold_db": -24.0 + (i % 7), "ratio": 2.0 + 0.5 * (i % 6), "attack_ms": 5.0 + (i % 11),
                                     "release_ms": 100.0 + 10.0 * (i % 13), "adaptive_release": True, "base_release_ms": 60.0,
                                     "measured_short_term_lufs": -24.0}, 3.5, 1.5, 8.0) for i in range(B)]
    search = cs.CompressorSearch(FS)
    search.load_device(audio.data_ptr(), n, B, n, rows)
    wall, phases, results = [], [], None
    for step in range(args.steps + 1):
        torch.cuda.synchronize()
        started = time.perf_counter()
        results = search.run(settings)
        torch.cuda.synchronize()
        if step:  # the first repetition is discarded
            wall.append((time.perf_counter() - started) * 1e3)
            phases.append(search.last_run_ms())
    search.close()
    evaluated = [int(r.evaluated_count) for r in results]
    feasible = sum(int(r.backend_available) for r in results)
    lanes = {"phase1": min(sum(evaluated), 50 * B), "phase2": max(0, sum(evaluated) - 50 * B), "verification": feasible}
    best = min(phases, key=lambda p: sum(p.values()))
    simulations = sum(evaluated) + feasible
    print(json.dumps({"bench": "compressor_search", "captures": B, "seconds": args.seconds, "blocks": blocks,
                      "ms_per_call": [round(v, 1) for v in wall],
                      "kernel_ms_per_phase": [{k: round(v, 2) for k, v in p.items()} for p in phases],
                      "kernel_ms": [round(sum(p.values()), 1) for p in phases], "lanes": lanes, "simulations": simulations,
                      "captures_with_a_feasible_candidate": feasible, "expanded_selected": sum(int(r.expanded_search_selected) for r in results),
                      "verification_equals_evaluation": sum(int(r.verification_equals_evaluation) for r in results),
                      "sweep_ns_per_sample": {k: round(best[f"{k}_sweep"] * 1e6 / n, 2) for k in lanes},
                      "sweep_ns_per_sample_and_lane": {k: round(best[f"{k}_sweep"] * 1e6 / n / max(v, 1), 6) for k, v in lanes.items()},
                      "captures_per_s": round(B / (min(wall) * 1e-3), 1),
                      "replaced_chain_ms": round(simulations / 4096.0 * args.chain_ms_per_step * args.seconds / 10.0, 1),
                      "chain_ms_per_step_assumed": args.chain_ms_per_step}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--captures", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--chain-ms-per-step", type=float, default=156.5)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        run(args)
        return
    for _ in range(args.processes):  # a fresh process each: code-object load and first allocations are in the discarded call
        forward = [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("captures", "seconds", "steps", "chain_ms_per_step")]
        subprocess.run([sys.executable, __file__, "--child", *forward], check=True)


if __name__ == "__main__":
    main()
