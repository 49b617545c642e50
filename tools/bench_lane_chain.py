"""Cost of per-stream settings: the streaming lane chain (mic_eq_mi.LaneChain, one lane per stream) against the group route
(simulate_auto_eq_chain_batch with per-stream presets: every distinct preset padded to a 64-stream group).  Reported, with one
gate that the driver checks and exits non-zero on: at 4096 distinct presets the lane chain's fastest call must be faster than
the group route's 4096-preset figure (the lanes line of this run, or of --gate-against FILE for a --groups-only run).

Without a step the tool is the driver: it runs every step below as a child process under `timeout`, one after the other, stops
at the first step that fails (a fault, an abort or a time limit: nothing more is started on the device), and appends every line
to --out.  Input is resident on the device; each step makes --steps + 1 calls and discards the first.

    lanes   LaneChain at --streams streams x --seconds, all settings distinct: wall ms per call (process_device + the wait)
            and the kernel's ms.
    short   the same object in calls of 960 samples (one 20 ms block): the realtime use, state load and store included.
    groups  the group route at --presets distinct presets x --seconds, ONE chunk of the larger counts: the packed input of
            4096 presets x 10 s is 503 GB, so 1024, 4096 and 16384 presets are not run; the line gives the measured chunk
            and, under "scaled_...", the chunk multiplied by the number of chunks each count needs.  "engine": an Engine
            with one preset per 64-stream group over device-resident packed input (what the operator runs inside, without
            its host packing and copies); "operator": simulate_auto_eq_chain_batch itself on host arrays.  --run-presets
            1024 (the driver's default) RUNS that count as well: 16 chunks, each an engine of its own with its own 64
            presets, "run_engine_wall_ms" being the sum of their process calls.

--root names the tree whose package is measured (default: this one), so that the parent commit's group route can be timed by
the same script from a checkout of the parent; --label is how the lines name that tree ("tree").

    python tools/bench_lane_chain.py [--out profiles/lane_chain_bench.jsonl] [--seconds 10] [--steps 3]
"""
from __future__ import annotations

import argparse
import json
import os
import pathlib
import subprocess
import sys
import time

HERE = pathlib.Path(__file__).resolve().parents[1]
FS = 48_000
LANE_COUNTS = (64, 1024, 4096, 16384)


def paths(root: pathlib.Path) -> None:
    for p in (root, root / "audio-forge_amd", HERE / "tests"):
        sys.path.insert(0, str(p))


def distinct_settings(count: int):
    import lane_chain_stimulus as LS

    bands, settings = [], []
    for i in range(count):
        st = LS.engine_settings(LS.settings(i % LS.N_STREAMS))
        st["compressor_enabled"] = st["limiter_enabled"] = True
        st["compressor_threshold_db"] = -40.0 + 30.0 * i / max(count - 1, 1)  # every stream its own
        bands.append(LS.bands(i))
        settings.append(st)
    return bands, settings


def device_audio(streams: int, n: int):
    import torch

    g = torch.Generator(device="cuda").manual_seed(7)
    level = torch.logspace(-1.7, 0.4, streams, device="cuda").unsqueeze(1)
    return torch.randn((streams, n), generator=g, device="cuda", dtype=torch.float32).mul_(0.25 * level)


def step_lanes(args, short: bool) -> dict:
    import torch

    import mic_eq_mi

    streams, n = args.streams, int(args.seconds * FS)
    bands, settings = distinct_settings(streams)
    d_in = device_audio(streams, n)
    d_out = torch.empty_like(d_in)
    chain = mic_eq_mi.LaneChain(float(FS), streams)
    started = time.perf_counter()
    chain.configure(range(streams), bands, settings)
    configure_ms = (time.perf_counter() - started) * 1e3
    wall, kernel = [], []
    call = 960 if short else n
    calls = (20 if short else 1) * (args.steps + 1)
    for k in range(calls):
        at = (k * call) % (n - call + 1) if short else 0
        torch.cuda.synchronize()
        started = time.perf_counter()
        chain.process_device(d_in.data_ptr() + 4 * at, d_out.data_ptr() + 4 * at, call, n)
        torch.cuda.synchronize()
        if k >= (20 if short else 1):  # the first repetition is discarded
            wall.append((time.perf_counter() - started) * 1e3)
            kernel.append(chain.last_kernel_ms())
    chain.close()
    line = {"bench": "lane_chain", "step": "short" if short else "lanes", "tree": args.label, "streams": streams, "samples_per_call": call,
            "configure_host_ms": round(configure_ms, 1)}
    if short:
        line.update(calls=len(wall), wall_ms_per_call_median=round(sorted(wall)[len(wall) // 2], 3),
                    kernel_ms_per_call_median=round(sorted(kernel)[len(kernel) // 2], 3), wall_ms_per_call_max=round(max(wall), 3))
    else:
        line.update(seconds=args.seconds, wall_ms_per_call=[round(v, 1) for v in wall], kernel_ms_per_call=[round(v, 1) for v in kernel])
    return line


def step_groups(args) -> dict:
    import ctypes as C

    import numpy as np
    import torch

    import mic_eq_mi
    from mic_eq_mi import _lib, mic_eq_core as core

    n = int(args.seconds * FS)
    presets = args.presets
    bands, settings = distinct_settings(presets)
    packed = presets * core.GROUP_STREAMS
    chunks = {count: -(-count // presets) for count in LANE_COUNTS}
    line = {"bench": "lane_chain", "step": "groups", "tree": args.label, "presets": presets, "seconds": args.seconds,
            "packed_streams": packed}
    # the engine the operator builds, over device-resident packed input (63 of 64 streams of a group are the padding's silence)
    d_in = torch.zeros((packed, n), device="cuda", dtype=torch.float32)
    d_in[:: core.GROUP_STREAMS] = device_audio(presets, n)
    d_out = torch.empty_like(d_in)

    def engine_calls(chunk_bands, chunk_settings, calls: int) -> list:
        engine = core.Engine(float(FS), packed)
        engine.set_preset_count(presets)
        for k in range(presets):
            engine.select_preset(k)
            core.configure_auto_eq_chain(engine, float(FS), chunk_bands[k], chunk_settings[k])
        gp = np.arange(presets, dtype=np.int32)
        _lib.check(engine._lib.af_engine_assign_presets(engine._h, gp.ctypes.data_as(C.POINTER(C.c_int32)), int(gp.size)))
        times = []
        for _ in range(calls):
            engine.reset()
            torch.cuda.synchronize()
            started = time.perf_counter()
            engine.process_device(d_in.data_ptr(), d_out.data_ptr(), n, n)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - started) * 1e3)
        engine.close()
        return times

    wall = engine_calls(bands, settings, args.steps + 1)[1:]  # the first repetition is discarded
    line["engine_wall_ms_per_call"] = [round(v, 1) for v in wall]
    line["scaled_engine_wall_ms"] = {str(count): round(min(wall) * k, 1) for count, k in chunks.items()}
    if args.run_presets > presets:  # this count is run, not scaled: one engine per chunk, every chunk its own presets
        all_bands, all_settings = distinct_settings(args.run_presets)
        total = 0.0
        for c0 in range(0, args.run_presets, presets):
            total += engine_calls(all_bands[c0 : c0 + presets], all_settings[c0 : c0 + presets], 1)[0]
        line["run_engine_wall_ms"] = {str(args.run_presets): round(total, 1)}
    del d_in, d_out
    if args.operator:
        audio = device_audio(presets, n).cpu().numpy()
        wall = []
        for k in range(args.steps + 1):
            started = time.perf_counter()
            mic_eq_mi.simulate_auto_eq_chain_batch(audio, FS, bands, settings, diagnostics=False)
            if k:
                wall.append((time.perf_counter() - started) * 1e3)
        line["operator_wall_ms_per_call"] = [round(v, 1) for v in wall]
        line["scaled_operator_wall_ms"] = {str(count): round(min(wall) * k, 1) for count, k in chunks.items()}
    return line


def drive(args) -> int:
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    env = dict(os.environ)
    for name in ("OMP_NUM_THREADS", "MKL_NUM_THREADS", "OPENBLAS_NUM_THREADS"):
        env[name] = str(min(16, int(env.get(name, "16") or 16)))
    base = [sys.executable, __file__, "--seconds", str(args.seconds), "--steps", str(args.steps), "--root", str(args.root),
            "--label", args.label]
    lines = [json.loads(t) for t in pathlib.Path(args.gate_against).read_text().splitlines() if t.startswith("{")] if args.gate_against else []
    steps = []
    if not args.groups_only:
        steps += [(["--step", "lanes", "--streams", str(c)], 240) for c in LANE_COUNTS]
        steps += [(["--step", "short", "--streams", "4096"], 120)]
    steps += [(["--step", "groups", "--presets", str(args.presets), "--operator", "--run-presets", str(args.run_presets)], 420)]
    for extra, limit in steps:
        done = subprocess.run(["timeout", "-k", "10", str(limit)] + base + extra, env=env, capture_output=True, text=True)
        sys.stderr.write(done.stderr[-2000:])
        if done.returncode != 0:
            print(json.dumps({"bench": "lane_chain", "failed_step": extra, "returncode": done.returncode}), flush=True)
            return done.returncode  # nothing more is started on the device
        for text in done.stdout.splitlines():
            if text.startswith("{"):
                print(text, flush=True)
                lines.append(json.loads(text))
                with out.open("a") as f:
                    f.write(text + "\n")
    # the gate: 4096 distinct presets
    lanes = [l for l in lines if l.get("step") == "lanes" and l.get("streams") == 4096]
    groups = [l for l in lines if l.get("step") == "groups"]
    if not lanes or not groups:
        print(json.dumps({"bench": "lane_chain", "gate": "not checked: needs a 4096-stream lanes line and a groups line"}), flush=True)
        return 1
    lane_ms = min(lanes[-1]["wall_ms_per_call"])
    group_ms = groups[-1]["scaled_engine_wall_ms"]["4096"]
    verdict = {"bench": "lane_chain", "gate": "lane chain faster than the group route at 4096 distinct presets", "group_route_tree": groups[-1]["tree"],
               "lane_chain_ms": lane_ms, "group_route_ms": group_ms, "passed": lane_ms < group_ms}
    print(json.dumps(verdict), flush=True)
    with out.open("a") as f:
        f.write(json.dumps(verdict) + "\n")
    return 0 if verdict["passed"] else 1


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=["lanes", "short", "groups"], default=None)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--presets", type=int, default=64, help="groups: distinct presets of the measured chunk (x 64 packed streams)")
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--operator", action="store_true", help="groups: also time simulate_auto_eq_chain_batch on host arrays")
    ap.add_argument("--groups-only", action="store_true")
    ap.add_argument("--run-presets", type=int, default=1024, help="groups: a count that is run chunk by chunk, not scaled (0: none)")
    ap.add_argument("--root", type=pathlib.Path, default=HERE)
    ap.add_argument("--label", default="this build", help="how the lines name the measured tree")
    ap.add_argument("--gate-against", default=None, metavar="FILE", help="--groups-only: the lines file that holds the 4096-stream lanes line")
    ap.add_argument("--out", default=str(HERE / "profiles" / "lane_chain_bench.jsonl"))
    args = ap.parse_args()
    if args.step is None:
        return drive(args)
    paths(args.root.resolve())
    import torch  # noqa: F401  (first: it bundles its own HIP runtime, tests/conftest.py)

    line = step_groups(args) if args.step == "groups" else step_lanes(args, args.step == "short")
    print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
