"""Cost of the output writer: 4096 streams, device pointers, 10 s of audio pushed as blocks of 480 and of 8192 frames, with
the limiter on and off.  The queue fills are spread so that the ratios cover the whole range (starved streams at 0.96
through the emergency 1.06) and a share of the streams writes short.  One JSON line per case: the kernel time of all passes
(HIP events, af_output_writer_last_kernel_ms, summed over the run's pushes; best of --steps runs after a warm-up) beside
two bounds: HBM (4 B read + 4 B written per frame, plus the scratch rows of this cut: the shaped block written and read
twice, the gain row written, rewritten and read) at the chip's 8 TB/s, and the serial chain of the gain pass (about four
dependent f32 operations per frame per stream, whatever the batch).  The serial figure is an ESTIMATE: the cycles per
dependent operation below are assumed, not measured.  The time of each pass is reported beside the total.

The kernel times are read after every push, so the host waits for each push: the run times the kernels, it does not
exercise the asynchronous path.  The output frames behind the bounds are read back for each of the first pushes, while the
drift EMA settles, and taken as constant after that.

    python tools/bench_output_writer.py [--streams 4096] [--seconds 10] [--steps 3]
"""
from __future__ import annotations

import argparse
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "audio-forge_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak
CLOCK_HZ = 2.4e9          # peak engine clock
DEPENDENT_OP_CYCLES = 8   # ASSUMED, not measured: cycles between dependent f32 VALU operations of one wave
SETTLE_PUSHES = 48        # 0.85 ** 48 < 1e-3: the EMA, and with it every stream's out_len, has settled


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()
    import torch

    from mic_eq_mi import mic_eq_core as core

    B, period, rate = args.streams, 48_000, 48_000
    cfg = core.output_writer_default_config(rate)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = (torch.randn(B, period, device="cuda", generator=g) * 0.35).contiguous()  # peaks pass the ceiling now and then
    # fills: from empty over the target centre to past the hard backlog; every 16th stream has a nearly full queue
    lane = torch.arange(B, device="cuda", dtype=torch.int64)
    fill = (lane % 15) * (cfg["hard_backlog"] + 200) // 14
    fill = torch.where(lane % 16 == 15, torch.full_like(fill, cfg["queue_capacity"] - 100), fill).contiguous()
    written = torch.zeros(B, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    total = int(args.seconds * rate)
    for frames in (480, 8192):
        starts = [(k * frames) % (period - frames) for k in range(total // frames)]
        for limiter in (True, False):
            best = None
            for _ in range(args.steps + 1):  # the first run is warm-up
                w = core.OutputWriter(rate, B)
                w.set_limiter(limiter, 0.84)
                width = w.max_output_frames(frames)
                y = torch.empty(B, width, device="cuda")
                ms, passes, out_total, out_frames = 0.0, [0.0] * 5, 0, 0
                for k, at in enumerate(starts):
                    w.push_device(x.data_ptr() + at * 4, frames, period, fill.data_ptr(), False, y.data_ptr(), width, width,
                                  written.data_ptr(), stream)
                    ms += w.last_kernel_ms()  # (waits for the push)
                    passes = [a + b for a, b in zip(passes, w.last_pass_ms())]
                    if k < SETTLE_PUSHES:
                        out_frames = int(w.meters()["out_len"].sum())
                    out_total += out_frames
                w.close()
                if best is None or ms < best[0]:
                    best = (ms, passes)
            pushed = len(starts) * frames
            # per output frame: caller's row 4 B out, shaped row 4 B out + 8 B in, gain row 4 + 4 B out and 4 + 4 B in (limiter on)
            per_out = 4 + 12 + (16 if limiter else 0)
            hbm_ms = (pushed * B * 4 + out_total * per_out) / HBM_BYTES_PER_S * 1e3
            serial_ms = (out_total / B) * 4 * DEPENDENT_OP_CYCLES / CLOCK_HZ * 1e3 if limiter else 0.0
            print(json.dumps(dict(bench="output_writer", streams=B, block_frames=frames, pushes=len(starts), limiter=limiter,
                                  audio_seconds=round(pushed / rate, 3), kernel_ms=round(best[0], 3),
                                  pass_ms=dict(zip(("plan", "shape", "gain", "out", "finish"), (round(v, 3) for v in best[1]))),
                                  hbm_bound_ms=round(hbm_ms, 3), gain_serial_estimate_ms=round(serial_ms, 3))), flush=True)


if __name__ == "__main__":
    main()
