"""Cost of the room-noise reference analysis: --pairs capture pairs of --noise-seconds of room tone and --voice-seconds of voice
at 48 kHz resident on the device, measured through af_noise_reference_analyze_device.  Reported, not gated.  --processes child
processes one after the other, each --steps + 1 calls with the first discarded; one JSON line per process: wall ms per call
(device events around the call, which include the host's decisions and copies between the kernels), the kernels' ms per stage
(af_noise_reference_last_kernel_ms: sample statistics and chunk sums, frame powers, frame spectra with the band sums, column
medians), capture pairs per second, and next to the frame-spectra time what the transform costs under three models: f64 flops
(8 M (p - 1) per radix-p stage, 12 N to load and window, 22 per bin for the real-input step), LDS bytes (every stage reads
and writes the M points once, 32 M bytes) and HBM bytes (the frame's samples and window once, its PSD row written once).

    python tools/bench_noise_reference.py [--pairs 4096] [--noise-seconds 3] [--voice-seconds 10] [--steps 3] [--processes 3]
"""
from __future__ import annotations

import argparse
import json
import pathlib
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "audio-forge_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

FS = 48_000
HBM_BYTES_PER_S = 8.0e12     # MI355X HBM3E peak
F64_FLOPS_PER_S = 78.6e12    # vector f64 peak
LDS_BYTES_PER_S = 256 * 128 * 2.4e9  # 256 CUs x 128 B a clock at 2.4 GHz


def factors(M: int) -> list[int]:
    out = []
    for p in (7, 5, 3, 2):
        while M % p == 0:
            out.append(p)
            M //= p
    return out


def run(args) -> None:
    import torch

    from mic_eq_mi import mic_eq_core as core

    B = args.pairs
    n_noise, n_voice = int(args.noise_seconds * FS), int(args.voice_seconds * FS)
    g = torch.Generator(device="cuda").manual_seed(23)
    t = torch.arange(n_voice, device="cuda", dtype=torch.float32) / FS
    rate = 0.5 + 0.4 * torch.rand(B, 1, device="cuda", generator=g)  # an on/off envelope below 1 Hz per stream
    phase = torch.rand(B, 1, device="cuda", generator=g)
    noise = torch.empty(B, n_noise, device="cuda")
    voice = torch.empty(B, n_voice, device="cuda")
    for s0 in range(0, B, 256):  # in slices: the generator's temporaries stay small
        b = min(256, B - s0)
        envelope = (torch.sin(2 * torch.pi * (rate[s0:s0 + b] * t + phase[s0:s0 + b])) > 0.3).float()
        noise[s0:s0 + b] = torch.randn(b, n_noise, device="cuda", generator=g) * 0.003
        voice[s0:s0 + b] = torch.randn(b, n_voice, device="cuda", generator=g) * (0.1 * envelope + 0.003)
    torch.cuda.synchronize()
    nr = core.NoiseReference(FS)
    N, noise_frames = nr.frame_size, nr.frames(n_noise)
    M = N // 2
    pointers = (noise.data_ptr(), n_noise, B, n_noise, voice.data_ptr(), n_voice, n_voice)
    wall, stages, r = [], [], None
    for step in range(args.steps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = nr.analyze(None, device_pointers=pointers)
        b.record()
        torch.cuda.synchronize()
        if step:  # the first repetition is discarded
            wall.append(a.elapsed_time(b))
            stages.append(nr.last_kernel_ms())
    nr.close()
    frames = int(B * noise_frames + r["in_capture_noise_frame_count"][r["has_in_capture_spectrum"] == 1].sum())
    best = min(stages, key=lambda s: sum(s.values()))
    flops = frames * (8.0 * M * sum(p - 1 for p in factors(M)) + 12.0 * N + 22.0 * (M + 1))
    lds = frames * 32.0 * M * (len(factors(M)) + 1)
    hbm = frames * (4.0 * N + 8.0 * N + 8.0 * (M + 1))
    fft_s = best["frame_spectra"] * 1e-3
    print(json.dumps({"bench": "noise_reference", "pairs": B, "noise_seconds": args.noise_seconds, "voice_seconds": args.voice_seconds,
                      "frame": N, "factors": factors(M), "frames_transformed": frames,
                      "statuses": [int((r["status"] == k).sum()) for k in range(3)],
                      "streams_with_in_capture_spectrum": int(r["has_in_capture_spectrum"].sum()),
                      "ms_per_call": [round(v, 2) for v in wall],
                      "kernel_ms_per_stage": [{k: round(v, 3) for k, v in s.items()} for s in stages],
                      "kernel_ms": [round(sum(s.values()), 2) for s in stages],
                      "pairs_per_s": round(B / (min(wall) * 1e-3)),
                      "pairs_per_s_kernels_only": round(B / (sum(best.values()) * 1e-3)),
                      "frame_spectra": {"ms": round(best["frame_spectra"], 3), "gflop": round(flops / 1e9, 2), "lds_gb": round(lds / 1e9, 2),
                                        "hbm_gb": round(hbm / 1e9, 2), "f64_fraction_of_peak": round(flops / fft_s / F64_FLOPS_PER_S, 4),
                                        "lds_fraction_of_peak": round(lds / fft_s / LDS_BYTES_PER_S, 4),
                                        "hbm_fraction_of_peak": round(hbm / fft_s / HBM_BYTES_PER_S, 4)}}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--noise-seconds", type=float, default=3.0)
    ap.add_argument("--voice-seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        run(args)
        return
    for _ in range(args.processes):  # a fresh process each: code-object load and first allocations are in the discarded call
        forward = [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("pairs", "noise_seconds", "voice_seconds", "steps")]
        subprocess.run([sys.executable, __file__, "--child", *forward], check=True)


if __name__ == "__main__":
    main()
