"""Cost of the voice spectrum measurement: --streams captures of --seconds at nperseg 4096 resident on the device, measured
through af_voice_spectrum_analyze_device.  Reported, not gated.  --processes child processes one after the other, each
--steps + 1 calls with the first discarded; one JSON line per process: wall ms per call (device events around the call, which
include the host's decisions and copies between the kernels), the kernels' own ms (af_voice_spectrum_last_kernel_ms), frames
per second, and the share of the HBM peak the kernels reach under a traffic model: the audio read about twice (50 % overlap,
once for the window spectra, once for Welch, plus the energy pass: 2.5 x) and every window-spectrum row written once and read
by the median's passes at least once.  --reliability also computes the second half of analyze_voice_spectrum (the robust
median and the reliability statistics) and reports each new kernel's ms and share of the call's kernel time (events around
every launch, af_voice_spectrum_last_reliability_kernel_ms) next to the kernels' ms of a call with the option off.

    python tools/bench_voice_spectrum.py [--streams 4096] [--seconds 10] [--nperseg 4096] [--steps 3] [--processes 3] [--reliability]
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

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak


def run(args) -> None:
    import torch

    from mic_eq_mi import mic_eq_core as core

    B, fs, N = args.streams, 48_000, args.nperseg
    n = int(args.seconds * fs)
    g = torch.Generator(device="cuda").manual_seed(11)
    t = torch.arange(n, device="cuda", dtype=torch.float32) / fs
    rate = 0.7 + 0.6 * torch.rand(B, 1, device="cuda", generator=g)  # an on/off envelope near 1 Hz per stream
    phase = torch.rand(B, 1, device="cuda", generator=g)
    envelope = (torch.sin(2 * torch.pi * (rate * t + phase)) > -0.2).float()
    audio = torch.empty(B, n, device="cuda")
    for s0 in range(0, B, 256):  # in slices: the generator's temporaries stay small
        audio[s0:s0 + 256] = torch.randn(min(256, B - s0), n, device="cuda", generator=g) * (0.1 * envelope[s0:s0 + 256] + 0.001)
    del envelope
    torch.cuda.synchronize()
    vs = core.VoiceSpectrum(fs, N)
    F, K = vs.frames(n), vs.bins
    pointers = (audio.data_ptr(), n, B, n)
    wall, kernel, shares, rows = [], [], [], 0
    for step in range(args.steps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = vs.analyze(None, device_pointers=pointers, reliability=args.reliability)
        b.record()
        torch.cuda.synchronize()
        if step:  # the first repetition is discarded
            wall.append(a.elapsed_time(b))
            kernel.append(vs.last_kernel_ms())
            shares.append(vs.last_reliability_kernel_ms())
        voiced = int(r["voiced"].sum())
        rows = voiced + int(((r["noise_reference_source"] == 2) * (F - r["voiced"])).sum())
    extra = {}
    if args.reliability:  # one call with the option off on the same handle: the new kernels' share is the difference
        main_branch = int((r["used_single_spectrum_fallback"] == 0).sum())
        vs.analyze(None, device_pointers=pointers)
        best_step = kernel.index(min(kernel))
        extra = {"reliability": True, "main_branch_streams": main_branch, "kernel_ms_option_off": round(vs.last_kernel_ms(), 2),
                 "reliability_kernel_ms": {k: round(v, 3) for k, v in shares[best_step].items()},
                 "reliability_kernel_share_of_kernels": {k: round(v / kernel[best_step], 4) for k, v in shares[best_step].items()}}
    vs.close()
    traffic = 2.5 * B * n * 4 + 2.0 * rows * K * 8
    best = min(kernel)
    print(json.dumps({"bench": "voice_spectrum", "streams": B, "seconds": args.seconds, "nperseg": N, "frames_per_stream": F,
                      "window_spectra": rows, "ms_per_call": [round(v, 2) for v in wall], "kernel_ms_per_call": [round(v, 2) for v in kernel],
                      "frames_per_s": round(B * F / (min(wall) * 1e-3)), "modelled_traffic_gb": round(traffic / 1e9, 2),
                      "hbm_fraction_of_kernels": round(traffic / (best * 1e-3) / HBM_BYTES_PER_S, 4), **extra}), flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--nperseg", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--reliability", action="store_true")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        run(args)
        return
    for _ in range(args.processes):  # a fresh process each: code-object load and first allocations are in the discarded call
        forward = [f"--{k}={getattr(args, k)}" for k in ("streams", "seconds", "nperseg", "steps")]
        subprocess.run([sys.executable, __file__, "--child", *forward, *(["--reliability"] if args.reliability else [])], check=True)


if __name__ == "__main__":
    main()
