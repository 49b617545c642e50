"""Cost of the speech-feature measurement: --pairs capture pairs of --noise-seconds of room tone and --voice-seconds of voice at
--fs (48 kHz by default) resident on the device, measured through af_speech_features_analyze_device -- at any other rate through
af_device_rate_features_analyze_device, whose "resampling" stage (resample_poly of signal and mask to 48 kHz) is reported beside
the K-weighting it feeds.  Reported, not gated.  --processes child
processes one after the other, each --steps + 1 calls with the first discarded; one JSON line per process: wall ms per call
(device events around the call, which include the host's decisions and copies between the kernels), the kernels' ms per stage
(af_speech_features_last_kernel_ms: frame powers, K-weighting, frame spectra, medians over frames, weighted peak), capture
pairs per second, and next to the frame-spectra time what sf_frame_kernel costs under three models: f64 flops (8 M (p - 1) per
radix-p stage, 12 N to centre and window, 22 per bin for the real-input step, S^2 compares for the rank selection over the S
sibilance bins), LDS bytes (every stage reads and writes the M points once, 32 M bytes; the selection reads 8 S^2) and HBM
bytes (the frame's samples and window once, the sibilance row and the band record written once).  The K-weighting kernel is
set against it as dependent f64 operations per sample and lane.

    python tools/bench_speech_features.py [--fs 48000] [--pairs 4096] [--noise-seconds 3] [--voice-seconds 10] [--steps 3] [--processes 3]
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



def factors(m: int) -> tuple:
    """nr_make_plan's factor list of the half-frame: the largest radix first."""
    out = []
    for p in (7, 5, 3, 2):
        while m % p == 0:
            out.append(p)
            m //= p
    return tuple(out)


HBM_BYTES_PER_S = 8.0e12     # MI355X HBM3E peak
F64_FLOPS_PER_S = 78.6e12    # vector f64 peak
LDS_BYTES_PER_S = 256 * 128 * 2.4e9  # 256 CUs x 128 B a clock at 2.4 GHz
KWEIGHT_OPS_PER_SAMPLE = 18  # two sections of 5 multiplies and 4 additions; the square and its addition come on top


def kweight_streams_per_workgroup(n_streams: int) -> int:
    """launch_sf_kweight's choice: 64, or down to 16 while that leaves fewer workgroups than the 256 compute units."""
    per = 64
    while per > 16 and -(-n_streams // per) < 256:
        per //= 2
    return per


def run(args) -> None:
    import torch

    from mic_eq_mi import mic_eq_core as core

    B, FS = args.pairs, args.fs
    M = int(FS * 20 / 1000.0)
    N, FACTORS = 2 * M, factors(M)
    n_noise, n_voice = int(args.noise_seconds * FS), int(args.voice_seconds * FS)
    g = torch.Generator(device="cuda").manual_seed(29)
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
    level = [-50.0] * B
    sf = core.SpeechFeatures(FS, B, n_voice, n_noise, device_rate=FS != 48_000)
    S = sf.sibilance_bins
    pointers = (voice.data_ptr(), n_voice, B, n_voice, noise.data_ptr(), n_noise, n_noise)
    wall, stages, r = [], [], None
    for step in range(args.steps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = sf.analyze(None, level, device_pointers=pointers)
        b.record()
        torch.cuda.synchronize()
        if step:  # the first repetition is discarded
            wall.append(a.elapsed_time(b))
            stages.append(sf.last_kernel_ms())
    noise_frames, sf_n48 = sf.frames(n_noise), sf.resampled_length(n_voice)
    sf.close()
    speech_frames = int(r["spectral_frames"].sum())
    frames = speech_frames + B * noise_frames
    best = min(stages, key=lambda s: sum(s.values()))
    flops = frames * (8.0 * M * sum(p - 1 for p in FACTORS) + 12.0 * N + 22.0 * (M + 1)) + speech_frames * 2.0 * S * S
    lds = frames * 32.0 * M * (len(FACTORS) + 1) + speech_frames * 8.0 * S * S
    hbm = frames * (4.0 * N + 8.0 * N) + speech_frames * 8.0 * (S + 8 + 2)
    fft_s, kw_s = best["frame_spectra"] * 1e-3, best["k_weighting"] * 1e-3
    resampling = {}
    if "resampling" in best:
        n48 = sf_n48
        resampling = {"resampling": {"ms": round(best["resampling"], 3), "samples_out": n48,
                                     "ns_per_output_sample_and_stream": round(best["resampling"] * 1e6 / (n48 * B), 4),
                                     "ratio_to_k_weighting": round(best["resampling"] / best["k_weighting"], 3)}}
    print(json.dumps({"bench": "speech_features", "fs": FS, "pairs": B, "noise_seconds": args.noise_seconds, "voice_seconds": args.voice_seconds,
                      "frame": N, "factors": list(FACTORS), "frames_transformed": frames, "speech_frames_listed": speech_frames,
                      "streams_with_evidence": int(r["evidence_available"].sum()), "non_finite_streams": int(r["non_finite"].sum()),
                      "ms_per_call": [round(v, 2) for v in wall],
                      "kernel_ms_per_stage": [{k: round(v, 3) for k, v in s.items()} for s in stages],
                      "kernel_ms": [round(sum(s.values()), 2) for s in stages],
                      "pairs_per_s": round(B / (min(wall) * 1e-3)),
                      "pairs_per_s_kernels_only": round(B / (sum(best.values()) * 1e-3)),
                      "frame_spectra": {"ms": round(best["frame_spectra"], 3), "gflop": round(flops / 1e9, 2), "lds_gb": round(lds / 1e9, 2),
                                        "hbm_gb": round(hbm / 1e9, 2), "f64_fraction_of_peak": round(flops / fft_s / F64_FLOPS_PER_S, 4),
                                        "lds_fraction_of_peak": round(lds / fft_s / LDS_BYTES_PER_S, 4),
                                        "hbm_fraction_of_peak": round(hbm / fft_s / HBM_BYTES_PER_S, 4)},
                      "k_weighting": {"ms": round(best["k_weighting"], 3), "workgroups": -(-B // kweight_streams_per_workgroup(B)),
                                      "ns_per_sample_and_lane": round(kw_s / n_voice * 1e9, 2),
                                      "dependent_f64_ops_per_sample": KWEIGHT_OPS_PER_SAMPLE,
                                      "ratio_to_frame_spectra": round(best["k_weighting"] / best["frame_spectra"], 3)}, **resampling}),
          flush=True)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--fs", type=int, default=48_000)
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
        forward = [f"--{k.replace('_', '-')}={getattr(args, k)}" for k in ("fs", "pairs", "noise_seconds", "voice_seconds", "steps")]
        subprocess.run([sys.executable, __file__, "--child", *forward], check=True)


if __name__ == "__main__":
    main()
