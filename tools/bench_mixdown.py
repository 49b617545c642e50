"""Cost of the input mixdown: 4096 stereo streams, device pointers, 10 s of audio pushed as callbacks of 480 and of 8192
frames, in each mode.  One JSON line per case: the kernel time of the decision passes and of the mix passes (HIP events,
af_mixdown_last_kernel_ms, summed over the run's callbacks; best of --steps runs after a warm-up) and the mix pass's share
of its HBM bound (8 B read + 4 B written per frame over the chip's 8 TB/s).  The material is one second per stream, pushed
cyclically (the state carries on): a third of the streams coherent, a third with the right channel 3 frames late, a third
in anti-phase, so that all three mixes of the phase-safe mode run.  Then the full-chain call through the engine with stereo
phase-safe input against mono input: wall time of Engine.stream on host arrays of --engine-seconds, the same session.

    python tools/bench_mixdown.py [--streams 4096] [--seconds 10] [--steps 3]
"""
from __future__ import annotations

import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "audio-forge_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--engine-seconds", type=float, default=1.0)
    args = ap.parse_args()
    import torch

    import signals as S
    from mic_eq_mi import mic_eq_core as core

    B, period = args.streams, 48_000
    g = torch.Generator(device="cuda").manual_seed(7)
    left = torch.randn(B, period + 8, device="cuda", generator=g) * 0.2
    kind = torch.arange(B, device="cuda") % 3
    right = torch.where(kind[:, None] == 0, left[:, 8:] * 0.8, torch.where(kind[:, None] == 1, left[:, 5:period + 5], -left[:, 8:]))
    x = torch.stack([left[:, 8:], right], dim=2).contiguous()  # [B, period, 2]
    y = torch.empty(B, 8192, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    total = int(args.seconds * 48_000)
    for frames in (480, 8192):
        starts = [(k * frames) % (period - frames) for k in range(total // frames)]
        for mode in ("average", "left", "right", "max_rms", "phase_safe_mono"):
            best = None
            for _ in range(args.steps + 1):  # the first run is warm-up
                m = core.Mixdown(2, mode, n_streams=B)
                dec = mix = 0.0
                for at in starts:
                    m.push_device(x.data_ptr() + at * 8, frames, period, y.data_ptr(), 8192, stream)
                    a, b = m.last_kernel_ms()
                    dec, mix = dec + a, mix + b
                m.close()
                if best is None or dec + mix < best[0] + best[1]:
                    best = (dec, mix)
            pushed = len(starts) * frames
            bound_ms = pushed * B * 12 / HBM_BYTES_PER_S * 1e3
            print(json.dumps(dict(bench="mixdown", streams=B, channels=2, mode=mode, callback_frames=frames, callbacks=len(starts),
                                  audio_seconds=round(pushed / 48_000, 3), decision_ms=round(best[0], 3), mix_ms=round(best[1], 3),
                                  mix_hbm_bound_ms=round(bound_ms, 3), mix_share_of_hbm_bound=round(bound_ms / best[1], 3))),
                  flush=True)
    # the engine: front end + dynamics chain, one call of --engine-seconds from host arrays
    n = int(args.engine_seconds * 48_000) // 480 * 480
    stereo = x[:, :n].cpu().numpy()
    mono = stereo[:, :, 0].copy()
    for channels in (1, 2):
        eng = core.Engine(48_000.0, B)
        core.configure_auto_eq_chain(eng, 48_000.0, S.LIMITER_BANDS, S.limiter_settings(2.0))
        eng.set_prefilter_enabled(1, 1)
        if channels == 2:
            eng.set_input_channels(2, "phase_safe_mono")
        best = None
        for _ in range(args.steps + 1):
            t0 = time.perf_counter()
            eng.stream(stereo if channels == 2 else mono)
            dt = (time.perf_counter() - t0) * 1e3
            best = dt if best is None else min(best, dt)
        eng.close()
        print(json.dumps(dict(bench="mixdown_engine_call", streams=B, input_channels=channels,
                              mode="phase_safe_mono" if channels == 2 else None, frames=n, stream_call_wall_ms=round(best, 2))),
              flush=True)


if __name__ == "__main__":
    main()
