"""Cost of the streaming product resampler: 4096 streams x 10 s at 44.1 -> 48 kHz on one GPU.

  (a) one push of the whole clip, against the one-shot kernel on the same job in the same session (the yardstick: the same
      FMAs; the streaming form moves f32 instead of f64 audio)
  (b) the same clip in pushes of 441 frames, the 10 ms wake-up of a 44.1 kHz device
  (c) the engine's dynamics chain through af_engine_stream_host, one-second calls, with and without the I/O resamplers
      (host buffers: the figure includes the copies to and from the device on both sides of the comparison)

Prints one JSON line per case.  Usage: python tools/bench_resampler_stream.py [--streams N] [--seconds S] [--cases abc]
"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "audio-forge_amd"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mic_eq_mi import mic_eq_core as core  # noqa: E402

FI, FO = 44_100, 48_000


def emit(**row):
    print(json.dumps(row), flush=True)


def case_a(streams, n, reps):
    stream = torch.cuda.current_stream().cuda_stream
    x32 = torch.randn(streams, n, dtype=torch.float32, device="cuda") * 0.1
    r = core.StreamResampler(FI, FO, n_streams=streams)
    n_out = r.output_frames(n)
    y32 = torch.empty(streams, n_out, dtype=torch.float32, device="cuda")
    ms = []
    for _ in range(reps + 1):
        r.reset()
        r.push_device(x32.data_ptr(), n, n, y32.data_ptr(), n_out, n_out, stream)
        torch.cuda.synchronize()
        ms.append(r.last_kernel_ms())
    r.close()
    emit(case="a_stream_one_push", streams=streams, frames_in=n, frames_out=n_out, kernel_ms=[round(v, 3) for v in ms[1:]],
         audio_bytes=streams * (n + n_out) * 4, f64_fma=streams * n_out * 512)
    del y32
    x64 = x32.double()
    del x32
    one = core.Resampler(FI, FO)
    m_out, _ = one.plan(n)
    y64 = torch.empty(streams, m_out, dtype=torch.float64, device="cuda")
    ms = []
    for _ in range(reps + 1):
        one.process_device(x64.data_ptr(), y64.data_ptr(), n, streams, n, m_out, stream)
        torch.cuda.synchronize()
        ms.append(one.last_kernel_ms())
    one.close()
    emit(case="a_one_shot_yardstick", streams=streams, frames_in=n, frames_out=m_out, kernel_ms=[round(v, 3) for v in ms[1:]],
         audio_bytes=streams * (n + m_out) * 8, f64_fma=streams * m_out * 512)


def case_b(streams, n, reps):
    stream = torch.cuda.current_stream().cuda_stream
    x = torch.randn(streams, n, dtype=torch.float32, device="cuda") * 0.1
    r = core.StreamResampler(FI, FO, n_streams=streams)
    cap = 2 * r.output_frames(1024) + 8
    y = torch.empty(streams, cap, dtype=torch.float32, device="cuda")
    wake = 441
    walls = []
    for _ in range(reps + 1):
        r.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        made = 0
        for at in range(0, n - wake + 1, wake):
            made += r.push_device(x.data_ptr() + 4 * at, wake, n, y.data_ptr(), cap, cap, stream)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
    r.close()
    emit(case="b_stream_441_frame_pushes", streams=streams, pushes=n // wake, frames_out=made, wall_ms=[round(v, 2) for v in walls[1:]],
         wall_ms_per_push=round(float(np.mean(walls[1:])) / (n // wake), 4))


def case_c(streams, seconds, reps):
    import bench  # the flagship's chain configuration

    def run(rate):
        eng = core.Engine(48_000.0, streams)
        settings = dict(bench.CHAIN_SETTINGS)
        core.configure_auto_eq_chain(eng, 48_000.0, bench.BANDS, settings)
        eng.set_io_sample_rates(rate, rate)
        rng = np.random.default_rng(1)
        x = (rng.standard_normal((streams, rate)) * 0.1).astype(np.float32)  # one second, reused
        walls = []
        for _ in range(reps + 1):
            eng.reset()
            t0 = time.perf_counter()
            frames = 0
            for _s in range(int(seconds)):
                frames += eng.stream(x).shape[1]
            walls.append((time.perf_counter() - t0) * 1e3)
        eng.close()
        return walls[1:], frames

    base, frames0 = run(48_000)
    emit(case="c_engine_dynamics_48k_io", streams=streams, seconds=seconds, frames_out=frames0, wall_ms=[round(v, 1) for v in base])
    with_rs, frames1 = run(FI)
    emit(case="c_engine_dynamics_44k1_io", streams=streams, seconds=seconds, frames_out=frames1, wall_ms=[round(v, 1) for v in with_rs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", type=str, default="abc")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU: there is no CPU path to time")
    n = int(round(args.seconds * FI))
    if "a" in args.cases:
        case_a(args.streams, n, args.reps)
    if "b" in args.cases:
        case_b(args.streams, n, args.reps)
    if "c" in args.cases:
        case_c(args.streams, args.seconds, args.reps)


if __name__ == "__main__":
    main()
