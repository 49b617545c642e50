"""Cost of the noise gate stage: 4096 streams x 10 s with the gate off and on, for the full realtime chain (front end +
suppressor + dynamics) and for the dynamics chain without the suppressor.  One JSON line per case: the call's kernel time
(af_engine_last_kernel_ms) and its split at the pre-pass | chain boundary (af_engine_last_stage_ms).  --fused adds the
VAD-fused modes (controller attached, mode 1 and 2, one shared probability per control block that follows the talk spurts):
"gate": "fused1" / "fused2", beside the expander path ("gate": 1) of the same run.

    python tools/bench_gate.py [--streams 4096] [--seconds 10] [--steps 3] [--fused]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[1]
for p in (ROOT, ROOT / "audio-forge_amd", ROOT / "tests"):
    sys.path.insert(0, str(p))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--fused", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch

    import signals as S
    from mic_eq_mi import mic_eq_core as core

    n = int(args.seconds * 48_000) // 480 * 480
    t = torch.arange(n, device="cuda", dtype=torch.float64) / 48_000.0
    f = 150.0 + 13.0 * torch.arange(args.streams, device="cuda", dtype=torch.float64)[:, None] % 17
    env = torch.where(((t + 0.037) % 2.0) < 1.0, 0.2, 0.002)  # talk and pauses: the gate opens and closes
    x = (env * torch.sin(2 * torch.pi * f * t)).to(torch.float32).contiguous()
    del t, f
    y = torch.empty_like(x)
    stream = torch.cuda.current_stream().cuda_stream
    for chain in ("full", "dynamics"):
        for gate in (0, 1) + (("fused1", "fused2") if args.fused else ()):
            eng = core.Engine(48_000.0, args.streams)
            core.configure_auto_eq_chain(eng, 48_000.0, S.LIMITER_BANDS, S.limiter_settings(2.0))
            eng.set_prefilter_enabled(1, 1)
            if chain == "full":
                eng.set_suppressor_enabled(1)
            eng.set_gate_enabled(int(gate != 0))
            prob = None
            if isinstance(gate, str):
                eng.gate_set_vad_auto_gate_enabled(1)
                eng.gate_set_mode(int(gate[-1]))
                tb = (np.arange(-(-n // 960)) + 0.5) * 960 / 48_000.0  # (configure_auto_eq_chain: control blocks of 960)
                prob = np.where(((tb + 0.037) % 2.0) < 1.0, 0.9, 0.05).astype(np.float32)
            eng.set_timing_enabled(1)
            best = None
            for _ in range(args.steps + 1):  # the first call is warm-up
                if prob is not None:
                    eng.gate_set_vad_evidence(prob, np.ones(prob.size, bool))
                eng.process_device(x.data_ptr(), y.data_ptr(), n, n, 0, stream)
                torch.cuda.synchronize()
                ms, launches = eng.last_kernel_ms()
                pre, ch = C.c_double(0.0), C.c_double(0.0)
                eng._lib.af_engine_last_stage_ms(eng._h, C.byref(pre), C.byref(ch))
                row = (ms, pre.value, ch.value, launches)
                best = row if best is None or (_ > 0 and row[0] < best[0]) else best
                if _ == 0:
                    best = None
            eng.close()
            print(json.dumps({"chain": chain, "gate": gate, "streams": args.streams, "seconds": n / 48_000.0,
                              "kernel_ms": round(best[0], 2), "prepass_ms": round(best[1], 2), "chain_ms": round(best[2], 2),
                              "launches": best[3]}), flush=True)


if __name__ == "__main__":
    main()
