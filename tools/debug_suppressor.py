"""Stage-by-stage comparison of the GPU suppressor against the CPU restatement (development aid: prints, asserts nothing;
tests/test_gpu_suppressor_stages.py is the check).  Both taps come through the helpers the tests use -- af_oracle_py.RnnoiseTap
and Engine.suppressor_debug_read -- so no struct layout is restated here.

    python tools/debug_suppressor.py [frames <= 16]
"""
import sys

sys.path[:0] = ["oracle", "tests", "audio-forge_amd"]
import numpy as np

import af_oracle_py as o
import mic_eq_mi
import signals as S

n_frames = int(sys.argv[1]) if len(sys.argv) > 1 else 6
assert 1 <= n_frames <= 16, "the device tap keeps one suppressor window: at most 16 frames at control block 480"
x = S.kat_signal(n_frames)
ref = o.RnnoiseTap(0x5EED).run(x)  # raw protocol, frame by frame

eng = mic_eq_mi.Engine(48000.0, 1)
eng.set_eq_enabled(0)
eng.set_limiter_enabled(0)
eng.set_suppressor_enabled(1)
eng.suppressor_set_raw_protocol(1)
eng.set_control_block_samples(480)
got = eng.process(x.reshape(1, -1))[0]


def rel(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


for f in range(n_frames):
    d = eng.suppressor_debug_read(f, 0)
    live = not d["silence"]
    print(f"frame {f}: X {rel(d['X'], ref['X'][f]):.2e} Ex {rel(d['Ex'], ref['Ex'][f]):.2e} "
          f"pitch {d['pitch_index']}/{ref['pitch_index'][f]} sil {d['silence']}/{ref['silence'][f]} "
          f"P {rel(d['P'], ref['P'][f]):.2e} Ep {rel(d['Ep'], ref['Ep'][f]):.2e} Exp {rel(d['Exp'], ref['Exp'][f]):.2e} "
          f"feat {float(np.max(np.abs(d['feat'][:42] - ref['features'][f]))):.2e} "
          f"graw {float(np.max(np.abs(d['gains_raw'] - ref['gains_raw'][f]))) if live else 0.0:.2e} "
          f"g {float(np.max(np.abs(d['gains'] - ref['gains'][f]))) if live else 0.0:.2e} "
          f"out {float(np.max(np.abs(got[f * 480:(f + 1) * 480] - ref['out'][f]))):.2e}")
eng.close()
