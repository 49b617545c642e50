#!/usr/bin/env python3
"""Record what the loaded build of supp_pitchsearch4_kernel gives on the stimulus of tests/pitch_search_forms_stimulus.py:
the stand-alone search tap (af_suppressor_debug_pitch_search) on every part -- the synthetic spans at 1, 3, 4 and 6 frames,
the 31 x 43 model-input stimulus, the single-frame steering spans -- into an .npz with, per part, the search's own index of
every cell as int16 and a 64-bit hash of every cell's whitened buffer.

    python tools/record_pitch_search.py [--out tests/golden/pitch_search_parent.npz]

tests/golden/pitch_search_parent.npz is taken ONCE, on an MI355X, from a build of the commit BEFORE a change of the search
kernel (AF_LIB_PATH names another build of the library); tests/test_gpu_pitch_search_forms.py holds later builds to it bit
for bit.  Needs a GPU.
"""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
for p in (ROOT / "tests", ROOT / "audio-forge_amd"):
    sys.path.insert(0, str(p))


def record() -> dict:
    import mic_eq_mi
    import pitch_search_forms_stimulus as F

    if not mic_eq_mi.CORE_AVAILABLE:
        raise RuntimeError("libaudioforge_mi.so is missing: build it first")
    out = {}
    for name, spans, frames in F.parts():
        ds, index = mic_eq_mi.Engine.suppressor_debug_pitch_search(spans)
        assert ds.shape == (frames, spans.shape[0], 864) and index.shape == ds.shape[:2]
        assert int(index.min()) >= -32768 and int(index.max()) <= 32767
        out[f"{name}_index"] = index.astype(np.int16)
        out[f"{name}_hash"] = F.buffer_hashes(ds)
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "pitch_search_parent.npz"))
    args = ap.parse_args()
    rec = record()
    np.savez_compressed(args.out, **rec)
    cells = sum(v.size for k, v in rec.items() if k.endswith("_index"))
    print(f"recorded {cells} cells in {len(rec) // 2} parts -> {args.out}")


if __name__ == "__main__":
    main()
