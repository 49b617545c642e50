"""bench.py on the MI355X at a small shape: a plain run prints the headline line without the CPU baseline, `--full` adds it,
and `--dump-outputs` writes the same outputs from both (the timed path and its input do not depend on --full)."""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--streams", "256", "--seconds", "1"]


def _bench(extra, out):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    proc = subprocess.run([sys.executable, str(ROOT / "bench.py"), *ARGS, *extra, "--dump-outputs", str(out)],
                          capture_output=True, text=True, env=env, timeout=600)
    assert proc.returncode == 0, proc.stderr[-3000:]
    line = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][0])
    return line, {p.stem: np.load(p) for p in sorted(out.glob("*.npy"))}


def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    plain, a = _bench([], tmp_path / "plain")
    full, b = _bench(["--full"], tmp_path / "full")
    for line in (plain, full):
        assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
        assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert "cpu_baseline" not in plain
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["single_thread"]["value"] > 0
    assert sorted(a) == ["block_stats", "output_audio_columns", "output_audio_streams"] == sorted(b)
    assert sum(arr.nbytes for arr in a.values()) <= 64 << 20
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.array_equal(a[name], b[name]), name
    # a real chain ran: the sampled streams are audio, and their block peaks stay under the line's own maximum
    audio = a["output_audio_streams"]
    assert 1 <= audio.shape[0] <= 256 and audio.shape[1] == 48_000
    assert np.all(np.isfinite(audio)) and float(np.sqrt(np.mean(audio ** 2))) > 0.01
    assert a["output_audio_columns"].shape[0] == 256
    assert float(np.max(np.abs(audio))) <= plain["checks"]["output_sample_peak"] + 1e-7
