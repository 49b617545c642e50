"""Every analysis stage of the GPU suppressor, per frame, against the float64 reference of tests/suppressor_stage_ref.py.

The engine's test tap (af_suppressor_debug_read) is read after every call for every frame of 19 of the 69 streams: the rows at
the edges of the 16-stream network tiles and of the two network workgroups (0, 15, 16, 47, 63, 64, 68) and every stream with
a role (tests/suppressor_stage_stimulus.py: silent from the start, silent mid-run across a call boundary, near the silence
threshold, clamped, quiet).  Each stage is computed in float64 from the DEVICE's tap of the stage before it, so an error is
found where it happens; a stage's bound is 4 x the CPU restatement's own worst distance from the same float64 reference on
the same frames (never under 4 f32 epsilons of the metric's scale), computed in the same run -- no figure here is tuned to the
device.  `gains = max(gains_raw, 0.6f x previous gains)`, the pad words feat[42:44] and the zero features of a silent frame
are exact comparisons.

The tap keeps the last suppressor window only, so every call is one window (at most 16 frames at control block 480); each
cell read is checked against the call's (silence, pitch index) trace, which would show a stale cell.

Measured on an MI355X, worst over the 988 cells of the six calls (device | restatement | bound = 4 x the restatement's);
every run prints them (pytest -s):
  X          2.0e-7 | 2.3e-7 | 9.3e-7 of the frame peak      P    2.0e-7 | 2.6e-7 | 1.0e-6
  Ex         2.9e-7 | 2.8e-7 | 1.1e-6 relative               Ep   2.7e-7 | 2.6e-7 | 1.0e-6      Exp  3.0e-7 | 3.1e-7 | 1.2e-6
  features   3.4e-5 | 3.8e-5 | 1.5e-4 (|feature| up to 83)   gains_raw  3.7e-7 | 4.7e-7 | 1.9e-6 (887 live cells)
  output     1.6e-7 | 1.4e-7 | 5.7e-7 of full scale
  loaded blob with -128 / +-127:  gains_raw 7.2e-7 | 7.3e-7 | 2.9e-6,  output 1.9e-7 | 1.7e-7 | 6.6e-7
  wrapper protocol (60 cells):    X 1.4e-7 | 1.7e-7 | 6.8e-7,  features 1.2e-5 | 7.9e-6 | 3.2e-5,  output 1.2e-7 | 1.3e-7 | 5.2e-7
No silence flag, pad word, silent frame's feature or `gains` floor was off.  Mutated builds of the library (never committed;
DESIGN.md 4.5 lists what each test did with them): the last band not doubled, the cepstral ring advanced on silent frames,
the GRU states of silent streams updated, two bytes of one `w4` word swapped -- each fails its stage's test here.
"""
import os

import numpy as np
import pytest

import suppressor_stage_ref as R
import suppressor_stage_stimulus as T

pytestmark = pytest.mark.gpu

SCHEDULE_SWITCHES = ("AF_SUPP_WINDOW_FRAMES", "AF_SUPP_RAMP", "AF_SUPP_RAMP_LIST", "AF_SUPP_RAMP_END")


def _device_run(kind: str) -> dict:
    """The run `kind` of the stimulus module through an engine (suppressor only, control block 480), its tap read after
    every call; the taps held against the float64 reference."""
    import mic_eq_mi

    assert mic_eq_mi.CORE_AVAILABLE
    ref = T.restatement(kind)
    wrapper = kind == "wrapper"
    audio = T.wrapper_batch() if wrapper else T.batch()
    calls = (T.WRAPPER_FRAMES,) if wrapper else T.CALLS
    streams = list(ref["streams"])
    assert np.array_equal(audio[streams], ref["audio"])
    saved = {k: os.environ.pop(k) for k in SCHEDULE_SWITCHES if k in os.environ}
    try:
        eng = mic_eq_mi.Engine(48_000.0, audio.shape[0])
        try:
            eng.set_eq_enabled(0)
            eng.set_limiter_enabled(0)
            eng.set_suppressor_enabled(1)
            eng.set_control_block_samples(480)
            if wrapper:
                eng.set_suppressor_strength(T.WRAPPER_STRENGTH)
            else:
                eng.suppressor_set_raw_protocol(1)
            if kind == "extreme":
                eng.suppressor_load_weights(ref["blob"], len(ref["blob"]))
            eng.suppressor_set_trace_enabled(1)
            cells, outs, call_of, f0 = [], [], [], 0
            for index, n in enumerate(calls):
                out = eng.process(audio[:, f0 * 480:(f0 + n) * 480])
                assert out.shape == (audio.shape[0], n * 480)
                trace = eng.suppressor_trace()
                assert trace.shape[0] == n
                for f in range(n):
                    row = [eng.suppressor_debug_read(f, s) for s in streams]
                    for cell, s in zip(row, streams):  # a call of several windows would leave earlier windows' cells behind
                        assert (cell["silence"], cell["pitch_index"]) == tuple(trace[f, s]), ("stale tap cell", index, f, s)
                    cells.append(row)
                    call_of.append((index, f))
                outs.append(out[streams])
                f0 += n
        finally:
            eng.close()
    finally:
        os.environ.update(saved)
    taps = R.stack_taps(cells)
    out = np.concatenate(outs, axis=1)
    assert np.all(np.isfinite(out))
    result = R.evaluate(ref["model_input"], taps, out, ref["blob"], dry=ref["audio"] if wrapper else None, strength=ref["strength"])
    return {"ref": ref, "taps": taps, "out": out, "result": result, "call_of": call_of, "streams": streams}


_RUNS: dict = {}


@pytest.fixture(scope="module")
def run():
    def get(kind: str) -> dict:
        if kind not in _RUNS:
            _RUNS[kind] = _device_run(kind)
        return _RUNS[kind]

    yield get
    _RUNS.clear()


def _hold(d: dict, stage: str) -> float:
    """Assert the device's worst error of `stage` over every cell read is inside its bound; report where it is."""
    restatement = d["ref"]["result"]
    errors = d["result"]["err"][stage]
    absent = (d["taps"]["silence"] != 0) if stage == "gains_raw" else np.zeros(errors.shape, dtype=bool)  # no gains on a silent frame
    assert np.array_equal(np.isnan(errors), absent), f"{stage}: a cell that was read is left out, or is not a number"
    value, f, s = R.worst(errors)
    limit = R.bound(stage, restatement)
    call, frame = d["call_of"][f]
    print(f"{stage:9s} device {value:.3e} (call {call}, frame {frame}, stream {d['streams'][s]}) | restatement "
          f"{R.worst(restatement['err'][stage])[0]:.3e} | bound {limit:.3e} | {int(np.sum(~np.isnan(errors)))} cells")
    assert value <= limit, (stage, value, limit, call, frame, d["streams"][s])
    return value


def _exact(d: dict, name: str) -> None:
    cells = [(*d["call_of"][f], d["streams"][s]) for f, s in d["result"]["fails"][name]]
    assert cells == [], (name, cells[:8])


def _silent_frames_occurred(d: dict) -> np.ndarray:
    """The silent frames the stimulus was built for did occur on the device: exactly where the restatement has them."""
    sil = d["taps"]["silence"] != 0
    assert np.array_equal(sil, d["ref"]["taps"]["silence"] != 0)
    col = {s: i for i, s in enumerate(d["streams"])}
    for s, role in T.ROLES.items():
        if role in T.SILENT_ROLES or role == "near":
            assert int(sil[:, col[s]].sum()) >= 10, (s, role)
    return sil


def test_spectra(run):
    """X from the f32-restated model input, P the same transform at the device's own pitch index: max |d| / frame peak."""
    d = run("synthetic")
    _silent_frames_occurred(d)
    pitch = d["taps"]["pitch_index"]
    assert np.any(pitch <= 61) and np.any(pitch >= 760)  # both ends of P's window offset
    _hold(d, "X")
    _hold(d, "P")


def test_bands_and_silence_flag(run):
    """Ex, Ep (relative), Exp (absolute) from the device's X and P; the flag against sum(Ex_ref) < 0.04."""
    d = run("synthetic")
    _silent_frames_occurred(d)
    for stage in ("Ex", "Ep", "Exp"):
        _hold(d, stage)
    _exact(d, "near_threshold")  # no frame was left out of the flag check
    _exact(d, "silence_wrong")


def test_features_and_pad_words(run):
    """The 42 features from the device's Ex, Exp and pitch index with the cepstral ring carried in f64 over all six calls;
    zero on a silent frame (and the ring does not move: the first live frame after it would show); pad words exactly 0."""
    d = run("synthetic")
    sil = _silent_frames_occurred(d)
    _hold(d, "feat")
    _exact(d, "pad_nonzero")
    _exact(d, "silent_feat_nonzero")
    after = R.first_frames_after_silence(sil)
    assert len(after) >= 8
    limit = R.bound("feat", d["ref"]["result"])
    assert all(d["result"]["err"]["feat"][f, s] <= limit for f, s in after)


def test_network_and_gain_floor(run):
    """gains_raw against the f64 network built from the int8 blob, fed the device's features, its GRU states carried over
    all 52 frames; gains bit for bit max(gains_raw, 0.6f x previous gains), held across silent frames and calls."""
    d = run("synthetic")
    _silent_frames_occurred(d)
    _hold(d, "gains_raw")
    _exact(d, "gains_floor_wrong")


def test_output_audio(run):
    """pitch_filter, renormalisation, band gains, inverse transform, window, overlap-add in f64 from the device's X, P and
    record, against the engine's output; a silent frame's X goes to the synthesis unmodified."""
    d = run("synthetic")
    _silent_frames_occurred(d)
    _hold(d, "out")


def test_silent_stream_keeps_its_state_beside_active_neighbours(run):
    """Sixteen streams share one matrix-core tile: a silent stream must keep its three GRU states while its neighbours
    update.  On the first live frame after a silence gains_raw must match as well as on any other frame -- and a reference
    that lets the states run through the silence is far outside the bound there, so the check can tell."""
    d = run("synthetic")
    sil = _silent_frames_occurred(d)
    col = {s: i for i, s in enumerate(d["streams"])}
    tile0 = [col[s] for s in d["streams"] if s < 16]
    assert len({tuple(sil[:, i]) for i in tile0}) >= 3 and not sil[:, col[0]].any() and not sil[:, col[15]].any()
    limit = R.bound("gains_raw", d["ref"]["result"])
    after = [(f, s) for f, s in R.first_frames_after_silence(sil) if f > 3]
    assert len(after) >= 8 and {d["streams"][s] for _, s in after} >= {3, 5, 9, 21, 37, 65, 66}
    mutant = R.evaluate(d["ref"]["model_input"], d["taps"], d["out"], d["ref"]["blob"], hold_silent=False)
    for f, s in after:
        assert d["result"]["err"]["gains_raw"][f, s] <= limit, (d["call_of"][f], d["streams"][s])
        assert mutant["err"]["gains_raw"][f, s] > 100 * limit, (d["call_of"][f], d["streams"][s])


def test_loaded_weights_reach_the_network(run):
    """A blob with -128, +-127 and 126 entries through af_suppressor_load_weights: the repack into the padded f32 matrices and
    the byte-packed `w4` operand order must hand the network the same numbers -- the f64 network is built from the same
    bytes.  The blob WITHOUT its extreme entries is far outside the bound, so those entries are seen."""
    d = run("extreme")
    _silent_frames_occurred(d)
    for stage in R.STAGES:
        _hold(d, stage)
    for name in d["result"]["fails"]:
        _exact(d, name)
    import af_oracle_py as oracle

    plain = R.evaluate(d["ref"]["model_input"], d["taps"], d["out"], oracle.rnn_synthetic_weights(0xB10B))
    assert R.worst(plain["err"]["gains_raw"])[0] > 1000 * R.bound("gains_raw", d["ref"]["result"])


def test_wrapper_protocol(run):
    """Not raw: X from scale_sample_for_model of the input (every third stream is in the soft clip), the output with the
    smoothed wet/dry mix at strength 0.6 restated in f32; the run starts with two frames of silence."""
    d = run("wrapper")
    sil = d["taps"]["silence"] != 0
    assert np.array_equal(sil, d["ref"]["taps"]["silence"] != 0) and sil[:2].all() and not sil[3:].any()
    assert float(np.abs(d["ref"]["audio"]).max()) > 1.0 and float(np.abs(d["ref"]["model_input"]).max()) <= 32760.0
    for stage in R.STAGES:
        _hold(d, stage)
    for name in d["result"]["fails"]:
        _exact(d, name)
