"""The oracle (af_oracle_py.RnnoiseTap, the f32 restatement) against the FREE-RUNNING float64 reference
(suppressor_stage_ref.free_run) on the lane stimulus of tests/test_gpu_gate_lanes.py.  No GPU.

tests/test_suppressor_stage_ref.py holds the oracle stage by stage, every stage fed the tap of the one before it: that
measures each stage's rounding and nothing of what the recursion (cepstral ring, three GRUs, `lastg`, overlap) makes of it.
Here nothing is teacher-forced but the pitch index, so the distance is what an f32 evaluation of the WHOLE algorithm is off
an exact one.  On most cells that is 1e-7 or less; on a few frames of a few streams it is several 1e-5 -- the streams
test_gpu_gate_lanes.py lists as SUPPRESSOR_EXCEPTIONS, at the frames test_gate_lane_stimulus.py names.  The f32 algorithm is
ill-conditioned there: the oracle is not the truth to 1e-5 on those frames, and a second correct f32 evaluation (the
device) may leave it by several 1e-5.  What the device may do there is bounded from these figures
(tests/test_gpu_suppressor_free_run.py, and the caps of test_gpu_gate_lanes.py).

Measured, 10 streams x 200 frames, wrapper protocol at strength 1.0 (oracle vs free run, worst cell | frames over 1e-5):
  stream   A: suppressor behind the prefilter        B: behind the gate (mode 1, defaults)
  29       2.66e-5 | 140 141 180 181                  3.97e-5 | 140 141 180 181
  68       1.72e-5 | 3 4                              1.93e-5 | 3 4
  82       2.08e-5 | 53 54                            1.29e-5 | 53 54
  93       2.63e-5 | 147 148 164 165                  2.43e-5 | 147 148 164 165 175
  4, 17    1.8e-6 (soft clip in ~135 frames)          1.9e-6
  0 10 63 64   at most 6.5e-8                         at most 6.4e-8
Ill-conditioned cells (over 2e-6, or within +-2 frames of such a cell): A 120 of 2000, B 121 of 2000; the worst calm cell
1.95e-6 / 1.89e-6; the median of every stream at or under 6.3e-8.  Silence flags equal on all cells (B: 36 silent ones).
At the frames over 1e-5 the oracle's features are up to 9.4e-4 off the free run's (3.8e-5 teacher-forced), and over 1e-4 only
in the pitch-correlation indices 34..39; `test_where_the_digits_go` prints them per stream and says where the digits go.
"""
import numpy as np
import pytest

import lane_free_run_stimulus as L
import suppressor_stage_ref as R
import suppressor_stage_stimulus as T

BUDGET = 1e-5  # the project's budget for the suppressor's output against the oracle
FEATURE_LOSS = 1e-4  # a feature this far from the free run carries the loss (teacher-forced the worst feature is 3.8e-5)


@pytest.fixture(scope="module", params=L.CONFIGS)
def lane(request, oracle):
    return request.param, L.run(request.param)


def _table(config, d):
    dist = d["distance"]
    print(f"configuration {config}: stream | oracle vs f64 free run, worst | median | frames over {BUDGET:g} | ill-conditioned cells")
    for i, s in enumerate(L.STREAMS):
        over = np.flatnonzero(dist[:, i] > BUDGET).tolist()
        print(f"  {s:3d} | {dist[:, i].max():.3e} | {np.median(dist[:, i]):.2e} | {over} | {int(d['ill'][:, i].sum())}")


def test_silence_flags_equal_everywhere(lane):
    config, d = lane
    assert np.array_equal(d["free"]["silence"], d["taps"]["silence"] != 0)
    margin = np.abs(d["free"]["Ex_sum"] - R.SILENCE_THRESHOLD) / R.SILENCE_THRESHOLD
    print(f"configuration {config}: {int(d['free']['silence'].sum())} silent cells; the band-energy sum nearest the threshold is "
          f"{margin.min():.2e} of it away")
    assert d["result"]["fails"]["near_threshold"] == [] and d["result"]["fails"]["silence_wrong"] == []


def test_ill_conditioned_cells_are_few_and_on_the_named_streams(lane):
    """At most 10 % of a configuration's cells are ill-conditioned; the streams with a cell over 1e-5 are exactly the named
    ones; the calm cells are within 2e-6 by their definition, which leaves the figure to print."""
    config, d = lane
    _table(config, d)
    dist, ill = d["distance"], d["ill"]
    print(f"configuration {config}: {int(ill.sum())} of {ill.size} cells ill-conditioned ({100.0 * ill.mean():.1f} %), "
          f"worst calm cell {dist[~ill].max():.3e}")
    assert ill.mean() <= 0.10
    assert float(dist[~ill].max()) <= L.CALM_LIMIT
    over = tuple(sorted(s for i, s in enumerate(L.STREAMS) if dist[:, i].max() > BUDGET))
    assert over == L.NAMED, over


def test_teacher_forced_the_oracle_is_ordinary_on_these_cells(lane):
    """Stage by stage (`evaluate`) the oracle is as close to f64 on the lane stimulus as on the stage stimulus: the loss is
    the recursion's, not a stage's.  The caps are those of test_suppressor_stage_ref.py."""
    from test_suppressor_stage_ref import CAPS

    config, d = lane
    for stage in R.STAGES:
        value, f, s = R.worst(d["result"]["err"][stage])
        print(f"configuration {config}: {stage:9s} oracle vs f64, teacher-forced {value:.3e} (frame {f}, stream {L.STREAMS[s]})")
        assert value <= CAPS[stage], (stage, value, f, L.STREAMS[s])
    for name, cells in d["result"]["fails"].items():
        assert cells == [], (name, cells[:8])


def test_where_the_digits_go(lane):
    """Per named stream, at the frames over 1e-5 and the two before each: the oracle's features, Ep and gains_raw against the
    free run's, which feature indices are over 1e-4, and pitch_filter's amplification sqrt(Ex / Ep).

    What it shows: each excess starts on a frame in which a loud, nearly pure tone changes level abruptly (29, 82, 93: a
    step of the level flutter from 0.8 to 0.06 of full scale inside one frame) or in which a +-4.0 sample sits on a tone
    (68).  X of that frame is broadband, but P, the pitch-lagged window, still holds the tone alone: in the upper bands Ep
    is ten decades under the frame's peak, so P is there nothing but the rounding floor of an f32 transform (Ep is 2e-4 ..
    7e-3 relative off the f64 value, against 2e-7 in an ordinary band).  pitch_filter adds r P with r ~ sqrt(Ex / Ep),
    3 000 .. 22 000 there, which lifts that floor towards the level of X: the frame and, through the overlap, the next one
    are off by a few 1e-5 of full scale.  The features see the same P through Exp: only the pitch-correlation features
    34..39 (the DCT of Exp) are over 1e-4.  The network is not the amplifier: gains_raw moves by 1.3e-5 at the most, and
    the free run's gains put into the synthesis of the oracle's own frame move it by 2e-7 .. 4.5e-6 of full scale; the free
    run's Ex, Ep and Exp put there move it by 6e-6 .. 2.0e-5."""
    config, d = lane
    taps, free = d["taps"], d["free"]
    diff = np.abs(taps["feat"][:, :, :R.NFEAT].astype(np.float64) - free["feat"])
    graw = np.abs(taps["gains_raw"].astype(np.float64) - free["gains_raw"]).max(axis=2)
    ep = np.abs(taps["Ep"].astype(np.float64) - free["Ep"]) / free["Ep"]
    lift = np.sqrt(free["Ex"] / (1e-8 + free["Ep"]))
    ordinary = R.worst(d["result"]["err"]["Ep"])[0]
    for i, s in enumerate(L.STREAMS[:len(L.NAMED)]):
        frames = sorted({g for f in np.flatnonzero(d["distance"][:, i] > BUDGET) for g in range(max(f - 2, 0), f + 1)})
        worst = diff[frames, i].max(axis=0)
        carried = np.flatnonzero(worst >= FEATURE_LOSS).tolist()
        print(f"configuration {config}, stream {s}, frames {frames}: features off by up to {worst.max():.2e}, indices at or over "
              f"{FEATURE_LOSS:g}: {carried}; Ep off by up to {ep[frames, i].max():.1e} relative (teacher-forced {ordinary:.1e}), "
              f"sqrt(Ex / Ep) up to {lift[frames, i].max():.0f}; gains_raw off by up to {graw[frames, i].max():.1e}")
        assert set(carried) <= set(range(34, 40)), (s, carried)
        assert ep[frames, i].max() > 100 * ordinary, (s, ep[frames, i].max())
        assert graw[frames, i].max() < 1e-4, (s, graw[frames, i].max())


@pytest.mark.parametrize("kind", ["synthetic", "wrapper"])
def test_free_run_agrees_with_the_oracle_on_the_stage_stimulus(oracle, kind):
    """Where nothing is ill-conditioned the free run and the oracle agree on every cell: silence flags equal, no cell over
    the calm limit (silent spans, a stream near the threshold, clamped and quiet streams; the wrapper run with the mix at
    strength 0.6)."""
    run = T.restatement(kind)
    wrapper = kind == "wrapper"
    free = R.free_run(run["model_input"], run["taps"]["pitch_index"], run["blob"], strength=run["strength"],
                      dry=run["audio"] if wrapper else None)
    silent = run["taps"]["silence"] != 0
    assert np.array_equal(free["silence"], silent) and silent.any() and (~silent).any()
    dist = L.cell_max(run["taps"]["out"].astype(np.float64) - free["out"])
    feat = np.abs(run["taps"]["feat"][:, :, :R.NFEAT].astype(np.float64) - free["feat"]).max()
    graw = np.abs(run["taps"]["gains_raw"].astype(np.float64) - free["gains_raw"]).max()
    print(f"{kind}: oracle vs free run over {dist.size} cells: output {dist.max():.3e}, features {feat:.2e}, gains_raw {graw:.2e}")
    assert not L.ill_conditioned(dist).any() and float(dist.max()) <= L.CALM_LIMIT
    assert np.all(free["gains_raw"][silent] == 0.0) and np.all(free["feat"][silent] == 0.0)


def test_expected_model_input_rows(oracle):
    """What the GPU test compares the pre-pass's buffer with: the stimulus reaches +-4.0 and non-finite samples in front of
    the soft clip, and the rows stay inside the model's range."""
    x = L.audio()
    assert x.shape == (L.N_STREAMS, L.N) and not np.isfinite(x).all() and float(np.abs(np.nan_to_num(x, posinf=0, neginf=0)).max()) == 4.0
    for config in L.CONFIGS:
        rows = L.expected_rows(config)
        assert rows.shape == (len(L.STREAMS), R.PBUF + L.N) and rows.dtype == np.float32 and np.isfinite(rows).all()
        assert not rows[:, :R.PBUF].any() and float(np.abs(L.run(config)["model_input"]).max()) <= 32768.0
    clipped = [s for i, s in enumerate(L.STREAMS) if float(np.abs(L.run("A")["signal"][i]).max()) > 1.0]
    print(f"streams of the selection over +-1.0 behind the prefilter: {clipped}")
    assert {4, 17} <= set(clipped)
