"""What the stimulus of tests/pitch_search_forms_stimulus.py reaches, shown on the float64 search of tests/pitch_stage_ref.py
and its intermediate decisions (the coarse pair, the fine pair, the interpolation offset) -- so that a build of the search
kernel held to a recording on that stimulus (tests/test_gpu_pitch_search_forms.py) has been held to every one of these
classes.  No GPU.

The coarse correlation's lag is 16 x row + column in the matrix form of the kernel (csrc/af_pitch_coarse_map.h): rows 0 .. 9,
columns 0 .. 15; row 9 holds the lags 144 .. 146 only.
"""
import functools

import numpy as np

import pitch_search_forms_stimulus as F
import pitch_stage_ref as P


def _coarse_terms(ds: np.ndarray):
    """The coarse stage's correlations and the values of its energy recurrence before the clamp, as pitch_stage_ref forms them."""
    x_lp, y = ds[P.PMAX >> 1:], ds
    n4, mp4 = P.PFRAME >> 2, P.MAX_PITCH >> 2
    x4 = x_lp[0:2 * n4:2]
    y4 = y[0:2 * ((P.PFRAME + P.MAX_PITCH) >> 2):2]
    xc4 = np.array([np.dot(x4, y4[i:i + n4]) for i in range(mp4)])
    syy, before = 1.0 + float(np.dot(y4[:n4], y4[:n4])), []
    for i in range(mp4):
        syy += float(y4[i + n4] * y4[i + n4] - y4[i] * y4[i])
        before.append(syy)
        syy = max(1.0, syy)
    return xc4, np.array(before)


@functools.lru_cache(maxsize=None)
def _cells() -> tuple:
    """(part, frame, stream, index, info, ds) of every cell of the stimulus, searched in f64."""
    out = []
    for name, spans, frames in F.parts():
        for f in range(frames):
            for s in range(spans.shape[0]):
                ds, _ = P.pitch_downsample(spans[s, P.FRAME * (f + 1):P.FRAME * (f + 1) + P.PBUF])
                index, info = P.pitch_search(ds)
                out.append((name, f, s, index, info, ds))
    return tuple(out)


def test_stimulus_is_deterministic_and_small():
    names = [p[0] for p in F.parts()]
    assert names == ["search1", "search3", "search4", "search6", "stimulus", "steer"]
    cells = sum(spans.shape[0] * frames for _, spans, frames in F.parts())
    assert 1500 <= cells <= 4000, cells
    for _, spans, frames in F.parts():
        assert spans.dtype == np.float32 and spans.shape[1] == P.PBUF + P.FRAME * frames and np.all(np.isfinite(spans))
    F.steer_spans.cache_clear()
    again = F.steer_spans()
    assert np.array_equal(again, F.parts()[-1][1]) and again.shape[0] == len(F.steer_cases())
    h = F.buffer_hashes(np.array([[np.zeros(864), np.full(864, -0.0)]], dtype=np.float32))
    assert h.shape == (1, 2) and h.dtype == np.uint64 and h[0, 0] != h[0, 1]


def test_every_row_and_column_of_the_coarse_map_wins_and_comes_second():
    best0 = {c[4]["coarse"][0] for c in _cells()}
    best1 = {c[4]["coarse"][1] for c in _cells()}
    for name, lags in (("best0", best0), ("best1", best1)):
        assert {lag >> 4 for lag in lags} == set(range(10)), (name, sorted({lag >> 4 for lag in lags}))
        assert {lag & 15 for lag in lags} == set(range(16)), (name, sorted({lag & 15 for lag in lags}))
        # row 9 exists as the columns 0 .. 2 only: every one of them
        assert {lag & 15 for lag in lags if lag >> 4 == 9} == {0, 1, 2}, name
        assert set(F.EDGE_LAGS) <= lags, (name, sorted(set(F.EDGE_LAGS) - lags))
    # beyond the rows and columns: every single lag, both ways
    assert best0 == set(range(147)) and best1 == set(range(147)), (sorted(set(range(147)) - best0), sorted(set(range(147)) - best1))


def test_candidate_order_overlap_and_blocks():
    coarse = [c[4]["coarse"] for c in _cells()]
    assert any(b1 < b0 for b0, b1 in coarse) and any(b1 > b0 for b0, b1 in coarse)
    assert any(c[4]["candidates_overlap"] and c[4]["coarse"][0] != c[4]["coarse"][1] for c in _cells())
    assert {abs(b0 - b1) for b0, b1 in coarse} >= {1, 2}
    # the fine candidates of one cell in different 64-lag blocks of the former five-round selection, every pair of blocks
    blocks = {tuple(sorted(((2 * b0) >> 6, (2 * b1) >> 6))) for b0, b1 in coarse}
    assert blocks >= {(a, b) for a in range(5) for b in range(a + 1, 5)}, sorted(blocks)


def test_fine_winner_edges_and_offsets():
    fine0 = {c[4]["fine"][0] for c in _cells()}
    assert 0 in fine0 and (292 in fine0 or 293 in fine0), (min(fine0), max(fine0))
    assert 293 in fine0  # the last lag: i + 1 >= mp, no interpolation
    assert {c[4]["offset"] for c in _cells()} == {-1, 0, 1}
    assert any(c[4]["best0_at_edge"] for c in _cells()) and any(not c[4]["best0_at_edge"] for c in _cells())
    # a fine winner that is not the centre of its coarse candidate: the +-1 and +-2 neighbours are really searched
    assert {c[4]["fine"][0] - 2 * c[4]["coarse"][0] for c in _cells() if abs(c[4]["fine"][0] - 2 * c[4]["coarse"][0]) <= 2} >= {-1, 0, 1}


def test_nothing_passes():
    zero = [c for c in _cells() if not np.any(c[5])]
    assert zero and all(c[3] == 768 and c[4]["coarse"] == (0, 1) and c[4]["fine"] == (0, 1) for c in zero)
    kinds = [k[0] for k in F.steer_cases()]
    neg = [c for c in _cells() if c[0] == "steer" and kinds[c[2]] == "negative"]
    assert len(neg) == 1
    ds = neg[0][5]
    xc4, _ = _coarse_terms(ds)
    assert np.any(ds != 0) and np.all(xc4 <= 0) and np.any(xc4 < 0)
    assert neg[0][3] == 768 and neg[0][4]["coarse"] == (0, 1) and neg[0][4]["fine"] == (0, 1)


def test_quiet_span_meets_the_clamp():
    kinds = [k[0] for k in F.steer_cases()]
    quiet = [c for c in _cells() if c[0] == "steer" and kinds[c[2]] == "quiet"]
    assert len(quiet) == len(F.QUIET_LEVELS)
    clamped = 0
    for c in quiet:
        xc4, before = _coarse_terms(c[5])
        assert float(np.dot(c[5], c[5])) < 1e4  # quiet: the 1 of `1 + energy` is not negligible
        assert c[4]["coarse"][0] == 92, c[4]["coarse"]
        clamped += int(np.any(before < 1.0))
    # 1 + e - e in floating point is 1 or one ulp beside it: at least one of the levels lands under 1 and is clamped
    assert clamped >= 1, clamped


def test_classes_no_signal_can_reach():
    """Named, with the reason: row 9 has no columns 3 .. 15 (the lags 147 .. 159 do not exist; the kernel computes and
    drops them), and the rows 10 .. 15 are idle.  The fine lags beyond 2 x 146 + 2 = 294 do not exist either."""
    lags = {lag for c in _cells() for lag in c[4]["coarse"]}
    assert max(lags) == 146 and max(c[4]["fine"][0] for c in _cells()) <= 293
