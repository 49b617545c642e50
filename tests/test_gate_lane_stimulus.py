"""The lane-role stimulus (`signals.gate_lane_batch`) does what tests/test_gpu_gate_lanes.py relies on: in every 64-stream
group and in every eight-row octet the gated pre-pass's F1 waves map (wave 2-5 x half-wave), the gate is open on some rows
and closed on others in the same 32-sample tile, changes state at tile offsets 0, 31 and in between, chatters, and (mode 1)
reaches the 24 dB auto-relax floor.  CPU only: the oracle's gate over the front end's output, in 32-sample chunks."""
import ctypes as C

import numpy as np
import pytest

import af_oracle_py as O
import chain_oracle as CO
import signals as S

N_STREAMS, N = 130, 96_000  # 2 groups + 2 rows; the length of tests/test_gpu_gate_lanes.py
CALLS = (1, 31, 33, 4799, 19_213, N - 24_077)  # its calls: the kernel's tiles restart at each call's first sample
SEED = 2
T, G, OCTET = S.GATE_LANE_TILE, S.GATE_LANE_GROUP, 8
FLOOR_24 = 10.0 ** (-24.0 / 20.0)


def _tiles(x: np.ndarray, vad_mode: bool):
    """Per tile (32 samples from each call's start, as the kernel tiles them) end: is_open, auto-relax armed, gain at the floor, chatter events; and the tile offsets of every change of
    is_open (a tile whose end state differs from its start is replayed sample by sample from a copy of the state)."""
    g = O.Gate(vad_mode=vad_mode)
    probe = O.Gate(vad_mode=vad_mode)
    starts = [t0 + k for t0, c in zip(np.cumsum((0,) + CALLS[:-1]), CALLS) for k in range(0, c, T)]
    ntiles = len(starts)
    is_open = np.zeros(ntiles, bool)
    floor = np.zeros(ntiles, bool)
    offsets = []
    for ti, (t0, t1) in enumerate(zip(starts, starts[1:] + [x.size])):
        tile = x[t0:t1]
        before = g.is_open
        C.memmove(C.byref(probe.s), C.byref(g.s), C.sizeof(g.s))
        g.process(tile)
        if g.is_open != before:
            for t in range(tile.size):
                was = probe.is_open
                probe.process(tile[t : t + 1])
                if probe.is_open != was:
                    offsets.append(t)
        is_open[ti] = g.is_open
        # the 24 dB floor is the target: closed, the relax armed, the detector more than 32 dB under the threshold
        floor[ti] = (not g.is_open and g.s.auto_relax_remaining_samples > 0
                     and g.s.detector_level_db < g.s.threshold_db - 32.0 and g.current_gain > FLOOR_24)
    return is_open, floor, np.asarray(offsets, dtype=np.int64), g.chatter_event_count


@pytest.fixture(scope="module")
def audio():
    return S.gate_lane_batch(N_STREAMS, N, SEED)


@pytest.fixture(scope="module")
def front(audio):
    return np.stack([O.prefilter(CO.sanitize(audio[s], False)) for s in range(N_STREAMS)])


@pytest.fixture(scope="module", params=[0, 1], ids=["mode0", "mode1"])
def tiles(request, front):
    rows = [_tiles(front[s], request.param == 1) for s in range(N_STREAMS)]
    return request.param, rows


def test_stimulus_is_deterministic_and_seeded(audio):
    assert audio.dtype == np.float32 and audio.shape == (N_STREAMS, N)
    assert audio.tobytes() == S.gate_lane_batch(N_STREAMS, N, SEED).tobytes()
    assert audio.tobytes() != S.gate_lane_batch(N_STREAMS, N, SEED + 1).tobytes()
    # a batch's first streams do not depend on how many follow
    assert audio[:70].tobytes() == S.gate_lane_batch(70, N, SEED).tobytes()
    assert audio[:64].tobytes() == S.gate_lane_batch(64, N, SEED).tobytes()


def test_stimulus_holds_the_edge_cases(audio):
    finite = np.where(np.isfinite(audio), audio, 0.0)
    for g0 in range(0, N_STREAMS, G):
        grp, fin = audio[g0 : g0 + G], finite[g0 : g0 + G]
        if grp.shape[0] < G:
            continue
        assert np.isnan(grp).any() and np.isposinf(grp).any() and np.isneginf(grp).any(), g0
        assert (np.abs(fin) == 4.0).any() and (np.abs(fin) == 1.5).any(), g0
        assert (np.abs(fin).max(axis=1) == 0.0).sum() == 1, g0  # one silent row
        assert (np.abs(fin.mean(axis=1)) > 0.25).sum() == 2, g0  # two rows with a DC offset
    for g0 in range(0, N_STREAMS, G):  # no two rows of a group are identical (only the silent rows repeat across groups)
        assert len({row.tobytes() for row in audio[g0 : g0 + G]}) == audio[g0 : g0 + G].shape[0], g0
    # the same lane holds different material in the two full groups
    assert not np.allclose(finite[:64].std(axis=1), finite[64:128].std(axis=1))


def test_every_octet_splits_its_rows(tiles):
    mode, rows = tiles
    for g0 in range(0, N_STREAMS - G + 1, G):  # (the complete groups; the last group's 2 rows are checked below)
        for o in range(G // OCTET):
            lanes = range(g0 + o * OCTET, g0 + (o + 1) * OCTET)
            where = f"mode {mode}, group {g0 // G}, F1 octet {o} (wave {2 + o // 2}, half {o % 2})"
            opened = np.stack([rows[s][0] for s in lanes])  # [row, tile]
            assert (opened.any(axis=0) & ~opened.all(axis=0)).mean() > 0.2, f"{where}: too few tiles split open / closed"
            offsets = np.concatenate([rows[s][2] for s in lanes])
            assert (offsets == 0).any() and (offsets == T - 1).any(), f"{where}: no change at tile offset 0 or 31"
            assert ((offsets > 0) & (offsets < T - 1)).sum() >= 8, f"{where}: too few changes inside tiles"
            assert any(rows[s][3] > 0 for s in lanes), f"{where}: no row chattered"
            if mode == 1:
                assert any(rows[s][1].any() for s in lanes), f"{where}: no row reached the 24 dB floor with the relax armed"
    tail = range(N_STREAMS - N_STREAMS % G, N_STREAMS)
    assert any(rows[s][0].any() for s in tail) and any((~rows[s][0]).any() for s in tail)


def test_suppressor_exceptions_are_not_pitch_filter_near_ties():
    """The frames where the GPU suppressor leaves 1e-5 of the oracle on this stimulus (tests/test_gpu_gate_lanes.py,
    SUPPRESSOR_EXCEPTIONS; stream: first frames of the excess) are not near-ties of pitch_filter's one discontinuous
    decision (Exp > g): every band is at least 5e-3 from its edge there."""
    import gate_oracle as GO

    calls = (1_000, 20_011, 33_333, N - 54_344)
    m = sum(GO.output_calls(calls, "wrapper"))
    x = S.gate_lane_batch(94, N, SEED)
    params = dict(GO.DEFAULT_GATE, mode=1)
    for s, frames in {29: (31, 140, 180), 68: (3,), 82: (54,), 93: (147, 164)}.items():
        gated, _ = GO.run_stream(x[s], 48_000.0, calls, params)
        margin = O.suppressor_pitch_filter_margins(gated[:m])
        for f in frames:
            assert margin[f - 2 : f + 1].min() >= 5e-3, (s, f, margin[f - 2 : f + 1])
