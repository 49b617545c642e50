"""The mixed-lane stimulus (`signals.lane_mix_batch`) does what the GPU chain-form tests rely on: waves of 64 streams whose
limiters engage on some lanes and not on others in the same control block.  CPU only: the oracle's block processor over
the stimulus, block rows read per 64-stream group."""
import numpy as np
import pytest

import chain_oracle as CO
import signals as S

N_STREAMS, CALLS = 130, (19_213, 24_000, 20_411)  # 2 groups + 2 lanes; the call pattern of tests/test_gpu_chain_forms.py
SEED = 7


@pytest.fixture(scope="module")
def rows():
    audio = S.lane_mix_batch(N_STREAMS, sum(CALLS), SEED)
    settings = dict(S.limiter_settings(2.0), compressor_enabled=False)
    _, r = CO.run_batch(audio, 48_000, S.LIMITER_BANDS, settings, CALLS)
    return r


def _groups():
    return [(g0 // S.LANE_MIX_GROUP, slice(g0, min(g0 + S.LANE_MIX_GROUP, N_STREAMS))) for g0 in range(0, N_STREAMS, S.LANE_MIX_GROUP)]


def test_stimulus_is_deterministic_and_seeded():
    a = S.lane_mix_batch(N_STREAMS, 20_000, SEED)
    b = S.lane_mix_batch(N_STREAMS, 20_000, SEED)
    assert a.dtype == np.float32 and a.shape == (N_STREAMS, 20_000)
    assert a.tobytes() == b.tobytes()
    assert a.tobytes() != S.lane_mix_batch(N_STREAMS, 20_000, SEED + 1).tobytes()
    # a batch's first streams do not depend on how many follow
    assert a[:70].tobytes() == S.lane_mix_batch(70, 20_000, SEED).tobytes()


def test_stimulus_holds_the_edge_cases():
    x = S.lane_mix_batch(N_STREAMS, sum(CALLS), SEED)
    mixed = x[: S.LANE_MIX_GROUP]
    finite = np.where(np.isfinite(mixed), mixed, 0.0)
    assert np.isnan(mixed).any() and np.isposinf(mixed).any() and np.isneginf(mixed).any()
    assert 0 < int((~np.isfinite(x).all(axis=1)).sum()) <= 4  # non-finite samples in a few streams only
    assert (np.abs(finite) == 4.0).any()
    assert (np.abs(finite).max(axis=1) == 0.0).sum() >= 2  # silent streams
    assert (np.abs(finite).max(axis=1) == 1.0).sum() >= 4  # full-scale squares / clipped two-tones
    # groups are permuted differently: the same lane holds different material in the two full groups
    assert not np.array_equal(finite.std(axis=1), x[64:128].std(axis=1))


def test_oracle_replay_is_reentrant_and_matches_simulate(oracle):
    x = S.lane_mix_batch(8, 30_000, SEED)
    settings = dict(S.limiter_settings(2.0), compressor_enabled=False)
    serial, serial_rows = CO.run_batch(x, 48_000, S.LIMITER_BANDS, settings, (30_000,), workers=1)
    threaded, threaded_rows = CO.run_batch(x, 48_000, S.LIMITER_BANDS, settings, (30_000,), workers=8)
    assert serial.tobytes() == threaded.tobytes() and serial_rows.tobytes() == threaded_rows.tobytes()
    for s in range(8):
        want = oracle.simulate_auto_eq_chain(x[s], 48_000, S.LIMITER_BANDS, settings)["output_audio"]
        assert np.array_equal(serial[s].view(np.uint32), want.view(np.uint32)), s


def test_every_group_splits_its_waves(rows):
    engaged = rows["limiter_peak_gain_reduction_db"] > 0.0  # [block, stream]
    for group, lanes in _groups():
        e = engaged[:, lanes]
        some, every = e.any(axis=1), e.all(axis=1)
        kind = S.lane_mix_kind(group)
        if kind == "under":
            assert not e.any(), f"group {group}: a stream of the all-under group reached the ceiling"
            assert (rows["true_peak_limited_events"][:, lanes] == 0).all()
            continue
        assert (some & ~every).any(), f"group {group}: no block where the limiter engages on some lanes but not all"
        if kind == "over":
            assert e.any(axis=0).all(), f"group {group}: a stream of the all-over group never reached the ceiling"
            assert every.any(), f"group {group}: no block where every lane is over the ceiling"
            assert (~some).any(), f"group {group}: no block where every lane is under the ceiling"
        else:
            assert (some & ~every).mean() > 0.9, f"group {group}: the waves are not split most of the time"


def test_true_peak_limiter_engages_on_some_streams_only(rows):
    events = rows["true_peak_limited_events"].sum(axis=0)
    assert (events > 0).any() and (events == 0).any()
    assert ((events > 0)[: S.LANE_MIX_GROUP]).any() and ((events == 0)[: S.LANE_MIX_GROUP]).any()
