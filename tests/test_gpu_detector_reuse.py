"""The token ring's output true-peak detector where it reuses the input observer's maxima, against kernel 1, bit for bit.

While the true-peak gain is exactly 1 and its clamp idle, the detector's ring holds the bits the observer's ring held 20
samples (five chunks) earlier, so chain_ring_kernel takes the chunk's output true peak from the maxima the observer stored
five chunks before instead of running the detector's own 128-tap FIR; after anything else it runs the FIR as before.  Which
path a chunk takes must not show anywhere: every case below holds the audio and EVERY block row of ALL 66 streams (two
workgroups, the second with two live lanes) to the lane-per-stream kernel on the same input, call by call, and reads the
engine's reuse counter (af_engine_debug_detector_reuse_chunks) to know which path ran.  The chain is the benchmark's
(tests/golden/limiter_lookahead.json, 2 ms lookahead), control block 960.

`output_true_peak` is also held to the CPU oracle at the parity tests' tolerance (2e-5 relative on the dB figure; the
oracle's simulator works in control blocks of 480, so that run uses 480 as well).
"""
import numpy as np
import pytest

import signals as S

pytestmark = pytest.mark.gpu

N_STREAMS = 66
SETTINGS = {k: v for k, v in S.limiter_settings(2.0).items() if k not in ("return_output_audio", "deesser_enabled")}


@pytest.fixture(scope="module")
def core():
    import mic_eq_mi
    from mic_eq_mi import _lib, mic_eq_core

    assert mic_eq_mi.CORE_AVAILABLE, "HIP library missing: GPU tests never fall back to the CPU"
    assert _lib.load().af_device_count() >= 1
    return mic_eq_core


def run(core, kernel, audio, calls, control_block=960):
    """(audio, block rows, the reuse counter after every call)."""
    eng = core.Engine(48_000.0, audio.shape[0])
    try:
        core.configure_auto_eq_chain(eng, 48_000.0, S.LIMITER_BANDS, dict(SETTINGS))
        eng.set_control_block_samples(control_block)
        eng.set_kernel(kernel)
        ys, rows, counts = [], [], []
        for lo, hi in calls:
            ys.append(eng.process(audio[:, lo:hi]))
            rows.append(eng.block_stats().copy())
            counts.append(eng.debug_detector_reuse_chunks())
            assert eng._lib.af_engine_last_kernel(eng._h) == kernel
        return np.concatenate(ys, axis=1), np.concatenate(rows, axis=0), counts
    finally:
        eng.close()


def both(core, audio, calls):
    """Kernel 2 held to kernel 1 on every sample, every row field and every stream; kernel 2's (audio, rows, counts)."""
    from mic_eq_mi import _lib

    y1, r1, c1 = run(core, _lib.KERNEL_LANE_PER_STREAM, audio, calls)
    y2, r2, c2 = run(core, _lib.KERNEL_PHASED, audio, calls)
    assert c1 == [0] * len(calls), "kernel 1 has no reuse path"
    assert y1.shape == y2.shape == (N_STREAMS, calls[-1][1])
    diff = np.argwhere(y1.view(np.uint32) != y2.view(np.uint32))
    assert diff.size == 0, f"{len(diff)} samples differ, first (stream, sample) {tuple(diff[0])}"
    assert r1.shape == r2.shape and r1.shape[1] == N_STREAMS
    for name in r1.dtype.names:
        a, b = r1[name], r2[name]
        same = (a.view(np.uint32) == b.view(np.uint32)) if a.dtype == np.float32 else (a == b) | ((a != a) & (b != b))
        bad = np.argwhere(~same)
        assert bad.size == 0, (name, "first (block, stream)", tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])
    for name in ("output_true_peak", "true_peak_limiter_input_peak", "true_peak_limited_events"):
        assert name in r1.dtype.names
    return y2, r2, c2


def spans(lengths):
    edges = np.concatenate([[0], np.cumsum(lengths)])
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:])]


def quiet(n):
    return S.batch_signal(N_STREAMS, (n + 479) // 480)[:, :n] * np.float32(0.5)


def test_quiet_input_reuses_and_matches_kernel_1_and_the_oracle(core, oracle):
    from mic_eq_mi import _lib

    calls = spans([960, 2880, 1001])  # the last call ends on a ragged chunk
    audio = quiet(calls[-1][1])
    _, rows, counts = both(core, audio, calls)
    assert counts[0] > 0 and counts[0] < counts[1] < counts[2], counts
    chunks = sum((hi - lo) // 4 for lo, hi in calls)
    assert counts[2] <= 2 * (chunks - 8 * len(calls)), "a launch's first eight chunks cannot reuse"
    assert not rows["true_peak_limited_events"].any()
    # the oracle's simulator: control blocks of 480
    _, rows480, counts480 = run(core, _lib.KERNEL_PHASED, audio, calls, control_block=480)
    assert counts480[-1] > 0
    for s in range(N_STREAMS):
        want = oracle.simulate_auto_eq_chain(audio[s], 48_000, S.LIMITER_BANDS, dict(SETTINGS))["output_true_peak_db"]
        got = float(core._linear_to_db(max(np.float32(0.0), np.float32(rows480["output_true_peak"][:, s].max()))))
        assert abs(got - want) <= 2e-5 * max(1.0, abs(want)), (s, got, want)


def test_bursts_over_the_ceiling_take_the_fir_path_in_the_same_call(core):
    """Streams 5 and 64 (one per workgroup) leave the sample limiter with inter-sample peaks over the true-peak ceiling: a
    12 kHz sine sampled 45 degrees off its crests.  Two seconds of the quiet signal follow."""
    lead, burst, tail = 9600, 960, 96_000
    n = lead + burst + tail
    audio = quiet(n)
    t = np.arange(burst)
    tone = (4.0 * np.sin(2.0 * np.pi * 12_000.0 / 48_000.0 * t + np.pi / 4.0)).astype(np.float32)
    for s in (5, 64):
        audio[s, lead:lead + burst] = tone
    _, rows, counts = both(core, audio, [(0, n)])
    limited = rows["true_peak_limited_events"].sum(axis=0)
    assert limited[5] > 0 and limited[64] > 0, limited[[5, 64]]
    others = np.delete(np.arange(N_STREAMS), [5, 64])
    assert not limited[others].any()
    # both paths in the one call: reuse ran in both workgroups (the lead-in alone allows 2400 - 8 chunks in each; 64 are
    # left for the stale streams that the second group's idle lanes mirror), and in either group at least half of the
    # burst's chunks, where the gain is under 1, ran the FIR
    assert 2 * (lead // 4 - 64) <= counts[0] <= 2 * (n // 4 - 8) - burst // 4, counts


def test_fade_through_denormals_on_the_reuse_path(core):
    n1, n2 = 9600, 1920
    audio = quiet(n1 + n2)
    fade = np.exp(np.linspace(0.0, np.log(1e-44), n1)).astype(np.float64)
    audio[:, :n1] = (audio[:, :n1].astype(np.float64) * fade).astype(np.float32)
    audio[:, n1:] = (audio[:, n1:].astype(np.float64) * 1e-44).astype(np.float32)
    tiny = np.finfo(np.float32).tiny
    assert np.any((np.abs(audio) > 0) & (np.abs(audio) < tiny)), "the input holds denormals"
    y, rows, counts = both(core, audio, spans([n1, n2]))
    print("denormal output samples:", int(np.count_nonzero((np.abs(y) > 0) & (np.abs(y) < tiny))))
    assert counts[0] > 0 and counts[1] - counts[0] >= 2 * (n2 // 4 - 8 - 64), counts
    assert not rows["true_peak_limited_events"].any()


def test_short_calls_never_reuse(core):
    """Sixteen samples are four chunks: the clean run starts at 0 in every launch and needs nine."""
    lengths = [16] * 12 + [960]
    calls = spans(lengths)
    _, _, counts = both(core, quiet(calls[-1][1]), calls)
    assert counts[:12] == [0] * 12, counts
    assert counts[12] > 0, counts
