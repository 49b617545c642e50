"""The streaming lane chain (csrc/af_lane_chain.hip) on the GPU: 70 streams (one full wave and a wave of six lanes) under 70
distinct settings (tests/lane_chain_stimulus.py), 7 300 samples in calls of 1, 63, 8, 900, 960, 1921, 1000 and the rest.

"Bit for bit" is np.array_equal on the raw bits of the audio and of every row field.  The reference of a stream is a plain
one-stream Engine on AUTO, configured by configure_auto_eq_chain with the stream's settings (and its EQ switched off where
the stream's is) and driven with the same calls; the 70 engine runs are made once and shared.  Against the CPU oracle
(tests/chain_oracle.run_calls) the output is within MAX_ABS = 2e-7, MAX_RMS = 2e-8, the bounds tests/test_gpu_parity.py uses for
these stages (the compressor's log10 / exp10 differ from the host's by an ulp or two), and equal bit for bit where the
compressor is off."""
import numpy as np
import pytest

import chain_oracle
import lane_chain_stimulus as LS

pytestmark = pytest.mark.gpu

MAX_ABS = 2e-7
MAX_RMS = 2e-8
ROW_FIELDS = ("input_sample_peak", "output_sample_peak", "true_peak_limiter_input_peak", "output_true_peak",
              "limiter_peak_gain_reduction_db", "true_peak_limiter_gain_reduction_db", "compressor_gain_reduction_db",
              "deesser_gain_reduction_db", "input_square_sum", "output_square_sum", "true_peak_limited_events", "non_finite_output",
              "compressor_makeup_gain_db", "auto_makeup_activity", "auto_makeup_reliability", "reserved")
RECONFIGURED = (3, 64, 69)
RECONFIGURE_AT = 2_500


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_rows_equal(got, want, where):
    assert got.shape == want.shape, where
    for field in ROW_FIELDS:
        assert same_bits(got[field], want[field]), (where, field)


def engine_run(x, fs, bands, st, calls):
    """One stream through a one-stream Engine on AUTO in the given calls: (output [n], rows [blocks])."""
    from mic_eq_mi import mic_eq_core as core

    engine = core.Engine(float(fs), 1)
    try:
        core.configure_auto_eq_chain(engine, float(fs), bands, LS.engine_settings(st))
        if not st.get("eq_enabled", True):
            engine.set_eq_enabled(0)
        out, rows, at = [], [], 0
        for length in calls:
            out.append(engine.process(x[None, at : at + length])[0])
            rows.append(engine.block_stats()[:, 0])
            at += length
    finally:
        engine.close()
    return np.concatenate(out), np.concatenate(rows)


def lane_run(chain, audio, calls):
    """All streams of a LaneChain in the given calls: (output [n_streams, n], rows [blocks, n_streams])."""
    out, rows, at = [], [], 0
    for length in calls:
        out.append(chain.process(audio[:, at : at + length]))
        rows.append(chain.block_stats())
        at += length
    return np.concatenate(out, axis=1), np.concatenate(rows, axis=0)


class Reference:
    """The stimulus, the 70 engine runs and the lane chain's first run; computed once, never changed."""

    def __init__(self):
        import mic_eq_mi

        self.mi = mic_eq_mi
        self.audio = LS.audio()
        self.bands = [LS.bands(i) for i in range(LS.N_STREAMS)]
        self.settings = [LS.settings(i) for i in range(LS.N_STREAMS)]
        runs = [engine_run(self.audio[i], LS.FS, self.bands[i], self.settings[i], LS.CALLS) for i in range(LS.N_STREAMS)]
        self.engine_out = np.stack([r[0] for r in runs])
        self.engine_rows = np.stack([r[1] for r in runs], axis=1)
        chain = self.chain()
        try:
            self.out, self.rows = lane_run(chain, self.audio, LS.CALLS)
            self.processed = [chain.samples_processed(i) for i in (0, 69)]
        finally:
            chain.close()
        for a in (self.audio, self.engine_out, self.out):
            a.setflags(write=False)

    def chain(self, streams=None):
        streams = list(range(LS.N_STREAMS)) if streams is None else list(streams)
        chain = self.mi.LaneChain(float(LS.FS), len(streams))
        chain.configure(range(len(streams)), [self.bands[i] for i in streams], [self.settings[i] for i in streams])
        return chain


@pytest.fixture(scope="module")
def ref():
    return Reference()


def test_every_stream_equals_an_engine_of_its_own(ref):
    assert ref.rows.shape == ref.engine_rows.shape == (13, LS.N_STREAMS) and ref.processed == [LS.N, LS.N]
    for i in range(LS.N_STREAMS):
        assert same_bits(ref.out[i], ref.engine_out[i]), i
        assert_rows_equal(ref.rows[:, i], ref.engine_rows[:, i], i)
    # the stimulus reaches what it is meant to reach: every stage engages on some streams and on none of others
    rows = ref.rows
    comp = rows["compressor_gain_reduction_db"].max(axis=0)
    lim = rows["limiter_peak_gain_reduction_db"].max(axis=0)
    events = rows["true_peak_limited_events"].sum(axis=0)
    on = np.array([LS.compressor_on(i) for i in range(LS.N_STREAMS)])
    lim_on = np.array([LS.limiter_on(i) for i in range(LS.N_STREAMS)])
    assert (comp[on] > 3.0).any() and (comp[on] == 0.0).any() and (comp[~on] == 0.0).all()
    assert (lim[lim_on] > 0.5).any() and (lim[lim_on] == 0.0).any() and (lim[~lim_on] == 0.0).all()
    assert events[lim_on].max() > 0 and (events[lim_on] == 0).any() and (events[~lim_on] == 0).all()
    assert rows["compressor_makeup_gain_db"].max() == np.float32(4.0) and not rows["non_finite_output"].any()
    assert np.isfinite(ref.out).all()


def test_every_stream_agrees_with_the_cpu_oracle(ref):
    worst_abs, worst_rms = 0.0, 0.0
    for i in range(LS.N_STREAMS):
        st = ref.settings[i]
        want, _ = chain_oracle.run_calls(ref.audio[i], LS.FS, ref.bands[i], LS.engine_settings(st), LS.CALLS, eq_enabled=st["eq_enabled"])
        if not st["compressor_enabled"]:
            assert same_bits(ref.out[i], want), i
            continue
        d = ref.out[i].astype(np.float64) - want.astype(np.float64)
        worst_abs = max(worst_abs, float(np.max(np.abs(d))))
        worst_rms = max(worst_rms, float(np.sqrt(np.mean(d * d))))
    print(f"largest |lane chain - oracle| over the streams with a compressor: {worst_abs:.3e} (allowed {MAX_ABS:.0e}), RMS {worst_rms:.3e} "
          f"(allowed {MAX_RMS:.0e})")
    assert worst_abs <= MAX_ABS and worst_rms <= MAX_RMS


def test_a_streams_bits_do_not_depend_on_its_neighbours(ref):
    order = list(range(LS.N_STREAMS))[::-1]
    chain = ref.chain(order)
    try:
        out, rows = lane_run(chain, ref.audio[::-1], LS.CALLS)
    finally:
        chain.close()
    assert same_bits(out[::-1], ref.out)
    assert_rows_equal(rows[:, ::-1], ref.rows, "reversed")
    for lo, hi in ((0, 35), (35, 70)):
        chain = ref.chain(range(lo, hi))
        try:
            out, rows = lane_run(chain, ref.audio[lo:hi], LS.CALLS)
        finally:
            chain.close()
        assert same_bits(out, ref.out[lo:hi])
        assert_rows_equal(rows, ref.rows[:, lo:hi], (lo, hi))


def test_calls_that_end_at_block_boundaries_equal_one_call(ref):
    total = 6 * 960
    chain = ref.chain()
    try:
        want_out, want_rows = lane_run(chain, ref.audio, (total,))
        chain.reset()
        out, rows = lane_run(chain, ref.audio, (960, 1920, 2880))
    finally:
        chain.close()
    assert same_bits(out, want_out)
    assert_rows_equal(rows, want_rows, "calls of 960 k")


def test_reconfiguring_a_slot_leaves_its_neighbours_alone(ref):
    """The 1921-sample call of the first run is made as 568 + 1353, so that 2 500 samples have passed between them.  A call
    boundary moves no audio bit (auto-makeup is off: the block-end smoothing holds the makeup gain where it is); it does split
    that call's rows, so rows are compared for the calls that are the same in both runs."""
    assert sum(LS.CALLS[:5]) + 568 == RECONFIGURE_AT
    calls = LS.CALLS[:5] + (568, 1353) + LS.CALLS[6:]
    others = [i for i in range(LS.N_STREAMS) if i not in RECONFIGURED]
    new_bands = {s: LS.bands(s, seed=11) for s in RECONFIGURED}
    new_settings = {s: LS.settings(LS.N_STREAMS - 1 - s, seed=11) for s in RECONFIGURED}
    assert all(new_settings[s] != ref.settings[s] for s in RECONFIGURED)
    chain = ref.chain()
    try:
        head_out, head_rows = lane_run(chain, ref.audio, calls[:6])
        assert [chain.samples_processed(s) for s in (0, 3)] == [RECONFIGURE_AT, RECONFIGURE_AT]
        chain.configure(RECONFIGURED, [new_bands[s] for s in RECONFIGURED], [new_settings[s] for s in RECONFIGURED])
        assert [chain.samples_processed(s) for s in (0, 3, 64, 69)] == [RECONFIGURE_AT, 0, 0, 0]
        tail_out, tail_rows = lane_run(chain, ref.audio[:, RECONFIGURE_AT:], calls[6:])
        assert [chain.samples_processed(s) for s in (0, 3, 64, 69)] == [LS.N] + [LS.N - RECONFIGURE_AT] * 3
        out = np.concatenate([head_out, tail_out], axis=1)
        assert same_bits(out[others], ref.out[others])
        assert same_bits(head_out[list(RECONFIGURED)], ref.out[list(RECONFIGURED), :RECONFIGURE_AT])
        assert_rows_equal(head_rows[:5, others], ref.rows[:5, others], "calls before the split call")
        assert_rows_equal(tail_rows[2:, others], ref.rows[8:, others], "calls after the split call")
        for s in RECONFIGURED:  # from the configure on: a fresh processor fed the remaining audio
            want_out, want_rows = engine_run(ref.audio[s, RECONFIGURE_AT:], LS.FS, new_bands[s], new_settings[s], calls[6:])
            assert same_bits(tail_out[s], want_out), s
            assert_rows_equal(tail_rows[:, s], want_rows, s)
        # reset: every stream a fresh processor under its current settings
        chain.reset()
        assert [chain.samples_processed(s) for s in (0, 3)] == [0, 0]
        out, rows = lane_run(chain, ref.audio, LS.CALLS)
        assert same_bits(out[others], ref.out[others])
        assert_rows_equal(rows[:, others], ref.rows[:, others], "after reset")
        for s in RECONFIGURED:
            want_out, want_rows = engine_run(ref.audio[s], LS.FS, new_bands[s], new_settings[s], LS.CALLS)
            assert same_bits(out[s], want_out), s
            assert_rows_equal(rows[:, s], want_rows, s)
    finally:
        chain.close()


@pytest.mark.parametrize("fs, lookahead_ms", [(44_100, 2.0), (48_000, 1.0)])
def test_other_geometry(fs, lookahead_ms):
    """44.1 kHz: control block 882, crossfade 66, lookahead 88.  48 kHz with a 1 ms lookahead: a ring of 49 rows."""
    import mic_eq_mi

    n_streams, calls = 5, (500,) * 6
    picks = (0, 3, 16, 22, 64)  # all stages on; limiter off; compressor off; EQ off; another full stream
    audio = LS.audio(n_streams, 3_000, fs, seed=5)
    bands = [LS.bands(i) for i in picks]
    settings = [LS.settings(i, lookahead_ms=lookahead_ms) for i in picks]
    chain = mic_eq_mi.LaneChain(float(fs), n_streams, limiter_lookahead_ms=lookahead_ms)
    try:
        chain.configure(range(n_streams), bands, settings)
        out, rows = lane_run(chain, audio, calls)
    finally:
        chain.close()
    assert rows.shape == (6, n_streams)
    for i in range(n_streams):
        want_out, want_rows = engine_run(audio[i], fs, bands[i], settings[i], calls)
        assert same_bits(out[i], want_out), i
        assert_rows_equal(rows[:, i], want_rows, i)


def test_hostile_input_and_bounds(ref):
    import torch

    n, pad, guard, sentinel = 2_000, 40, 2, 12345.0
    audio = np.array(ref.audio[:, :n])
    hostile = (5, 66)  # one in each wave
    for s in hostile:
        audio[s, 100::97] = np.nan
        audio[s, 150::89] = np.inf
        audio[s, 170::83] = -np.inf
        audio[s, 200::61] = 4.0
        audio[s, 230::67] = -4.0
    d_in = torch.full((LS.N_STREAMS + guard, n + pad), sentinel, dtype=torch.float32, device="cuda")
    d_out = torch.full((LS.N_STREAMS + guard, n + pad), sentinel, dtype=torch.float32, device="cuda")
    d_in[: LS.N_STREAMS, :n] = torch.from_numpy(audio).cuda()
    before = d_in.clone()
    torch.cuda.synchronize()
    chain = ref.chain()
    try:
        chain.process_device(d_in.data_ptr(), d_out.data_ptr(), n, n + pad)
        rows = chain.block_stats()  # (waits for the call)
    finally:
        chain.close()
    got = d_out.cpu().numpy()
    assert torch.equal(d_in.view(torch.int32), before.view(torch.int32))  # (bits: the input holds NaNs)
    assert (got[LS.N_STREAMS :] == sentinel).all() and (got[:, n:] == sentinel).all()  # every sentinel is intact
    out = got[: LS.N_STREAMS, :n]
    assert np.isfinite(out).all() and not rows["non_finite_output"].any()
    for s in hostile:
        want_out, want_rows = engine_run(audio[s], LS.FS, ref.bands[s], ref.settings[s], (n,))
        assert same_bits(out[s], want_out), s
        assert_rows_equal(rows[:, s], want_rows, s)
    clean = [s for s in range(LS.N_STREAMS) if s not in hostile]
    want_out, _ = lane_run_single(ref, audio, n)
    assert same_bits(out[clean], want_out[clean])


def test_process_device_in_place(ref):
    """`out` may equal `in`: every tile is loaded before its region is stored, and a wave owns its rows."""
    import torch

    n, pad = 2_000, 24
    audio = np.array(ref.audio[:, :n])
    want_out, want_rows = lane_run_single(ref, audio, n)
    buffer = torch.zeros((LS.N_STREAMS, n + pad), dtype=torch.float32, device="cuda")
    buffer[:, :n] = torch.from_numpy(audio).cuda()
    torch.cuda.synchronize()
    chain = ref.chain()
    try:
        chain.process_device(buffer.data_ptr(), buffer.data_ptr(), n, n + pad)
        rows = chain.block_stats()  # (waits for the call)
    finally:
        chain.close()
    got = buffer.cpu().numpy()
    assert same_bits(got[:, :n], want_out) and (got[:, n:] == 0.0).all()
    assert_rows_equal(rows, want_rows, "in place")


def lane_run_single(ref, audio, n):
    chain = ref.chain()
    try:
        return lane_run(chain, audio, (n,))
    finally:
        chain.close()


def test_operator_route_lanes_equals_route_groups(ref):
    n_streams, n = 5, 4_000
    audio = np.array(ref.audio[[0, 7, 21, 40, 69], :n])
    presets = [(ref.bands[i], LS.engine_settings(ref.settings[i])) for i in (0, 7, 21)]
    which = (0, 1, 2, 1, 0)  # 3 distinct presets over 5 streams
    bands = [presets[k][0] for k in which]
    settings = [presets[k][1] for k in which]
    want_out, want = ref.mi.simulate_auto_eq_chain_batch(audio, LS.FS, bands, settings)
    out, got = ref.mi.simulate_auto_eq_chain_batch(audio, LS.FS, bands, settings, route="lanes")
    assert same_bits(out, want_out) and len(got) == len(want) == n_streams
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for key in w:
            if key != "candidate_runtime_ms":
                assert g[key] == w[key], key
