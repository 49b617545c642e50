"""Per-stream lifecycle on the device: restart, export and import of single streams of a running engine, bit for bit.

Every engine has the switch on and 960-sample control blocks; the big ones have 130 streams (two full 64-stream groups and a
two-stream tail).  Calls are 4800 samples (4800 % 97 = 47, 4800 % 21 = 12: the limiter's ring is never at phase 0 after the
first call).  The stimulus is the loud per-stream voices of tests/live_control_cases.py; every test asserts from the block rows
that the limiter reduces gain in the blocks on both sides of every call boundary, so the ring that is moved is never silent.

"Equal" below is np.array_equal on the audio and on every field of the block rows -- no tolerance.  The one tolerance is the
oracle comparison of a restarted stream, at tests/test_gpu_parity.py's bound for that chain (2e-7 max abs, 2e-8 rms).

The refusal tests want to show that a refused call touched nothing by comparing exports from before and after it.  Taken
literally that cannot be run: while the refusing condition holds an export is refused too, and once it is gone the streams
have moved on.  So the refused calls are made on one of two engines that are otherwise driven alike, and byte-equal exports of
every stream (and equal audio) are demanded from both at the next point where an export is accepted: a refused call that had
touched anything would show there."""
import numpy as np
import pytest

import chain_oracle as CO
import live_control_cases as LC
import stream_lifecycle_cases as SL

pytestmark = pytest.mark.gpu

C_ = SL.CALL
PARITY_TOL = (2e-7, 2e-8)  # tests/test_gpu_parity.py MAX_ABS / MAX_RMS
RESTARTED = [0, 63, 64, 129]
MOVED_FROM, MOVED_TO = [5, 70, 129], [63, 0, 17]
FIELDS = None


def _fields():
    global FIELDS
    if FIELDS is None:
        from mic_eq_mi import mic_eq_core as core

        FIELDS = tuple(n for n in core.STATS_DTYPE.names if n != "reserved")
    return FIELDS


def _audio():
    return SL.audio(SL.N_STREAMS, 7 * C_)  # calls 1-6, and one more for the engines that start a call earlier


def _run(eng, x, calls=None):
    """`x` through `eng` in calls of 4800 samples: (audio [streams, n], rows [blocks, streams])."""
    outs, rows = [], []
    at = 0
    for n in calls or (C_,) * (x.shape[1] // C_):
        outs.append(eng.process(x[:, at : at + n]))
        rows.append(eng.block_stats().copy())
        at += n
    return np.concatenate(outs, axis=1), np.concatenate(rows, axis=0)


def _assert_equal(name, got, want, streams_got, streams_want=None):
    """Audio and rows of `streams_got` of `got` equal those of `streams_want` of `want`, bit for bit."""
    streams_want = streams_got if streams_want is None else streams_want
    a, ar = got
    b, br = want
    assert a.shape[1] == b.shape[1] and ar.shape[0] == br.shape[0], (name, a.shape, b.shape, ar.shape, br.shape)
    for sg, sw in zip(streams_got, streams_want):
        if not np.array_equal(a[sg], b[sw]):
            first = int(np.flatnonzero(a[sg] != b[sw])[0])
            raise AssertionError(f"{name}: stream {sg} differs from {sw} in {int((a[sg] != b[sw]).sum())} samples, first at {first}: "
                                 f"{a[sg, first]!r} != {b[sw, first]!r}")
        for f in _fields():
            assert np.array_equal(ar[f][:, sg], br[f][:, sw]), f"{name}: stream {sg}: row field {f} differs from stream {sw}'s"


def _assert_limiter_busy(name, rows, streams, n_calls):
    """limiter_peak_gr_db > 0 in the last block of every call and the first block of the next, on `streams`."""
    per_call = C_ // SL.BLOCK
    gr = rows["limiter_peak_gain_reduction_db"]
    for k in range(1, n_calls):
        for blk in (k * per_call - 1, k * per_call):
            quiet = [s for s in streams if not gr[blk, s] > 0.0]
            assert not quiet, f"{name}: the limiter is idle in block {blk} of streams {quiet[:6]}: the ring would be trivial"


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _twin(config, lookahead_ms=2.0):
    """The uninterrupted 130-stream engine over calls 1-6."""
    def make():
        eng = SL.engine(config, lookahead_ms=lookahead_ms)
        try:
            res = _run(eng, _audio()[:, : 6 * C_])
            assert eng.last_kernel() != 4, "the stage pipeline must not run with the lifecycle on"
            return res
        finally:
            eng.close()
    return _cached(("twin", config, lookahead_ms), make)


def _fresh(config):
    """A fresh 130-stream engine over the input of calls 4-6."""
    def make():
        eng = SL.engine(config)
        try:
            return _run(eng, _audio()[:, 3 * C_ : 6 * C_])
        finally:
            eng.close()
    return _cached(("fresh", config), make)


def _tail(res, first_call, n_calls=3):
    """Calls first_call .. first_call + n_calls - 1 (0-based) of a result."""
    a, r = res
    per_call = C_ // SL.BLOCK
    return a[:, first_call * C_ : (first_call + n_calls) * C_], r[first_call * per_call : (first_call + n_calls) * per_call]


# ------------------------------------------------------------------------------------------------------------- 1. restart
def _restart_case(config, listed):
    x = _audio()
    eng = SL.engine(config)
    try:
        head = _run(eng, x[:, : 3 * C_])
        with pytest.raises(RuntimeError, match="after streaming started"):
            eng.set_stream_lifecycle(False)  # configuration mode only
        eng.restart_streams(listed)
        tail = _run(eng, x[:, 3 * C_ : 6 * C_])
        counts = [eng.stream_samples_processed(s) for s in range(SL.N_STREAMS)]
    finally:
        eng.close()
    twin = _twin(config)
    others = [s for s in range(SL.N_STREAMS) if s not in set(listed)]
    _assert_limiter_busy(f"restart/{config}", twin[1], range(SL.N_STREAMS), 6)
    _assert_equal(f"restart/{config}: before the restart", head, _tail(twin, 0), range(SL.N_STREAMS))
    _assert_equal(f"restart/{config}: restarted streams against a fresh engine", tail, _fresh(config), listed)
    _assert_equal(f"restart/{config}: untouched streams against the uninterrupted twin", tail, _tail(twin, 3), others)
    assert all(counts[s] == 3 * C_ for s in listed) and all(counts[s] == 6 * C_ for s in others)
    return tail


@pytest.mark.parametrize("config", SL.CONFIGS)
def test_restart(config):
    # (config "presets": streams 0 / 63, 64 and 129 run presets 0, 1 and 2)
    tail = _restart_case(config, RESTARTED)
    if config != "dynamics":
        return
    # ... and the restarted stream IS the reference's fresh processor: one of them against the oracle
    s = 63
    x = _audio()[s, 3 * C_ : 6 * C_]
    want, want_rows = CO.run_calls(x, float(SL.FS), LC.BANDS, LC.SETTINGS, (C_,) * 3)
    d = tail[0][s].astype(np.float64) - want.astype(np.float64)
    max_abs, rms = float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))
    print(f"restart: stream {s} against the oracle: max abs {max_abs:.3e}, rms {rms:.3e}")
    assert max_abs <= PARITY_TOL[0] and rms <= PARITY_TOL[1], (max_abs, rms)
    assert (want_rows["limiter_peak_gain_reduction_db"] > 0.0).all()


# ------------------------------------------------------------------------------------------------------------- 5. list shapes
@pytest.mark.parametrize("listed", [[129], [129, 5, 64, 0, 70, 63, 1]], ids=["one", "unsorted"])
def test_restart_list_shapes(listed):
    _restart_case("dynamics", listed)


def test_restart_of_every_stream_is_a_reset():
    x = _audio()
    everyone = list(range(SL.N_STREAMS))
    eng = SL.engine("dynamics")
    try:
        _run(eng, x[:, : 3 * C_])
        eng.restart_streams(everyone)
        restarted = _run(eng, x[:, 3 * C_ : 6 * C_])
        eng.reset()  # af_engine_reset, then the same input
        reset = _run(eng, x[:, 3 * C_ : 6 * C_])
    finally:
        eng.close()
    _assert_limiter_busy("restart/all", restarted[1], everyone, 3)
    _assert_equal("restart of all 130 streams against af_engine_reset", restarted, reset, everyone)
    _assert_equal("restart of all 130 streams against a fresh engine", restarted, _fresh("dynamics"), everyone)


# ------------------------------------------------------------------------------------------------------------- 2. migrate
def _destination(config, lookahead_ms, preset):
    return SL.engine(config, n_streams=64, lookahead_ms=lookahead_ms, group_presets=[preset] if config == "presets" else None)


@pytest.mark.parametrize("lookahead_ms", [2.0, SL.SHORT_LOOKAHEAD_MS], ids=["W97", "W21"])
@pytest.mark.parametrize("config", SL.CONFIGS)
def test_migrate(config, lookahead_ms):
    x = _audio()
    a = SL.engine(config, lookahead_ms=lookahead_ms)
    try:
        assert a.limiter_lookahead_samples() == (96 if lookahead_ms == 2.0 else 20)
        _run(a, x[:, : 3 * C_])
        blobs = a.export_stream_state(MOVED_FROM)
        a_tail = _run(a, x[:, 3 * C_ : 6 * C_])
    finally:
        a.close()
    twin = _twin(config, lookahead_ms)
    _assert_limiter_busy(f"migrate/{config}", twin[1], range(SL.N_STREAMS), 6)
    _assert_equal(f"migrate/{config}: the source is not disturbed by an export", a_tail, _tail(twin, 3), range(SL.N_STREAMS))
    assert [SL.header_of(b)["samples"] for b in blobs] == [3 * C_] * 3
    # Destinations: 64 streams, two calls behind (another size, another phase: 9600 % 97 = 94, 9600 % 21 = 3).  With three
    # presets over the source's groups each moved stream goes to an engine whose group runs that stream's preset.
    plans = [(g, [MOVED_FROM[g]], [MOVED_TO[g]]) for g in range(3)] if config == "presets" else [(0, MOVED_FROM, MOVED_TO)]
    for preset, src, dst in plans:
        own = x[:64, : 5 * C_]
        d_twin = _cached(("dtwin", config, lookahead_ms, preset), lambda: _run_and_close(_destination(config, lookahead_ms, preset), own))
        d = _destination(config, lookahead_ms, preset)
        try:
            d_head = _run(d, own[:, : 2 * C_])
            d.import_stream_state(dst, [blobs[MOVED_FROM.index(s)] for s in src])
            feed = own[:, 2 * C_ :].copy()
            for s, t in zip(src, dst):
                feed[t] = x[s, 3 * C_ : 6 * C_]
            d_tail = _run(d, feed)
            counts = [d.stream_samples_processed(t) for t in dst]
        finally:
            d.close()
        others = [s for s in range(64) if s not in set(dst)]
        name = f"migrate/{config}/preset {preset}"
        _assert_equal(f"{name}: destination before the import", d_head, _tail(d_twin, 0, 2), range(64))
        _assert_equal(f"{name}: moved streams continue as in the source", d_tail, a_tail, dst, src)
        _assert_equal(f"{name}: the destination's other streams", d_tail, _tail(d_twin, 2), others)
        assert counts == [6 * C_] * len(dst)


def _run_and_close(eng, x):
    try:
        return _run(eng, x)
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------- 3. round trip, canonical form
@pytest.mark.parametrize("config", SL.CONFIGS)
def test_round_trip(config):
    x = _audio()
    eng = SL.engine(config)
    try:
        _run(eng, x[:, : 3 * C_])
        blobs = eng.export_stream_state(MOVED_FROM)
        again = eng.export_stream_state(MOVED_FROM)
        assert blobs == again, "two exports in a row differ"
        assert all(len(b) == eng.stream_state_size() for b in blobs)
        eng.import_stream_state(MOVED_FROM, blobs)
        assert eng.export_stream_state(MOVED_FROM[::-1]) == blobs[::-1], "an import into the same slot changed the state"
        tail = _run(eng, x[:, 3 * C_ : 6 * C_])
    finally:
        eng.close()
    twin = _twin(config)
    _assert_limiter_busy(f"round trip/{config}", twin[1], MOVED_FROM, 6)
    _assert_equal(f"round trip/{config}", tail, _tail(twin, 3), range(SL.N_STREAMS))


@pytest.mark.parametrize("config, lookahead_ms", [(c, 2.0) for c in SL.CONFIGS] + [("dynamics", SL.SHORT_LOOKAHEAD_MS)])
def test_blob_is_free_of_the_engines_phase(config, lookahead_ms):
    """Two engines over the same per-stream input, the second one call further on its own sample axis: it ran one more call
    first, after which the slots were restarted.  The same stream exports the same bytes from both."""
    x = _audio()
    same = x[:, C_ : 4 * C_]
    first = SL.engine(config, lookahead_ms=lookahead_ms)
    second = SL.engine(config, lookahead_ms=lookahead_ms)
    try:
        rows = _run(first, same)[1]
        want = first.export_stream_state(MOVED_FROM)
        _run(second, x[:, 6 * C_ : 7 * C_])
        second.restart_streams(MOVED_FROM)
        _run(second, same)
        got = second.export_stream_state(MOVED_FROM)
        assert first.samples_processed() + C_ == second.samples_processed() == 4 * C_
    finally:
        first.close()
        second.close()
    _assert_limiter_busy(f"phase-free/{config}", rows, MOVED_FROM, 3)
    for s, a, b in zip(MOVED_FROM, got, want):
        if a != b:
            diff = np.flatnonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))
            raise AssertionError(f"{config}: stream {s}: {diff.size} bytes differ between the engines, first at offset {int(diff[0])}")
        assert SL.header_of(a)["samples"] == 3 * C_


# ------------------------------------------------------------------------------------------- 4. refusals on the device path
def _refused(eng, match):
    size = eng.stream_state_size()
    for call in (lambda: eng.restart_streams([3, 70]), lambda: eng.export_stream_state([3, 70]),
                 lambda: eng.import_stream_state([3], [bytes(size)])):
        try:
            call()
        except NotImplementedError as err:
            assert match in str(err), err
        except ValueError as err:  # (the import's header check comes before the engine's state: a zero blob is no blob)
            assert "magic" in str(err), err
        else:
            raise AssertionError(f"a lifecycle call was accepted although {match}")


def test_refused_while_samples_are_pending():
    x = _audio()
    tried, plain = SL.engine("suppressor-gate"), SL.engine("suppressor-gate")
    try:
        for eng in (tried, plain):
            _run(eng, x[:, : 3 * C_])
        good = tried.export_stream_state([3])[0]
        outs = []
        for eng in (tried, plain):
            outs.append([eng.process(x[:, 3 * C_ : 3 * C_ + 4700])])  # nine frames out, 380 samples wait
            if eng is tried:
                _refused(eng, "pending")
                with pytest.raises(NotImplementedError, match="pending"):
                    eng.import_stream_state([3], [good])
            outs[-1].append(eng.process(x[:, 3 * C_ + 4700 : 4 * C_]))  # the tenth frame: 19 200 samples, twenty blocks
        assert outs[0][0].shape[1] == 4320 and outs[0][1].shape[1] == 480
        for a, b in zip(*outs):
            assert np.array_equal(a, b)
        everyone = list(range(SL.N_STREAMS))
        assert tried.export_stream_state(everyone) == plain.export_stream_state(everyone)
    finally:
        tried.close()
        plain.close()


def test_refused_while_a_crossfade_is_in_flight():
    x = _audio()
    tried, plain = SL.engine("dynamics", live=True), SL.engine("dynamics", live=True)
    try:
        for eng in (tried, plain):
            _run(eng, x[:, : 3 * C_])
        good = tried.export_stream_state([3])[0]
        outs = []
        for eng in (tried, plain):
            eng.eq_set_band_gain(3, 6.0)  # a live setter: a 72-sample crossfade from the next call's first sample on
            if eng is tried:
                _refused(eng, "crossfade is in flight")
                with pytest.raises(NotImplementedError, match="crossfade is in flight"):
                    eng.import_stream_state([3], [good])
            outs.append(eng.process(x[:, 3 * C_ : 4 * C_]))
        assert np.array_equal(outs[0], outs[1])
        everyone = list(range(SL.N_STREAMS))
        assert tried.export_stream_state(everyone) == plain.export_stream_state(everyone)  # the crossfade has ended: accepted
        # ... and a sample count that is no whole number of control blocks
        tried.process(x[:, 4 * C_ : 4 * C_ + 100])
        _refused(tried, "not a whole number")
    finally:
        tried.close()
        plain.close()
