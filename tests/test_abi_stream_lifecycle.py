"""The per-stream lifecycle's host side (af_engine_set_stream_lifecycle and the five entry points behind it) on a machine
without a GPU: the switch, every argument error, every refusal that the engine's configuration decides, header validation of
hand-made blobs, and the blob size against the documented layout.  An engine cannot start here, so every call below returns
before its first HIP call -- a call that reached the runtime would fail with a backend RuntimeError that names it."""
import ctypes as C

import numpy as np
import pytest

import stream_lifecycle_cases as SL


@pytest.fixture(scope="module")
def core():
    import mic_eq_mi
    from mic_eq_mi import mic_eq_core

    assert mic_eq_mi.CORE_AVAILABLE
    return mic_eq_core


NOT_STARTED = "streaming has not started"


def _calls(eng, blob=None):
    """The three entry points that take a list, as callables of the list."""
    if blob is None:  # a well-formed blob of the default chain (with a gate row where the engine has a gate plane)
        h, size = _documented_header("dynamics")
        if eng.stream_state_size() != size:
            h, size = dict(h, gate_plane=1, blob_bytes=size + 8 * SL.GATE_WORDS), size + 8 * SL.GATE_WORDS
        blob = _blob(h, size)
    return {
        "restart": eng.restart_streams,
        "export": eng.export_stream_state,
        "import": lambda idx: eng.import_stream_state(idx, [blob] * len(list(idx))),
    }


def test_switch_is_host_only_and_off_by_default(core):
    eng = SL.engine("dynamics", lifecycle=False)
    try:
        for name, call in _calls(eng).items():
            with pytest.raises(RuntimeError, match="af_engine_set_stream_lifecycle"):
                call([0])
        eng.set_stream_lifecycle(True)  # no device needed
        with pytest.raises(RuntimeError, match=NOT_STARTED):
            eng.restart_streams([0])
        eng.set_stream_lifecycle(False)
        with pytest.raises(RuntimeError, match="af_engine_set_stream_lifecycle"):
            eng.restart_streams([0])
        eng.reset()  # a reset keeps the engine in configuration mode, where the switch is a setter like any other
        eng.set_stream_lifecycle(True)
        assert eng.stream_samples_processed(0) == 0
    finally:
        eng.close()
    with pytest.raises(ValueError, match="engine is null"):
        core._lib.check(core._lib.load().af_engine_set_stream_lifecycle(None, 1))


def test_argument_errors_come_first(core):
    eng = SL.engine("dynamics")
    lib = eng._lib
    try:
        for name, call in _calls(eng).items():
            with pytest.raises(ValueError, match="repeats stream 5"):
                call([5, 7, 5])
            with pytest.raises(ValueError, match="out of range for 130 streams"):
                call([0, SL.N_STREAMS])
            with pytest.raises(ValueError, match="out of range"):
                call([-1])
            with pytest.raises(RuntimeError, match=NOT_STARTED):  # a valid list, unsorted, every stream: only the state refuses
                call(list(range(SL.N_STREAMS))[::-1])
        one = (C.c_int32 * 1)(3)
        buf = (C.c_ubyte * eng.stream_state_size())()
        for fn, args in ((lib.af_engine_restart_streams, ()), (lib.af_engine_export_stream_state, (C.cast(buf, C.c_void_p),)),
                         (lib.af_engine_import_stream_state, (C.cast(buf, C.c_void_p),))):
            with pytest.raises(ValueError, match="negative"):
                core._lib.check(fn(eng._h, one, -1, *args))
            with pytest.raises(ValueError, match="list is null"):
                core._lib.check(fn(eng._h, None, 1, *args))
            with pytest.raises(ValueError, match="engine is null"):
                core._lib.check(fn(None, one, 1, *args))
        for fn in (lib.af_engine_export_stream_state, lib.af_engine_import_stream_state):
            with pytest.raises(ValueError, match="blobs is null"):
                core._lib.check(fn(eng._h, one, 1, None))
        with pytest.raises(ValueError, match="null argument"):
            core._lib.check(lib.af_engine_stream_state_size(eng._h, None))
        with pytest.raises(ValueError, match="out of range"):
            eng.stream_samples_processed(SL.N_STREAMS)
        with pytest.raises(ValueError, match="null argument"):
            core._lib.check(lib.af_engine_stream_samples_processed(eng._h, 0, None))
        with pytest.raises(ValueError, match="expected 2 blobs"):
            eng.import_stream_state([0, 1], [bytes(eng.stream_state_size())])
        with pytest.raises(ValueError, match="bytes"):
            eng.import_stream_state([0], [b"short"])
    finally:
        eng.close()


@pytest.mark.parametrize("rule, configure", [
    ("device-rate I/O", lambda e: e.set_io_sample_rates(44_100, 48_000)),
    ("device-rate I/O", lambda e: e.set_io_sample_rates(48_000, 44_100)),
    ("multichannel input", lambda e: e.set_input_channels(2, 0)),
    ("output writer", lambda e: e.set_output_writer(1)),
    ("VAD-fused gate", lambda e: (e.set_gate_enabled(1), e.gate_set_vad_auto_gate_enabled(1))),
    ("stage pipeline", lambda e: e.set_kernel(4)),
])
def test_configuration_refusals_need_no_device(core, rule, configure):
    eng = SL.engine("dynamics")
    try:
        configure(eng)
        for name, call in _calls(eng).items():
            with pytest.raises(NotImplementedError, match=rule):
                call([0, 64, 129])
            with pytest.raises(ValueError, match="repeats"):  # ... but a bad list is still a bad list
                call([1, 1])
    finally:
        eng.close()


def test_forced_stage_pipeline_is_refused_at_the_first_call(core):
    eng = SL.engine("dynamics")
    try:
        eng.set_kernel(4)
        with pytest.raises(NotImplementedError, match="hand-over rings"):
            eng.process(np.zeros((SL.N_STREAMS, SL.BLOCK), dtype=np.float32))
        eng.set_stream_lifecycle(False)  # still configuration mode: the refused call started nothing
    finally:
        eng.close()


# ---- the documented layout: default chain; de-esser + auto-makeup; suppressor + gate (ten one-section EQ bands, W = 97,
# 20 meter slots of 960 samples in 400 ms)
SHAPES = {
    "dynamics": dict(n_eq_sections=10, lookahead=96, meter_slots=0, suppressor=0, gate_plane=0, live_rows=0,
                     stage_flags=SL.FLAG_EQ | SL.FLAG_COMP | SL.FLAG_LIM | SL.FLAG_SCRUB),
    "deesser-makeup": dict(n_eq_sections=10, lookahead=96, meter_slots=20, suppressor=0, gate_plane=0, live_rows=0,
                           stage_flags=SL.FLAG_DEESSER | SL.FLAG_EQ | SL.FLAG_COMP | SL.FLAG_LIM | SL.FLAG_SCRUB | SL.FLAG_AUTO_MAKEUP),
    "suppressor-gate": dict(n_eq_sections=10, lookahead=96, meter_slots=0, suppressor=1, gate_plane=1, live_rows=0,
                            stage_flags=SL.FLAG_EQ | SL.FLAG_COMP | SL.FLAG_LIM | SL.FLAG_SCRUB),
}


def _documented_header(config, **changes):
    shape = dict(SHAPES[config], sample_rate=float(SL.FS), control_block=SL.BLOCK)
    shape["rows64"] = SL.rows64(shape["n_eq_sections"], shape["meter_slots"], bool(shape["live_rows"]))
    shape["rows32"] = SL.F32_FIXED + shape["lookahead"] + 1
    size = SL.blob_bytes(shape["rows64"], shape["lookahead"] + 1, bool(shape["gate_plane"]), bool(shape["suppressor"]))
    h = dict(shape, magic=SL.MAGIC, version=SL.VERSION, header_bytes=SL.HEADER_BYTES, blob_bytes=size, samples=0)
    h.update(changes)
    return h, size


def _blob(h, size):
    return SL.HEADER.pack(*(h[f] for f in SL.HEADER_FIELDS)) + bytes(size - SL.HEADER_BYTES)


@pytest.mark.parametrize("config", sorted(SHAPES))
def test_state_size_agrees_with_the_documented_layout(core, config):
    eng = SL.engine(config)
    try:
        h, size = _documented_header(config)
        assert eng.stream_state_size() == size
        assert size == {"dynamics": 1800, "deesser-makeup": 2000, "suppressor-gate": 12208}[config]
        # a blob with exactly the documented header passes validation: what refuses it is that the engine has not started
        with pytest.raises(RuntimeError, match=NOT_STARTED):
            eng.import_stream_state([129], [_blob(h, size)])
    finally:
        eng.close()
    if config == "dynamics":  # live control: fifteen more f64 rows
        live = SL.engine(config, live=True)
        try:
            assert live.stream_state_size() == size + 8 * 15
        finally:
            live.close()


@pytest.mark.parametrize("config", sorted(SHAPES))
def test_header_validation_names_the_field(core, config):
    eng = SL.engine(config)
    try:
        good, size = _documented_header(config)
        for field, value in (("magic", SL.MAGIC ^ 0x100), ("version", SL.VERSION + 1), ("header_bytes", SL.HEADER_BYTES + 8),
                             ("blob_bytes", size + 8), ("sample_rate", 44_100.0)):
            with pytest.raises(ValueError, match=rf"blob 1 for stream 64: stream state blob: {field} is"):
                eng.import_stream_state([0, 64], [_blob(good, size), _blob(dict(good, **{field: value}), size)])
        for field in SL.SHAPE_FIELDS:  # each shape field off by one, either way
            for delta in (1, -1):
                bad = dict(good, **{field: good[field] + delta})
                if bad[field] < 0:
                    continue
                with pytest.raises(ValueError, match=rf"stream state blob: {field} is"):
                    eng.import_stream_state([7], [_blob(bad, size)])
        # the stream's own sample count is carried, not checked
        with pytest.raises(RuntimeError, match=NOT_STARTED):
            eng.import_stream_state([7], [_blob(dict(good, samples=123_456_789), size)])
    finally:
        eng.close()


def test_header_is_checked_against_the_slots_own_preset(core):
    """Three presets over three groups: preset 2 turns adaptive release on (a parameter: same shape), so every slot takes the
    same shape here; a preset with another lookahead changes the shape of its own group's slots only."""
    from mic_eq_mi import mic_eq_core as mc

    eng = SL.engine("presets")
    try:
        good, size = _documented_header("dynamics")
        assert eng.stream_state_size() == size
        with pytest.raises(RuntimeError, match=NOT_STARTED):
            eng.import_stream_state([0, 64, 128], [_blob(good, size)] * 3)
        eng.select_preset(1)
        eng.limiter_set_lookahead_ms(SL.SHORT_LOOKAHEAD_MS)  # W = 21 in group 1; the planes keep the capacity of W = 97
        assert eng.limiter_lookahead_samples() == 20
        assert eng.stream_state_size() == size
        with pytest.raises(ValueError, match="blob 1 for stream 64: stream state blob: lookahead is 96, the destination slot has 20"):
            eng.import_stream_state([0, 64, 128], [_blob(good, size)] * 3)
        with pytest.raises(RuntimeError, match=NOT_STARTED):
            eng.import_stream_state([0, 64, 128], [_blob(good, size), _blob(dict(good, lookahead=20), size), _blob(good, size)])
    finally:
        eng.close()
    assert mc is core
