"""CPU checks of the streaming lane chain's boundary (af_lane_chain_*, mic_eq_mi.LaneChain, route="lanes"): creating,
configuring and destroying an object is host work; every argument error gives its status and a message that names the argument
before any device work; the settings a lane does not run are refused by name; and simulate_auto_eq_chain_batch without the
keyword, or with route="groups", takes the path it always took.  No GPU is touched here."""
import ctypes as C

import numpy as np
import pytest

import lane_chain_stimulus as LS

AF_OK, AF_ERR_INVALID_ARGUMENT = 0, -1
BANDS = LS.bands(0)


@pytest.fixture(scope="module")
def mi():
    import mic_eq_mi

    assert mic_eq_mi.CORE_AVAILABLE, "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    return mic_eq_mi


@pytest.fixture(scope="module")
def lib(mi):
    from mic_eq_mi import _lib

    return _lib.load()


def error(lib) -> str:
    return lib.af_last_error().decode()


def create(lib, fs=48_000.0, n_streams=4, lookahead_ms=2.0, device=0):
    h = C.c_void_p()
    return lib.af_lane_chain_create(fs, n_streams, lookahead_ms, device, C.byref(h)), h


def default_record(lib):
    from mic_eq_mi._lib import LaneChainSettings

    r = LaneChainSettings()
    assert lib.af_lane_chain_default_settings(C.byref(r)) == AF_OK
    return r


def test_create_configure_and_destroy_are_host_only(mi, lib):
    rc, h = create(lib, n_streams=70)
    assert rc == AF_OK and h.value
    r = default_record(lib)
    # simulate_auto_eq_chain's defaults (python_api.rs:400-487)
    assert (r.compressor_threshold_db, r.compressor_ratio, r.compressor_attack_ms, r.compressor_release_ms) == (-20.0, 4.0, 10.0, 200.0)
    assert (r.compressor_makeup_gain_db, r.compressor_base_release_ms, r.limiter_ceiling_db, r.limiter_release_ms) == (0.0, 50.0, -0.5, 50.0)
    assert (r.eq_enabled, r.compressor_enabled, r.limiter_enabled) == (1, 1, 1)
    assert (r.compressor_adaptive_release, r.compressor_sidechain_highpass_enabled, r.limiter_careful_output_enabled) == (0, 1, 1)
    streams = (C.c_int32 * 2)(3, 69)
    records = (type(r) * 2)(r, r)
    assert lib.af_lane_chain_configure(h, streams, 2, records) == AF_OK
    n = C.c_int64(-1)
    assert lib.af_lane_chain_samples_processed(h, 69, C.byref(n)) == AF_OK and n.value == 0
    assert lib.af_lane_chain_blocks(h) == 0
    ms = C.c_double(-1.0)
    assert lib.af_lane_chain_last_kernel_ms(h, C.byref(ms)) == AF_OK and ms.value == 0.0
    assert lib.af_lane_chain_reset(h) == AF_OK
    # n_samples == 0 is a no-op that touches no device
    x = np.zeros((70, 4), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    assert lib.af_lane_chain_process_host(h, x.ctypes.data_as(fp), x.ctypes.data_as(fp), 0, 4) == AF_OK
    lib.af_lane_chain_destroy(h)
    lib.af_lane_chain_destroy(None)
    chain = mi.LaneChain(44_100.0, 5, limiter_lookahead_ms=1.0)
    chain.configure([0, 4], BANDS, {"compressor_threshold_db": -30.0, "limiter_lookahead_ms": 1.0})
    chain.configure(range(5), [LS.bands(i) for i in range(5)], [LS.settings(i, lookahead_ms=1.0) for i in range(5)])
    assert chain.samples_processed(4) == 0 and chain.block_stats().shape == (0, 5) and chain.last_kernel_ms() == 0.0
    chain.reset()
    chain.close()


def test_create_argument_errors(lib):
    assert lib.af_lane_chain_create(48_000.0, 4, 2.0, 0, None) == AF_ERR_INVALID_ARGUMENT and "out" in error(lib)
    for kwargs, name in (({"fs": float("nan")}, "sample_rate"), ({"fs": 0.0}, "sample_rate"), ({"n_streams": 0}, "n_streams"),
                         ({"n_streams": -3}, "n_streams"), ({"lookahead_ms": float("inf")}, "limiter_lookahead_ms"),
                         ({"lookahead_ms": 0.0}, "limiter_lookahead_ms"), ({"device": -1}, "device")):
        rc, h = create(lib, **kwargs)
        assert rc == AF_ERR_INVALID_ARGUMENT and not h.value and name in error(lib), (kwargs, error(lib))


def test_configure_argument_errors(lib):
    rc, h = create(lib, n_streams=4)
    assert rc == AF_OK
    r = default_record(lib)
    one = (C.c_int32 * 1)(0)
    records = (type(r) * 2)(r, r)
    assert lib.af_lane_chain_configure(None, one, 1, records) == AF_ERR_INVALID_ARGUMENT and "handle" in error(lib)
    assert lib.af_lane_chain_configure(h, None, 1, records) == AF_ERR_INVALID_ARGUMENT and "streams" in error(lib)
    assert lib.af_lane_chain_configure(h, one, 1, None) == AF_ERR_INVALID_ARGUMENT and "settings" in error(lib)
    assert lib.af_lane_chain_configure(h, one, 0, records) == AF_ERR_INVALID_ARGUMENT and "n must" in error(lib)
    for pair in ((0, 4), (-1, 0)):
        assert lib.af_lane_chain_configure(h, (C.c_int32 * 2)(*pair), 2, records) == AF_ERR_INVALID_ARGUMENT
        assert "streams[" in error(lib) and "out of range" in error(lib)
    assert lib.af_lane_chain_configure(h, (C.c_int32 * 2)(2, 2), 2, records) == AF_ERR_INVALID_ARGUMENT
    assert "streams[1] = 2" in error(lib) and "twice" in error(lib)
    for poke in ("compressor_threshold_db", "compressor_ratio", "compressor_attack_ms", "compressor_release_ms",
                 "compressor_makeup_gain_db", "compressor_base_release_ms", "limiter_ceiling_db", "limiter_release_ms", "bands"):
        bad = default_record(lib)
        if poke == "bands":
            bad.bands[7][1] = float("nan")
        else:
            setattr(bad, poke, float("inf"))
        assert lib.af_lane_chain_configure(h, (C.c_int32 * 2)(1, 3), 2, (type(r) * 2)(r, bad)) == AF_ERR_INVALID_ARGUMENT, poke
        assert "settings[1]" in error(lib) and "finite" in error(lib)
    n = C.c_int64(0)
    assert lib.af_lane_chain_samples_processed(h, 4, C.byref(n)) == AF_ERR_INVALID_ARGUMENT and "stream" in error(lib)
    assert lib.af_lane_chain_samples_processed(h, 0, None) == AF_ERR_INVALID_ARGUMENT and "out" in error(lib)
    assert lib.af_lane_chain_last_kernel_ms(h, None) == AF_ERR_INVALID_ARGUMENT and "ms" in error(lib)
    assert lib.af_lane_chain_read_rows(h, None, 0) == AF_ERR_INVALID_ARGUMENT and "rows" in error(lib)
    lib.af_lane_chain_destroy(h)


def test_process_argument_errors_come_before_device_work(lib):
    rc, h = create(lib, n_streams=4)
    assert rc == AF_OK
    x = np.zeros((4, 16), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    p = x.ctypes.data_as(fp)
    assert lib.af_lane_chain_process_host(None, p, p, 16, 16) == AF_ERR_INVALID_ARGUMENT and "handle" in error(lib)
    assert lib.af_lane_chain_process_host(h, None, p, 16, 16) == AF_ERR_INVALID_ARGUMENT and "in is null" in error(lib)
    assert lib.af_lane_chain_process_host(h, p, None, 16, 16) == AF_ERR_INVALID_ARGUMENT and "out is null" in error(lib)
    assert lib.af_lane_chain_process_host(h, p, p, 16, 15) == AF_ERR_INVALID_ARGUMENT and "stride" in error(lib)
    assert lib.af_lane_chain_process_host(h, p, p, -1, 16) == AF_ERR_INVALID_ARGUMENT and "n_samples" in error(lib)
    assert lib.af_lane_chain_process_device(h, None, None, 16, 16, None) == AF_ERR_INVALID_ARGUMENT and "in is null" in error(lib)
    assert lib.af_lane_chain_process_device(h, 4096, 4096, 16, 8, None) == AF_ERR_INVALID_ARGUMENT and "stride" in error(lib)
    lib.af_lane_chain_destroy(h)


REFUSED = ({"deesser_enabled": True}, {"compressor_auto_makeup_enabled": True}, {"eq_bands_v2": []}, {"eq_before_deesser": True},
           {"limiter_lookahead_ms": 1.0})


@pytest.mark.parametrize("setting", REFUSED, ids=lambda d: next(iter(d)))
def test_out_of_scope_settings_are_refused_by_name(mi, setting):
    name = next(iter(setting))
    chain = mi.LaneChain(48_000.0, 3)
    try:
        with pytest.raises(NotImplementedError, match=name):
            chain.configure([1], BANDS, setting)
        with pytest.raises(NotImplementedError, match=name):
            chain.configure([0, 2], BANDS, [None, dict(LS.engine_settings(LS.settings(2)), **setting)])
    finally:
        chain.close()
    audio = np.zeros((3, 8), dtype=np.float32)
    with pytest.raises(NotImplementedError, match=name):
        mi.simulate_auto_eq_chain_batch(audio, 48_000, BANDS, [None, None, setting], route="lanes")


def test_python_argument_errors(mi):
    chain = mi.LaneChain(48_000.0, 3)
    try:
        with pytest.raises(ValueError, match="expected 10 EQ bands"):
            chain.configure([0], BANDS[:9], None)
        with pytest.raises(ValueError, match="one preset per stream"):
            chain.configure([0, 1], [BANDS], [None, None])
        with pytest.raises(ValueError, match="twice"):
            chain.configure([1, 1], BANDS, None)
        with pytest.raises(ValueError, match="out of range"):
            chain.configure([3], BANDS, None)
        with pytest.raises(TypeError, match="must be a bool"):
            chain.configure([0], BANDS, {"limiter_enabled": 1.0})
        with pytest.raises(ValueError, match="n_streams"):
            chain.process(np.zeros((2, 8), dtype=np.float32))
    finally:
        chain.close()
    with pytest.raises(ValueError, match="sample_rate"):
        mi.LaneChain(float("nan"), 1)
    with pytest.raises(ValueError, match="n_streams"):
        mi.LaneChain(48_000.0, 0)
    audio = np.zeros((2, 8), dtype=np.float32)
    with pytest.raises(ValueError, match="route"):
        mi.simulate_auto_eq_chain_batch(audio, 48_000, BANDS, None, route="waves")
    with pytest.raises(ValueError, match="expected 10 EQ bands"):
        mi.simulate_auto_eq_chain_batch(audio, 48_000, BANDS[:3], None, route="lanes")
    with pytest.raises(ValueError, match="one preset per stream"):
        mi.simulate_auto_eq_chain_batch(audio, 48_000, BANDS, [None], route="lanes")


def test_default_route_is_the_group_route(mi, monkeypatch):
    """Without the keyword and with route="groups" the call goes where it always went: the old argument checks in the old
    order, then an Engine over packed groups of 64 -- seen here on a stand-in Engine, so that nothing reaches a device."""
    from mic_eq_mi import lane_chain, mic_eq_core as core

    audio = np.zeros((3, 8), dtype=np.float32)
    for kwargs in ({}, {"route": "groups"}):
        with pytest.raises(ValueError, match="expected 10 EQ bands"):
            mi.simulate_auto_eq_chain_batch(audio, 48_000, BANDS[:3], None, **kwargs)
        with pytest.raises(ValueError, match="one preset per stream"):
            mi.simulate_auto_eq_chain_batch(audio, 48_000, BANDS, [None], **kwargs)
        with pytest.raises(TypeError, match="n_streams, n_samples"):
            mi.simulate_auto_eq_chain_batch(audio[0], 48_000, BANDS, None, **kwargs)

    class GroupRoute(Exception):
        pass

    def engine_stand_in(sample_rate, n_streams, device=0):
        raise GroupRoute(n_streams)

    def lanes_stand_in(*args, **kwargs):
        raise AssertionError("the lane route was taken")

    monkeypatch.setattr(core, "Engine", engine_stand_in)
    monkeypatch.setattr(lane_chain, "simulate_lanes", lanes_stand_in)
    presets = [{"compressor_threshold_db": -30.0}, {"deesser_enabled": True}, {"compressor_threshold_db": -30.0}]
    for kwargs in ({}, {"route": "groups"}):
        with pytest.raises(GroupRoute) as info:
            core.simulate_auto_eq_chain_batch(audio, 48_000, BANDS, presets, **kwargs)
        assert info.value.args == (128,)  # two distinct presets, each padded to a group of 64; the de-esser is not refused here
