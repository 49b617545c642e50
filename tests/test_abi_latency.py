"""The argument contract of the latency calibration (af_latency_*) and the host-only parts of mic_eq_mi.latency_calibration:
every check runs on the host, before any GPU work, so these pass without a device."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import latency_oracle as LO
import latency_stimulus as LS


@pytest.fixture(scope="module")
def mi():
    import mic_eq_mi

    assert mic_eq_mi.CORE_AVAILABLE
    return mic_eq_mi


def test_create_rejects_bad_arguments(mi):
    probe = LS.probe()
    for rate in (0.0, -48_000.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sample_rate"):
            mi.LatencyCalibration(rate, probe, 4, LS.LONG)
    with pytest.raises(ValueError, match="probe_samples"):
        mi.LatencyCalibration(48_000, probe[:15], 4, LS.LONG)
    with pytest.raises(ValueError, match="finite"):
        mi.LatencyCalibration(48_000, np.where(np.arange(probe.size) == 7, np.nan, probe), 4, LS.LONG)
    with pytest.raises(ValueError, match="max_streams"):
        mi.LatencyCalibration(48_000, probe, 0, LS.LONG)
    with pytest.raises(ValueError, match="max_record_samples"):
        mi.LatencyCalibration(48_000, probe, 4, 0)
    with pytest.raises(ValueError, match="device"):
        mi.LatencyCalibration(48_000, probe, 4, LS.LONG, -1)
    # 2^18 real points hold a recording of 262144 - 312 samples at 48 kHz: 5.4 s
    with pytest.raises(ValueError, match=r"transform of 524288 real points; at most 262144 .*5\.4 s at 48 kHz"):
        mi.LatencyCalibration(48_000, probe, 4, (1 << 18) - 311)
    mi.LatencyCalibration(48_000, probe, 4, (1 << 18) - 312).close()


def test_layout_is_the_reference_burst_layout(mi):
    for rate in LS.RATES:
        probe = LS.probe(rate)
        burst, offsets = LO.coded_probe_components(rate, probe.size)
        lc = mi.LatencyCalibration(rate, probe, 1, 4 * probe.size)
        assert (lc.offsets, lc.burst_samples) == (offsets, burst.size)
        assert lc.local_radius == max(int(round(rate * 0.010)), burst.size)
        lc.close()
        lc.close()
    assert LO.coded_probe_components(16_000, LS.probe(16_000).size)[0].size == 13 * 6  # the chip length went from 8 to 6


def test_analyze_rejects_invalid_arguments_on_the_host(mi):
    from mic_eq_mi import _lib
    from mic_eq_mi.latency_calibration import _Result, _Search

    lc = mi.LatencyCalibration(48_000, LS.probe(), 3, 5000)
    lib = _lib.load()
    audio = np.zeros((3, 5000), dtype=np.float32)
    search = (_Search * 3)()
    for q in search:
        q.min_search_ms, q.max_search_ms, q.route_supported = 5.0, 500.0, 1
    lengths = np.asarray([5000, 4000, 0], dtype=np.int64)
    lp = lengths.ctypes.data_as(C.POINTER(C.c_int64))
    for run in (lib.af_latency_analyze_host, lib.af_latency_analyze_device):
        pointer = audio.ctypes.data_as(C.POINTER(C.c_float)) if run is lib.af_latency_analyze_host else C.c_void_p(audio.ctypes.data)
        for args, text in (((None, 5000, 5000, 3, lp, search), "null"), ((pointer, 5000, 5000, 3, lp, None), "null"),
                           ((pointer, 5000, 4999, 3, lp, search), "stride"), ((pointer, 5000, 5000, 0, lp, search), "n_streams"),
                           ((pointer, 5000, 5000, 4, lp, search), r"n_streams must be in 1\.\.3"),
                           ((pointer, 0, 5000, 3, lp, search), "n_samples"), ((pointer, 5001, 5001, 3, lp, search), "max_record_samples"),
                           ((pointer, 4500, 5000, 3, lp, search), r"lengths\[0\]")):
            with pytest.raises(ValueError, match=text):
                _lib.check(run(lc._h, *args))
        search[1].max_search_ms = float("nan")
        with pytest.raises(ValueError, match=r"search\[1\].*finite"):
            _lib.check(run(lc._h, pointer, 5000, 5000, 3, lp, search))
        search[1].max_search_ms = 500.0
    with pytest.raises(RuntimeError, match="no analysis"):
        _lib.check(lib.af_latency_read_results(lc._h, (_Result * 3)(), 3))
    with pytest.raises(RuntimeError, match="no analysis"):
        lc.scores(0)
    with pytest.raises(ValueError, match="one value per stream"):
        lc.analyze(audio, max_search_ms=[500.0, 400.0])
    with pytest.raises(ValueError, match="lengths"):
        lc.analyze(audio, lengths=[5000, 4000])
    with pytest.raises(TypeError):
        lc.analyze(audio[0])
    with pytest.raises(ValueError, match="power of two"):
        lc.debug_rfft(np.zeros(1000, dtype=np.float32))
    assert lc.last_kernel_ms() == 0.0
    assert lib.af_latency_message_text(0, 0) == b"ok" and lib.af_latency_message_text(5, 0) == LO.NON_FINITE_MESSAGE.encode()
    assert lib.af_latency_message_text(6, 0) is None and lib.af_latency_message_text(0, 4) is None
    lc.close()


def test_host_only_exits_of_the_single_call_and_the_dataclass(mi):
    assert [f.name for f in dataclasses.fields(mi.LatencyCalibrationResult)] == list(LO.FIELDS)
    r = mi.LatencyCalibrationResult(True, 1.0, 0.0, 1.0, 0.5, 48)
    assert (r.message, r.repetition_count, r.agreement_ms, r.ambiguity_score, r.sub_sample_offset, r.route_latency_ms,
            r.directional_latency_ms, r.route_kind, r.compensation_basis) == ("", 0, 0.0, 0.0, 0.0, 0.0, None, "output_to_input",
                                                                               "measured_output_to_input_route")
    probe = LS.probe()
    for got, want in ((mi.analyze_latency(probe, LS.recording("bad_route"), route_kind=" Input_To_Output "),
                       LO._failed("Unsupported latency route; expected output_to_input.", "input_to_output")),
                      (mi.analyze_latency(None, probe), LO._failed("Missing probe or recording.")),
                      (mi.analyze_latency(probe, None), LO._failed("Missing probe or recording.")),
                      (mi.analyze_latency(probe[:15], probe), LO._failed("Recording too short for reliable correlation.")),
                      (mi.analyze_latency(probe, LS.recording("too_short")), LO._failed("Recording too short for reliable correlation."))):
        assert dataclasses.asdict(got) == want


def test_probe_and_profile_follow_the_reference(mi):
    golden = np.load(LS.GOLDEN)
    for rate in LS.RATES:
        got = mi.generate_probe_signal(rate, LS.PROBE_MS[rate])
        assert got.dtype == np.float32 and np.array_equal(got, golden[f"probe_{rate}"])
    assert mi.generate_probe_signal().size == 3840 and mi.generate_probe_signal(48_000, 0.0).size == 1
    assert abs(float(np.max(np.abs(mi.generate_probe_signal(amplitude=0.25)))) - 0.25) < 1e-7
    r = mi.LatencyCalibrationResult(True, 12.5, 0.0, 12.5, 0.9, 600, "ok", 4, 0.01, 0.6, 600.0, 12.5)
    profile = mi.result_to_profile(r, 44_100, engine_latency_ms=-3.0, engine_config_signature=7)
    assert list(profile) == ["measured_round_trip_ms", "estimated_one_way_ms", "applied_compensation_ms", "route_latency_ms",
                             "directional_latency_ms", "route_kind", "compensation_basis", "confidence", "agreement_ms",
                             "ambiguity_score", "repetition_count", "sample_rate", "engine_latency_ms", "total_latency_ms",
                             "engine_config_signature", "timestamp_utc"]
    assert profile["total_latency_ms"] == 12.5 and profile["engine_latency_ms"] == 0.0 and profile["engine_config_signature"] == "7"
    assert profile["sample_rate"] == 44_100 and profile["directional_latency_ms"] is None and profile["timestamp_utc"].endswith("+00:00")
    legacy = mi.LatencyCalibrationResult(True, 8.0, 0.0, 9.0, 0.9, 400)  # route_latency_ms 0: the larger of the legacy fields
    assert mi.result_to_profile(legacy, engine_latency_ms=2.0)["total_latency_ms"] == 11.0
