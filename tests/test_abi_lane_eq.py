"""The argument contract of the per-lane EQ (af_lane_eq_*) and of the headroom operators: every check runs on the host, before any
GPU work, so these pass without a device."""
import numpy as np
import pytest

import headroom_stimulus as HS


@pytest.fixture(scope="module")
def mi():
    import mic_eq_mi

    assert mic_eq_mi.CORE_AVAILABLE
    return mic_eq_mi


BANDS = np.asarray([[(f, g, q) for f, g, q in zip(HS.FREQS, HS.GAINS[1], HS.QS[1])]] * 3, dtype=np.float64)


def test_create_rejects_a_bad_rate_or_device(mi):
    for rate in (0.0, -48_000.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sample_rate"):
            mi.LaneEq(rate)
    with pytest.raises(ValueError, match="device"):
        mi.LaneEq(48_000.0, -1)


def test_run_rejects_invalid_arguments_on_the_host(mi):
    import ctypes as C

    from mic_eq_mi import _lib

    eq = mi.LaneEq(48_000.0)
    lib = _lib.load()
    audio = np.zeros((2, 100), dtype=np.float32)
    lanes = np.asarray([0, 1, 1], dtype=np.int32)
    fp, ip, dp = audio.ctypes.data_as(C.POINTER(C.c_float)), lanes.ctypes.data_as(C.POINTER(C.c_int32)), BANDS.ctypes.data_as(C.POINTER(C.c_double))
    for run in (lib.af_lane_eq_run_host, lib.af_lane_eq_run_device):
        pointer = fp if run is lib.af_lane_eq_run_host else C.c_void_p(audio.ctypes.data)
        for args, text in (((None, 100, 2, 100, ip, 3, dp), "null"), ((pointer, 100, 2, 100, None, 3, dp), "null"),
                           ((pointer, 100, 2, 100, ip, 3, None), "null"), ((pointer, 100, 2, 100, ip, 0, dp), "n_lanes"),
                           ((pointer, 100, 2, 100, ip, -4, dp), "n_lanes"), ((pointer, 100, 2, 99, ip, 3, dp), "stride"),
                           ((pointer, 0, 2, 100, ip, 3, dp), "n_samples"), ((pointer, 100, 0, 100, ip, 3, dp), "n_captures"),
                           ((pointer, 100, 1, 100, ip, 3, dp), "names capture")):
            with pytest.raises(ValueError, match=text):
                _lib.check(run(eq._h, *args))
    with pytest.raises(ValueError, match="names capture"):
        eq.run(audio, [0, -1, 1], BANDS)
    bad = BANDS.copy()
    bad[2, 4, 1] = np.nan
    with pytest.raises(ValueError, match="finite"):
        eq.run(audio, lanes, bad)
    with pytest.raises(ValueError, match="expected bands"):
        eq.run(audio, lanes, BANDS[:2])
    with pytest.raises(RuntimeError, match="no run"):
        eq.device_output()
    with pytest.raises(RuntimeError, match="no run"):
        eq.output()
    assert eq.last_kernel_ms() == 0.0
    eq.close()
    eq.close()


def test_settings_helpers_follow_the_reference(mi):
    from mic_eq_mi import headroom as H

    assert H.HEADROOM_SCALES == HS.SCALES
    flat = H._flatten_chain_settings(None)
    assert flat == {"return_output_audio": False, "deesser_enabled": False, "deesser_auto_enabled": True, "deesser_auto_amount": 0.5,
                    "deesser_low_cut_hz": 4000.0, "deesser_high_cut_hz": 11000.0, "deesser_threshold_db": -28.0, "deesser_ratio": 4.0,
                    "deesser_attack_ms": 2.0, "deesser_release_ms": 80.0, "deesser_max_reduction_db": 6.0, "compressor_enabled": True,
                    "compressor_threshold_db": -20.0, "compressor_ratio": 4.0, "compressor_attack_ms": 10.0, "compressor_release_ms": 200.0,
                    "compressor_makeup_gain_db": 0.0, "compressor_adaptive_release": False, "compressor_base_release_ms": 50.0,
                    "compressor_auto_makeup_enabled": False, "compressor_target_lufs": -18.0,
                    "compressor_sidechain_highpass_enabled": True, "limiter_enabled": True, "limiter_ceiling_db": -0.5,
                    "limiter_release_ms": 50.0, "limiter_careful_output_enabled": True}
    assert list(flat) == list(H._flatten_chain_settings({}))
    flat = H._flatten_chain_settings({"deesser": {"enabled": 1, "ratio": "6"}, "compressor": {"ratio": float("nan"), "enabled": False},
                                      "limiter": {"ceiling_db": None}})
    assert flat["deesser_enabled"] is False and flat["deesser_ratio"] == 6.0  # only a bool is a bool; float() parses text
    assert flat["compressor_ratio"] == 4.0 and flat["compressor_enabled"] is False and flat["limiter_ceiling_db"] == -0.5
    assert H._bands_from_settings({"band_freqs": HS.FREQS, "band_gains": [None] * 10, "band_qs": ["x"] * 10}) == [(f, 0.0, 1.41) for f in HS.FREQS]
    safe = {"pre_limiter_true_peak_headroom_db": 1.0, "limiter_gain_reduction_db": 1.0, "true_peak_limiter_gain_reduction_db": 0.5}
    assert H._is_headroom_safe(safe) and H._is_headroom_safe({}) and H._is_headroom_safe({"true_peak_headroom_db": 1.0})
    for key, value in (("pre_limiter_true_peak_headroom_db", 0.999), ("limiter_gain_reduction_db", 1.001),
                       ("true_peak_limiter_gain_reduction_db", 0.501)):
        assert not H._is_headroom_safe(dict(safe, **{key: value}))
    assert not H._is_headroom_safe({"true_peak_headroom_db": 0.5})


def test_operators_check_their_arguments_before_any_gpu_work(mi):
    audio = HS.captures()[:2]
    eq = HS.eq_settings(1)
    for key in ("band_freqs", "band_gains", "band_qs"):
        with pytest.raises(ValueError, match="Auto-EQ settings must contain 10 frequencies, gains, and Q values"):
            mi.simulate_candidate_chain_batch(audio, HS.FS, dict(eq, **{key: eq[key][:9]}))
    with pytest.raises(ValueError, match="Auto-EQ settings must contain 10"):
        mi.apply_headroom_validation_batch(audio, HS.FS, dict(eq, band_qs=[]))
    with pytest.raises(ValueError, match="one eq_settings per stream"):
        mi.simulate_candidate_chain_batch(audio, HS.FS, [eq] * 3)
    with pytest.raises(ValueError, match="route"):
        mi.simulate_candidate_chain_batch(audio, HS.FS, eq, route="fast")
    with pytest.raises(ValueError, match="route 'sweep'"):
        mi.simulate_candidate_chain_batch(audio, HS.FS, eq, {"compressor": {"enabled": False}}, route="sweep")
    with pytest.raises(ValueError, match="sample_rate"):
        mi.simulate_candidate_chain_batch(audio, 0.0, eq)


def test_wrong_length_band_gains_returns_the_copy_untouched(mi):
    audio = HS.captures()[:2]
    given = [dict(HS.eq_settings(0), band_gains=[1.0] * 9, nested={"a": [1]}), dict(HS.eq_settings(1), band_gains=[])]
    got = mi.apply_headroom_validation_batch(audio, HS.FS, given)
    assert got == given and got[0] is not given[0] and got[0]["nested"]["a"] is not given[0]["nested"]["a"]
    one = mi.apply_headroom_validation(audio[0], HS.FS, given[0])
    assert one == given[0] and "headroom_validation" not in one
