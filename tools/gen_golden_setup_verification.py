#!/usr/bin/env python3
"""Build-container-only: generate tests/golden/setup_verification.npz by IMPORTING the reference's own get_target_curve
(python/mic_eq/analysis/auto_eq_parts/target.py:65-104), _shape_error_db and _rms_db (python/mic_eq/analysis/voice_setup.py
:1446-1465, :102-106) and running them on the closed-form spectra and signals of tests/setup_verification_stimulus.py.

What is written is data, never reference text: per (nperseg, spectrum, preset) the shape error; for nperseg 64, and for the clip-driving spectra
at nperseg 2048, also the adaptive target curve over the masked bins; per signal length the level; and what
validate_voice_setup_verification itself decides on the hand-made cases of tests/setup_verification_rules_stimulus.py (see
rules()).  The generator asserts what the tests rely on: the masked
bin counts (even, odd, below 8), that every clip a spectrum can drive is driven to both ends, and the unknown-preset error.

    python tools/gen_golden_setup_verification.py      (needs the reference checkout; AF_REFERENCE overrides its place)
"""
from __future__ import annotations

import hashlib
import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
REFERENCE = pathlib.Path(os.environ.get("AF_REFERENCE", "/root/reference"))


def main() -> None:
    if not (REFERENCE / "python" / "mic_eq").is_dir():
        raise SystemExit("tools/gen_golden_setup_verification.py runs in the build container only (the reference is not here)")
    sys.path.insert(0, str(REFERENCE / "python"))
    sys.path.insert(0, str(ROOT / "tests"))
    from mic_eq.analysis import voice_setup as V
    from mic_eq.analysis.auto_eq_parts import target as T

    import setup_verification_stimulus as SV

    out: dict = {}
    errors = np.zeros((len(SV.NPERSEGS), len(SV.SPECTRA), len(SV.PRESETS)))
    digests = np.zeros((len(SV.NPERSEGS), len(SV.SPECTRA), 32), dtype=np.uint8)
    for g, nperseg in enumerate(SV.NPERSEGS):
        f = SV.grid(nperseg)
        mask = (f >= 80.0) & (f <= 12_000.0)
        assert int(np.count_nonzero(mask)) == SV.MASKED_BINS[nperseg], (nperseg, int(np.count_nonzero(mask)))
        for i, name in enumerate(SV.SPECTRA):
            db = SV.spectrum(name, nperseg)
            digests[g, i] = np.frombuffer(hashlib.sha256(db.tobytes()).digest(), dtype=np.uint8)
            for j, preset in enumerate(SV.PRESETS):
                error = V._shape_error_db(f, db, preset)
                errors[g, i, j] = error
                assert np.isinf(error) == (SV.MASKED_BINS[nperseg] < 8)
                if nperseg == 64 or (nperseg == 2048 and (name == "voice" or name in SV.CLIP_CASES)):
                    out[f"curve/{nperseg}/{name}/{preset}"] = np.asarray(T.get_target_curve(f[mask], preset, db[mask], target_mode="adaptive"))
            if nperseg == 2048:  # the clips: what _adaptive_voice_offsets derives, recomputed from its own helper for the assertion only
                body, presence = T._band_mean(f[mask], db[mask], 180.0, 800.0), T._band_mean(f[mask], db[mask], 1200.0, 3500.0)
                sibilance = T._band_mean(f[mask], db[mask], 5500.0, 8500.0)
                voice = mask & (f >= 100.0) & (f <= 8000.0)
                slope = float(np.polyfit(np.log10(f[voice]), db[voice], 1)[0])  # dB per decade
                seen = {"low_mid_balance": (body - presence) / 8.0, "sibilance": (sibilance - presence) / 7.0,
                        "tilt": slope * np.log10(2.0) / 4.0}
                if name in SV.CLIP_CASES:
                    which, sign = SV.CLIP_CASES[name]
                    assert sign * seen[which] > 1.0, (name, seen)
    out["errors"], out["sha256"] = errors, digests  # [nperseg][spectrum][preset], [nperseg][spectrum][32]
    for preset in SV.PRESETS:  # the catalog curve alone ("static")
        out[f"static/{preset}"] = np.asarray(T.get_target_curve(SV.grid(64), preset, None, target_mode="static"))
    try:
        T.get_target_curve(SV.grid(64), "warm")
        raise AssertionError("an unknown preset must raise")
    except ValueError as error:
        out["unknown_preset_message"] = np.array(str(error))
    for n in SV.LENGTHS:
        out[f"rms_db/{n}"] = np.float64(V._rms_db(SV.signal(n, n % 7)))
    out["rms_db/0"] = np.float64(V._rms_db(np.zeros(0, dtype=np.float32)))
    rules(V, out)
    runs(V, out)
    offline(V, out)
    target = ROOT / "tests" / "golden" / "setup_verification.npz"
    np.savez_compressed(target, **out)
    print(f"wrote {target} ({target.stat().st_size} bytes, {len(out)} entries)")


def rules(V, out: dict) -> None:
    """validate_voice_setup_verification itself on the hand-made cases of tests/setup_verification_rules_stimulus.py: its measuring
    helpers (the renderer, the spectrum analysis, _shape_error_db, the speech features, _rms_db) answer from the case's numbers,
    so what is recorded is what the reference's own rules make of them."""
    import types

    import setup_verification_rules_stimulus as RS

    real = {name: getattr(V, name) for name in ("simulate_candidate_chain", "analyze_voice_spectrum", "_shape_error_db",
                                                 "_vad_masked_speech_features", "_rms_db")}
    freqs = np.fft.rfftfreq(64, 1.0 / RS.FS)
    mask = (freqs >= 80.0) & (freqs <= 12_000.0)
    seen = set()
    decisions, reasons, keys = [], [], []
    numbers, flags = np.full((len(RS.CASES), len(RS.NUMBER_KEYS)), np.nan), np.full((len(RS.CASES), 2), -1, dtype=np.int64)
    for index, (name, overrides, expected) in enumerate(RS.CASES):
        c = RS.case(overrides)
        verification = np.full(c["samples"], 0.01, dtype=np.float32)
        verification[0] = c["peak"]
        if c["non_finite"]:
            verification[-1] = np.nan
        noise, original = np.zeros(1000, dtype=np.float32), np.zeros(150_007, dtype=np.float32)
        rendered, rendered_noise = np.full(c["samples"] + 1, 0.01, dtype=np.float32), np.zeros(1001, dtype=np.float32)
        rendered[3] = c["rendered_peak"]
        tags = {noise.size: "noise", original.size: "original", verification.size: "verification", rendered.size: "rendered",
                rendered_noise.size: "rendered_noise"}
        assert len(tags) == 5
        renders = iter([rendered, rendered_noise])
        delta = np.zeros(freqs.size)
        delta[mask] = c["shape_delta"] * np.where(np.arange(int(mask.sum())) % 2 == 0, 1.0, -1.0)  # median 0, RMS shape_delta
        spectra = iter([types.SimpleNamespace(freqs=freqs, median_spectrum_db=np.zeros(freqs.size), snr_db=0.0, spectral_snr_db=None),
                        types.SimpleNamespace(freqs=freqs, median_spectrum_db=delta, snr_db=c["snr_before"], spectral_snr_db=None),
                        types.SimpleNamespace(freqs=freqs, median_spectrum_db=np.zeros(freqs.size), snr_db=c["snr_after"],
                                              spectral_snr_db=None)])
        errors = iter([c["error_before"], c["error_after"]])
        spreads = iter([c["spread_before"], c["spread_after"]])

        def simulate(audio, sample_rate, eq_settings, chain_settings=None):
            result = dict(c["sim"])
            result["simulation_backend"] = c["backend"]
            result["output_audio"] = next(renders)
            return result

        V.simulate_candidate_chain = simulate
        V.analyze_voice_spectrum = lambda *a, **k: next(spectra)
        V._shape_error_db = lambda *a, **k: next(errors)
        V._vad_masked_speech_features = lambda *a, **k: {"active_loudness_spread_db": next(spreads)}
        V._rms_db = lambda audio: c["rms"][tags[np.asarray(audio).size]]
        try:
            result = V.validate_voice_setup_verification(noise, original, verification, RS.FS, {
                "deesser_settings": dict(c["deesser"]), "compressor_settings": dict(c["compressor"])}, "broadcast")
        finally:
            for key, fn in real.items():
                setattr(V, key, fn)
        assert result["decision"] == expected, (name, result["decision"], expected)
        assert len(result["reasons"]) == 1 and result["perceptual_validation"] is False
        decisions.append(result["decision"])
        reasons.append(result["reasons"][0])
        keys.append("|".join(sorted(result)))
        seen.add((result["decision"], result["reasons"][0]))
        if set(result) - RS.EARLY_KEYS - {"simulation_backend"}:
            numbers[index] = [result[key] for key in RS.NUMBER_KEYS]
            flags[index] = [result["limiter_activity_events"], int(result["clipped"])]
            assert result["frequency_dependent_snr_db"] == {} and result["simulation_backend"] == "rust"
            assert result["evidence_scope"] == "repeatability_and_exact_native_chain_constraints"
    out["rules/names"] = np.array([name for name, _, _ in RS.CASES])
    out["rules/decisions"], out["rules/reasons"], out["rules/keys"] = np.array(decisions), np.array(reasons), np.array(keys)
    out["rules/numbers"], out["rules/flags"] = numbers, flags  # NaN / -1 rows: an early exit has no numbers
    assert {d for d, _ in seen} == {"accept", "reduce", "rollback", "retry"} and len(seen) == 7, seen


RUN_NUMBERS = ("spectral_target_error_before_db", "spectral_target_error_after_db", "loudness_variation_before_db",
               "loudness_variation_after_db", "noise_floor_change_db", "relative_noise_floor_change_db", "snr_change_db",
               "compressor_gain_reduction_median_db", "compressor_gain_reduction_p95_db", "compressor_gain_reduction_peak_db",
               "deesser_gain_reduction_median_db", "deesser_gain_reduction_p95_db", "output_true_peak_db")
RUN_BANDS = ("low", "body", "presence", "sibilance")


def runs(V, out: dict) -> None:
    """validate_voice_setup_verification itself on the whole captures of setup_verification_stimulus.run_batch(): its
    simulate_candidate_chain is answered by this repository's CPU oracle behind the reference's own _flatten_chain_settings and
    _bands_from_settings, marked "rust" as the native binding's result is; everything else is the reference's own code."""
    sys.path.insert(0, str(ROOT / "oracle"))
    from mic_eq.analysis.auto_eq_parts import headroom as H

    import af_oracle_py as oracle
    import setup_verification_stimulus as SV

    def simulate(audio, sample_rate, eq_settings, chain_settings=None):
        flat = H._flatten_chain_settings(chain_settings)
        result = dict(oracle.simulate_auto_eq_chain(np.ascontiguousarray(audio, dtype=np.float32), float(sample_rate),
                                                    H._bands_from_settings(eq_settings), flat))
        result["simulation_backend"] = "rust"
        sims.append(result)
        return result

    sims: list = []
    real = V.simulate_candidate_chain
    V.simulate_candidate_chain = simulate
    try:
        b = SV.run_batch()
        decisions, reasons, keys = [], [], []
        numbers = np.full((len(SV.RUN_CASES), len(RUN_NUMBERS)), np.nan)
        bands = np.full((len(SV.RUN_CASES), 4), np.nan)
        flags = np.full((len(SV.RUN_CASES), 2), -1, dtype=np.int64)
        margins = np.full(len(SV.RUN_CASES), np.nan)
        for k, (name, *_rest) in enumerate(SV.RUN_CASES):
            sims.clear()
            r = V.validate_voice_setup_verification(b["noise"][k], b["original"][k], b["verification"][k], SV.FS, b["setups"][k], b["presets"][k])
            decisions.append(r["decision"])
            reasons.append(r["reasons"][0])
            keys.append("|".join(sorted(r)))
            if "snr_change_db" in r:
                numbers[k] = [r[key] for key in RUN_NUMBERS]
                bands[k] = [r["frequency_dependent_snr_db"].get(name_, np.nan) for name_ in RUN_BANDS]
                flags[k] = [r["limiter_activity_events"], int(r["clipped"])]
                # the smallest distance of a compared quantity from its threshold (:1608-1627), from the returned numbers, the
                # verification render's own ceiling and the two levels; the repeatability delta is not returned: the GPU test
                # checks its own distance from 5 dB
                compressor, deesser = b["setups"][k].get("compressor_settings") or {}, b["setups"][k].get("deesser_settings") or {}
                ceiling = float(sims[0].get("limiter_effective_ceiling_db", -1.5))
                level = abs(V._rms_db(b["verification"][k]) - V._rms_db(b["original"][k]))
                margins[k] = min(
                    abs(level - 8.0), abs(r["spectral_target_error_after_db"] - r["spectral_target_error_before_db"] - 1.0),
                    abs(r["relative_noise_floor_change_db"] - 4.0), abs(r["relative_noise_floor_change_db"] - 3.0),
                    abs(r["snr_change_db"] + 4.0),
                    abs(r["compressor_gain_reduction_peak_db"] - float(compressor.get("peak_reduction_cap_db", 8.0)) - 0.25),
                    abs(r["output_true_peak_db"] - ceiling - 0.15),
                    abs(r["compressor_gain_reduction_p95_db"] - float(compressor.get("target_p95_reduction_db", 3.5)) - 0.75),
                    abs(r["deesser_gain_reduction_p95_db"] - float(deesser.get("max_reduction_db", 6.0)) * 0.9))
            print(f"  {name}: {r['decision']} ({r['reasons'][0]})")
        short = V.validate_voice_setup_verification(b["noise"][0], b["original"][0], b["verification"][0][:SV.SHORT_SAMPLES], SV.FS,
                                                    b["setups"][0], "broadcast")
    finally:
        V.simulate_candidate_chain = real
    assert short == {"decision": "retry", "reasons": ["verification passage was too short"], "perceptual_validation": False}
    count = {d: decisions.count(d) for d in ("accept", "reduce", "rollback", "retry")}
    assert all(n >= 2 for n in count.values()), count  # all four decisions, at least two streams each
    assert {"verification delivery differs too much from the setup passage", "verification passage was non-finite or clipped"} <= set(reasons)
    by_name = dict(zip([c[0] for c in SV.RUN_CASES], decisions))
    assert by_name["treble_boost"] == "rollback" and by_name["hard_compressor_0"] == "rollback"  # through the caller's EQ, and the compressor
    for key in ("noise", "original", "verification"):
        out[f"runs/sha256/{key}"] = np.frombuffer(hashlib.sha256(b[key].tobytes()).digest(), dtype=np.uint8)
    out["runs/names"] = np.array([c[0] for c in SV.RUN_CASES])
    out["runs/decisions"], out["runs/reasons"], out["runs/keys"] = np.array(decisions), np.array(reasons), np.array(keys)
    out["runs/numbers"], out["runs/bands"], out["runs/flags"], out["runs/margins"] = numbers, bands, flags, margins
    print(f"  smallest threshold margin {np.nanmin(margins):.3e} dB ({SV.RUN_CASES[int(np.nanargmin(margins))][0]})")


OFFLINE_NUMBERS = ("setup_confidence", "recommendation_uncertainty", "capture_confidence", "eq_confidence", "gate_confidence",
                   "deesser_confidence", "compressor_confidence")
OFFLINE_FLAGS = ("weak_capture", "apply_recommended", "offline_validation_passed")


def offline(V, out: dict) -> None:
    """analyze_voice_setup itself on the six chain pairs under the two argument sets of the chain fixture, without EQ settings
    (its Auto-EQ call raises, as in tools/gen_golden_speech_features.py) and with the caller's EQ of the stimulus in its place (the
    calibration search behind it, which has a fixture of its own, hands the settings back unchanged); its native VAD helper is
    answered with the stimulus' posteriors and its simulate_candidate_chain by the CPU oracle, marked "rust"."""
    from mic_eq.analysis.auto_eq_parts import headroom as H

    import af_oracle_py as oracle
    import setup_verification_stimulus as SV
    import speech_features_stimulus as SS

    c = SS.chain_batch()
    current = {}

    def stimulus_vad(audio, sample_rate, **_):
        return (current["vad"] if np.asarray(audio).size == c["speech"].shape[1] else current["noise_vad"]).copy(), "stimulus"

    def auto_eq(*_, **__):
        if current["eq"] is None:
            raise RuntimeError("Auto-EQ is not part of this fixture")
        return dict(current["eq"]), None

    def simulate(audio, sample_rate, eq_settings, chain_settings=None):
        result = dict(oracle.simulate_auto_eq_chain(np.ascontiguousarray(audio, dtype=np.float32), float(sample_rate),
                                                    H._bands_from_settings(eq_settings), H._flatten_chain_settings(chain_settings)))
        result["simulation_backend"] = "python" if current["mode"] == "advisory" else "rust"
        return result

    def no_calibration(*, compressor_settings, **_):
        return compressor_settings, {"backend": "unavailable", "target_gain_reduction_db": 0.0, "measured_gain_reduction_db": 0.0, "iterations": 0}

    real = {name: getattr(V, name) for name in ("analyze_offline_vad", "analyze_auto_eq", "simulate_candidate_chain", "_calibrate_compressor_threshold")}
    V.analyze_offline_vad, V.analyze_auto_eq, V.simulate_candidate_chain = stimulus_vad, auto_eq, simulate
    V._calibrate_compressor_threshold = no_calibration
    seen, roundtrip = set(), []
    try:
        for a, arguments in enumerate(SS.CHAIN_ARGUMENTS):
            for mode in ("flat", "eq", "advisory"):  # advisory: the flat run with a renderer that is not the native one (:1342-1344)
                numbers, flags, reasons, validation, inputs = [], [], [], [], []
                for i in range(c["speech"].shape[0]):
                    current.update(vad=c["vad"][i], noise_vad=c["noise_vad"][i], eq=SV.offline_eq(i) if mode == "eq" else None, mode=mode)
                    r = V.analyze_voice_setup(c["noise"][i], c["speech"][i], SS.FS, arguments["target_preset"],
                                              dynamics_intensity=arguments["dynamics_intensity"],
                                              custom_target_p95_db=arguments["custom_target_p95_db"],
                                              custom_peak_cap_db=arguments["custom_peak_cap_db"])
                    d = r["diagnostics"]
                    # what the rules of :1265-1364 read, for the restatement's CPU test
                    inputs.append([d["capture_confidence"], d["speech_dynamic_range_db"], d["conservative_noise_rms_db"],
                                   d["noise_referenced_snr_db"], d["vad_active_duration_s"], d["deesser_frame_evidence_confidence"],
                                   float(d["deesser_enabled"]), float(d["noise_reference_quality"]["status"] == "usable"),
                                   r["compressor_settings"]["peak_reduction_cap_db"], r["compressor_settings"]["target_p95_reduction_db"],
                                   float(d["offline_validation"]["limiter_effective_ceiling_db"]),
                                   float(len(d["noise_reference_quality"]["reasons"]))])
                    numbers.append([d[key] for key in OFFLINE_NUMBERS])
                    flags.append([int(d[key]) for key in OFFLINE_FLAGS])
                    reasons.append("|".join(d["uncertainty_reasons"]))
                    v = d["offline_validation"]
                    validation.append([v["output_true_peak_db"], v["compressor_gain_reduction_db"], v["compressor_gain_reduction_p95_db"],
                                       v["deesser_gain_reduction_db"]])
                    if a == 0 and mode == "flat":  # recommend -> verify: the reference's own result on a second passage (played backwards)
                        second = np.ascontiguousarray(c["speech"][i][::-1])
                        roundtrip.append(V.validate_voice_setup_verification(c["noise"][i], c["speech"][i], second, SS.FS, r,
                                                                             arguments["target_preset"])["decision"])
                    seen.update({("passed", d["offline_validation_passed"]), ("weak", d["weak_capture"]), ("apply", d["apply_recommended"])})
                out[f"offline/{a}/{mode}/numbers"] = np.array(numbers, dtype=np.float64)
                out[f"offline/{a}/{mode}/flags"] = np.array(flags, dtype=np.int32)
                out[f"offline/{a}/{mode}/reasons"] = np.array(reasons)
                out[f"offline/{a}/{mode}/validation"] = np.array(validation, dtype=np.float64)
                out[f"offline/{a}/{mode}/inputs"] = np.array(inputs, dtype=np.float64)
    finally:
        for key, fn in real.items():
            setattr(V, key, fn)
    out["offline/roundtrip_decisions"] = np.array(roundtrip)
    assert "accept" in roundtrip, roundtrip
    print("  offline classes", sorted(map(str, seen)), "round trip", roundtrip)
    assert {("passed", True), ("passed", False)} <= seen, seen  # both offline_validation_passed values


if __name__ == "__main__":
    main()
