#!/usr/bin/env python3
"""Build-container-only: generate tests/golden/speech_features.npz by IMPORTING the reference's own
python/mic_eq/analysis/voice_setup.py and running _vad_masked_speech_features over the stimuli of
tests/speech_features_stimulus.py.

What is written is data, never reference text: fingerprints of the stimuli, and per stream what the reference returned --
every scalar of its dict and of its de-esser evidence, the counts, and for a few streams of the main batch the per-frame
arrays (frame levels, the active mask, the indices, probabilities and feature rows of the spectrally active frames).

It asserts the conditions the parity tests rest on: every class of the stimulus is present (a loudness fallback, a short-term
fallback, posteriors used and not used, the energy mask kept below six posterior frames, the percentile-10 noise fallback, no
active frame, evidence available and not); no decision quantity lies within 1e-6 of its cut (the adaptive floor and the
supported-energy floor against every frame level, the 0.40 / 0.65 posterior cuts, the 0.55 window activity, the six-frame
rule is an integer); every arg-max has a runner-up at least 1e-9 relative below it; every compared band sum lies a factor 1e6
above the transform's rounding floor N eps^2 sum |x w|^2 unless its frame is exactly zero; for the recommendation rules
(:1143-1223 with the reference's _recommend_* functions, on the made-up spectrum inputs of the stimulus, main batch) the de-esser
is enabled on some streams and not on others, all three dynamics profiles and "custom" occur with auto-makeup on and off, and
the 6 dB, 0.55, 10 dB and enable-threshold cuts are at least 1e-6 away, and the 2 s cut compares a whole number of hops; for six
whole capture pairs (chain/...) the reference's analyze_voice_setup itself, fed the stimulus' posteriors in place of its native
VAD helper and run without the Auto-EQ optimiser, with the same cuts clear and the de-esser and auto-makeup both on and off; and the file is no larger than the
largest fixture already there.  Re-run:
    python tools/gen_golden_speech_features.py      (needs the reference checkout; AF_REFERENCE overrides its place)
"""
from __future__ import annotations

import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
REFERENCE = pathlib.Path(os.environ.get("AF_REFERENCE", "/root/reference"))
OUT = ROOT / "tests" / "golden" / "speech_features.npz"
FRAME_STREAMS = (0, 1, 2, 64, 66)  # streams of the main batch whose per-frame arrays are kept
SCALARS = ("active_duration_s", "active_ratio", "vad_active_frame_ratio", "short_term_lufs", "momentary_lufs",
           "active_loudness_spread_db", "loudness_range_db", "sibilance_excess_db")
BANDS = ("low", "body", "presence", "sibilance")
EVIDENCE = ("confidence", "frame_probability_p90", "frame_probability_top_mean", "temporal_score", "absolute_hf_strength_p90",
            "noise_reliability_p90", "excess_p90_db", "temporal_contrast_db", "candidate_frame_ratio", "candidate_snr_db", "peak_hz")
# af_voice_setup_recommendation's fields as the reference's rules give them for the main batch (main/setup_numbers, _flags)
SETUP_NUMBERS = ("speech_floor_db", "speech_body_db", "speech_frame_peak_db", "speech_snr_db", "snr_confidence", "capture_confidence",
                 "gate_threshold_db", "gate_vad_threshold", "gate_vad_hold_time_ms", "gate_vad_pre_gain", "gate_margin_db",
                 "deesser_auto_amount", "deesser_low_cut_hz", "deesser_high_cut_hz", "deesser_ratio", "deesser_max_reduction_db",
                 "deesser_sibilance_excess_db", "deesser_peak_hz", "deesser_frame_evidence_confidence", "deesser_detection_probability",
                 "compressor_threshold_db", "compressor_ratio", "compressor_attack_ms", "compressor_release_ms", "compressor_makeup_gain_db",
                 "compressor_base_release_ms", "compressor_target_lufs", "compressor_target_p95_db", "compressor_target_median_db",
                 "compressor_peak_cap_db", "compressor_noise_reference_reliability")
SETUP_FLAGS = ("gate_mode", "gate_auto_threshold_enabled", "deesser_enabled", "deesser_frame_evidence_available", "deesser_invalid_evidence",
               "compressor_auto_makeup_enabled", "compressor_profile")
PROFILES = ("gentle", "balanced", "dense", "custom")
# what the reference's analyze_voice_setup itself returns for the whole capture pairs of the stimulus (chain/numbers, chain/flags):
# (name, where it is in the returned dict)
CHAIN_NUMBERS = (("capture_confidence", "diagnostics"), ("speech_floor_db", "diagnostics"), ("speech_body_db", "diagnostics"),
                 ("speech_snr_db", "diagnostics"), ("conservative_noise_rms_db", "diagnostics"), ("noise_referenced_snr_db", "diagnostics"),
                 ("short_term_lufs", "diagnostics"), ("loudness_range_db", "diagnostics"), ("sibilance_excess_db", "diagnostics"),
                 ("sibilance_peak_hz", "diagnostics"), ("deesser_detection_probability", "diagnostics"),
                 ("deesser_frame_evidence_confidence", "diagnostics"),
                 ("threshold_db", "gate_settings"), ("vad_threshold", "gate_settings"), ("vad_hold_time_ms", "gate_settings"),
                 ("vad_pre_gain", "gate_settings"), ("gate_margin_db", "gate_settings"),
                 ("auto_amount", "deesser_settings"), ("low_cut_hz", "deesser_settings"), ("high_cut_hz", "deesser_settings"),
                 ("ratio", "deesser_settings"), ("max_reduction_db", "deesser_settings"),
                 ("threshold_db", "compressor_settings"), ("ratio", "compressor_settings"), ("attack_ms", "compressor_settings"),
                 ("release_ms", "compressor_settings"), ("makeup_gain_db", "compressor_settings"), ("base_release_ms", "compressor_settings"),
                 ("target_lufs", "compressor_settings"), ("target_p95_reduction_db", "compressor_settings"),
                 ("peak_reduction_cap_db", "compressor_settings"), ("noise_reference_reliability", "compressor_settings"))
CHAIN_FLAGS = (("gate_mode", "gate_settings"), ("auto_threshold_enabled", "gate_settings"), ("enabled", "deesser_settings"),
               ("auto_makeup_enabled", "compressor_settings"))


def chain_fixture(V, SS, data) -> None:
    """analyze_voice_setup on the whole capture pairs, with the stimulus' posteriors where it would ask its native VAD helper and
    without the Auto-EQ optimiser (so without the calibration search behind it): the rules' inputs are then the reference's own
    noise reference, voice spectrum and features of each pair."""
    c = SS.chain_batch()
    current = {}

    def stimulus_vad(audio, sample_rate, **_):
        return (current["vad"] if np.asarray(audio).size == c["speech"].shape[1] else current["noise_vad"]).copy(), "stimulus"

    def no_auto_eq(*_, **__):
        raise RuntimeError("Auto-EQ is not part of this fixture")

    V.analyze_offline_vad, V.analyze_auto_eq = stimulus_vad, no_auto_eq
    nearest, seen = np.inf, set()
    for a, arguments in enumerate(SS.CHAIN_ARGUMENTS):
        numbers, flags, profiles, statuses = [], [], [], []
        for i in range(c["speech"].shape[0]):
            current.update(vad=c["vad"][i], noise_vad=c["noise_vad"][i])
            r = V.analyze_voice_setup(c["noise"][i], c["speech"][i], SS.FS, arguments["target_preset"],
                                      dynamics_intensity=arguments["dynamics_intensity"],
                                      custom_target_p95_db=arguments["custom_target_p95_db"],
                                      custom_peak_cap_db=arguments["custom_peak_cap_db"])
            d = r["diagnostics"]
            assert r["eq_settings"] is None and d["vad_analysis_backend"] == "stimulus" and d["vad_probability_used"]
            numbers.append([r[where][key] for key, where in CHAIN_NUMBERS])
            flags.append([int(r[where][key]) for key, where in CHAIN_FLAGS])
            profiles.append(PROFILES.index(r["compressor_settings"]["dynamics_intensity"]))
            statuses.append(d["noise_reference_quality"]["status"])
            nearest = min(nearest, abs(d["noise_referenced_snr_db"] - 6.0), abs(d["capture_confidence"] - 0.55), abs(d["speech_snr_db"] - 10.0),
                          abs(d["deesser_detection_probability"] - d["deesser_enable_probability_threshold"]))
            seen.update({("deesser", r["deesser_settings"]["enabled"]), ("makeup", r["compressor_settings"]["auto_makeup_enabled"])})
        data[f"chain/{a}/numbers"] = np.array(numbers, dtype=np.float64)
        data[f"chain/{a}/flags"] = np.array(flags, dtype=np.int32)
        data[f"chain/{a}/profiles"] = np.array(profiles, dtype=np.int32)
        data[f"chain/{a}/status"] = np.array(statuses)
    for key in ("speech", "vad", "noise", "noise_vad"):
        data[f"chain/{key}_sha256"] = np.array(SS.fingerprint(c[key])["sha256"])
    data["chain/nearest_decision"] = np.array(nearest)
    print(f"chain: nearest decision {nearest:.3e}, classes {sorted(map(str, seen))}")
    assert seen == {("deesser", True), ("deesser", False), ("makeup", True), ("makeup", False)}, seen
    assert nearest > SS.MARGIN, nearest
COUNTS = ("frames", "active_frames", "spectral_frames", "vad_probability_used", "short_term_window_count", "loudness_window_count",
          "evidence_available")


def main() -> None:
    if not (REFERENCE / "python" / "mic_eq" / "analysis" / "voice_setup.py").exists():
        raise SystemExit("tools/gen_golden_speech_features.py runs in the build container only (the reference is not here)")
    sys.path.insert(0, str(REFERENCE / "python"))
    sys.path.insert(0, str(ROOT / "tests"))
    from mic_eq.analysis import voice_setup as V
    from mic_eq.analysis.spectrum import _interpolate_vad_probabilities

    import speech_features_stimulus as SS

    eps = np.finfo(np.float64).eps
    window = np.hanning(SS.FRAME)
    freqs = np.fft.rfftfreq(SS.FRAME, 1.0 / SS.FS)
    band_masks = [(freqs >= lo) & (freqs <= hi) for lo, hi in ((80, 250), (250, 2000), (2000, 5000), (5000, 10000), (250, 4500), (5000, 9500))]
    sib = band_masks[5]
    data: dict[str, np.ndarray] = {}
    nearest, runner_up, floor_ratio = np.inf, np.inf, np.inf
    classes = dict.fromkeys(("masked-mean fallback", "short-term fallback", "two short-term windows", "posteriors used", "no posteriors",
                             "energy mask kept", "posterior mask taken", "percentile-10 noise level", "noise frames", "no active frame",
                             "evidence available", "evidence unavailable", "non-finite", "partial tail chunk", "frame below the spectral list",
                             "sibilant frames outside the posterior mask"), 0)
    setup_numbers, setup_flags, setup_clip, setup_nearest, setup_classes = [], [], [], np.inf, set()
    for b in SS.batches():
        name, B, n = b["name"], b["speech"].shape[0], b["speech"].shape[1]
        counts = np.zeros((B, len(COUNTS)), dtype=np.int64)
        scalars = np.full((B, len(SCALARS) + len(BANDS) + len(EVIDENCE)), np.nan)
        for s in range(B):
            x = b["speech"][s].astype(np.float64)
            vad = None if b["vad"] is None else b["vad"][s]
            z = None if b["noise"] is None else b["noise"][s].astype(np.float64)
            level = float(b["noise_rms_db"][s])
            if not np.all(np.isfinite(x)):
                counts[s] = -1
                classes["non-finite"] += 1
                continue
            r = V._vad_masked_speech_features(x, SS.FS, level, vad, z)
            ev = r["deesser_frame_evidence"]
            mask = np.asarray(r["active_frame_mask"], dtype=bool)
            F, A = r["frame_db"].size, ev["frame_indices"].size
            counts[s] = (F, np.count_nonzero(mask), A, r["vad_probability_used"], r["short_term_window_count"], r["loudness_window_count"],
                         ev["available"])
            scalars[s] = ([r[k] for k in SCALARS] + [r["band_energy_db"][k] for k in BANDS]
                          + [ev.get(k, np.nan) if ev["available"] or k in ("confidence", "excess_p90_db", "temporal_contrast_db",
                                                                          "candidate_frame_ratio", "candidate_snr_db", "peak_hz") else np.nan
                             for k in EVIDENCE])

            # ---- how close the decisions are
            db = r["frame_db"]
            floor = max(level + 6.0, float(np.percentile(db, 30.0)) + 2.0)
            energy_active = db >= floor
            nearest = min(nearest, float(np.min(np.abs(db - floor))))  # (the floor is a maximum: which side wins decides nothing)
            raw = energy_active
            if vad is not None:
                p = _interpolate_vad_probabilities(vad, np.arange(F) * SS.HOP, SS.FRAME, SS.FS)
                low = max(level + 2.0, floor - 4.0)
                nearest = min(nearest, float(np.min(np.abs(p - 0.40))), float(np.min(np.abs(p - 0.65))), float(np.min(np.abs(db - low))))
                posterior = ((p >= 0.40) & (db >= low)) | (p >= 0.65)
                taken = np.count_nonzero(posterior) >= 6
                classes["posterior mask taken" if taken else "energy mask kept"] += 1
                raw = posterior if taken else energy_active
                classes["sibilant frames outside the posterior mask"] += bool(taken and np.any(energy_active & ~mask))
            dil = np.convolve(raw.astype(int), np.ones(3, dtype=int), mode="same") > 0 if F >= 3 else raw
            assert np.array_equal(dil, mask), (name, s)
            sample_mask = np.zeros(n, dtype=bool)
            for f in np.flatnonzero(mask):
                sample_mask[f * SS.HOP: min(n, f * SS.HOP + SS.FRAME)] = True
            for W, H in ((19_200, 4800), (144_000, 48_000)):
                for start in range(0, n - W + 1, H):
                    nearest = min(nearest, abs(float(np.mean(sample_mask[start:start + W])) - 0.55))
            # ---- arg-maxima and the rounding floor of the compared band sums
            frames = np.lib.stride_tricks.sliding_window_view(x, SS.FRAME)[:: SS.HOP]
            if A:
                rows = frames[ev["frame_indices"]]
                centred = (rows - rows.mean(axis=1, keepdims=True)) * window
                power = np.abs(np.fft.rfft(centred, axis=1)) ** 2 + 1e-18
                local = power[:, sib]
                top2 = np.sort(local, axis=1)[:, -2:]
                runner_up = min(runner_up, float(np.min(1.0 - top2[:, 0] / top2[:, 1])))
                cand = np.sort(np.average(power, axis=0, weights=np.maximum(ev["frame_probabilities"], 1e-6))[sib])
                runner_up = min(runner_up, float(1.0 - cand[-2] / cand[-1]))
                floor_power = SS.FRAME * eps * eps * np.sum(centred * centred, axis=1)
                live = floor_power > 0.0
                sums = np.stack([power[:, m].sum(axis=1) for m in band_masks], axis=1)
                if np.any(live):
                    floor_ratio = min(floor_ratio, float(np.min(sums[live] / floor_power[live, None])))
            # ---- classes
            classes["masked-mean fallback"] += F < 19
            classes["short-term fallback"] += n < 144_000 and n >= 19_200
            classes["two short-term windows"] += r["short_term_window_count"] == 2 and n >= 144_000
            classes["posteriors used" if r["vad_probability_used"] else "no posteriors"] += 1
            classes["percentile-10 noise level"] += bool(A and (z is None or z.size < SS.FRAME))
            classes["noise frames"] += bool(A and z is not None and z.size >= SS.FRAME)
            classes["no active frame"] += np.count_nonzero(mask) == 0
            classes["evidence available" if ev["available"] else "evidence unavailable"] += 1
            classes["partial tail chunk"] += n % SS.HOP != 0
            classes["frame below the spectral list"] += A < F
            # The rules on made-up inputs, to reach every profile, preset and status.  The three _recommend_* calls and the two
            # helpers are the reference's; the level percentiles and the caps of :1143-1190 between them are inline code of its
            # analyze_voice_setup and are repeated here -- chain_fixture() below takes those lines from the reference itself.
            if name == "main":
                k = SS.setup_inputs(s)
                level_db = db[mask] if np.count_nonzero(mask) >= 6 else db
                floor_db, body_db, peak_db = (float(np.percentile(level_db, q)) for q in (20.0, 60.0, 95.0))
                snr = body_db - k["conservative_noise_rms_db"]
                snr_conf = V._clamp((k["snr_db"] - 6.0) / 12.0, 0.0, 1.0)
                conf = V._bounded_quality_score([(k["residual_confidence"], 0.30), (snr_conf, 0.22), (k["noise_quality_score"], 0.23),
                                                 (V._clamp(float(r["active_duration_s"]) / 3.0, 0.0, 1.0), 0.17),
                                                 (V._clamp(float(r["loudness_window_count"]) / 8.0, 0.0, 1.0), 0.08)])
                if k["snr_db"] < 6.0:
                    conf = min(conf, 0.40)
                if float(r["active_duration_s"]) < 2.0:
                    conf = min(conf, 0.45)
                if k["used_single_spectrum_fallback"]:
                    conf = min(conf, 0.40)
                if k["noise_status"] == "questionable":
                    conf = min(conf, 0.49)
                elif k["noise_status"] == "invalid":
                    conf = min(conf, 0.20)
                gate = V._recommend_gate_settings(vad_available=k["vad_available"], noise_rms_db=k["conservative_noise_rms_db"],
                                                  speech_floor_db=floor_db, speech_body_db=body_db, speech_snr_db=snr,
                                                  speech_dynamic_range_db=float(r["loudness_range_db"]))
                de, de_diag = V._recommend_deesser_settings(freqs=k["freqs"], spectrum_db=k["smoothed_spectrum_db"], capture_confidence=conf,
                                                            noise_reference_quality=k["noise_quality_score"],
                                                            noise_reference_status=k["noise_status"],
                                                            robust_sibilance_excess_db=float(r["sibilance_excess_db"]), frame_evidence=ev)
                co, co_diag = V._recommend_compressor_settings(target_preset=k["target_preset"], speech_body_db=body_db,
                                                               speech_loudness_lufs=float(r["short_term_lufs"]),
                                                               loudness_range_db=float(r["loudness_range_db"]), speech_snr_db=snr,
                                                               capture_confidence=conf, dynamics_intensity=k["dynamics_intensity"],
                                                               custom_target_p95_db=k["custom_target_p95_db"],
                                                               custom_peak_cap_db=k["custom_peak_cap_db"])
                setup_numbers.append([floor_db, body_db, peak_db, snr, snr_conf, conf, gate["threshold_db"], gate["vad_threshold"],
                                      gate["vad_hold_time_ms"], gate["vad_pre_gain"], gate["gate_margin_db"], de["auto_amount"],
                                      de["low_cut_hz"], de["high_cut_hz"], de["ratio"], de["max_reduction_db"], de_diag["sibilance_excess_db"],
                                      de_diag["peak_hz"], de_diag["frame_evidence_confidence"], de_diag["detection_probability"],
                                      co["threshold_db"], co["ratio"], co["attack_ms"], co["release_ms"], co["makeup_gain_db"],
                                      co["base_release_ms"], co["target_lufs"], co["target_p95_reduction_db"],
                                      co_diag["target_median_reduction_db"], co["peak_reduction_cap_db"],
                                      float(np.clip(k["noise_quality_score"], 0.0, 1.0))])
                setup_flags.append([gate["gate_mode"], gate["auto_threshold_enabled"], de["enabled"], de_diag["frame_evidence_available"],
                                    de_diag["invalid_evidence"], co["auto_makeup_enabled"], PROFILES.index(co["dynamics_intensity"])])
                setup_clip.append(list(de_diag["clip_features"].values()))
                assert gate["enabled"] and gate["attack_ms"] == 5.0 and gate["release_ms"] == 120.0 and de["auto_enabled"]
                assert (de["threshold_db"], de["attack_ms"], de["release_ms"]) == (-28.0, 2.0, 80.0) and co["adaptive_release"]
                assert co["enabled"] and co["sidechain_highpass_enabled"] and co["measured_short_term_lufs"] == r["short_term_lufs"]
                # the cuts of the rules: 6 dB of :1181, 0.55 / 10 dB of :665, the enable threshold.  (The 2 s cut of :1183 compares
                # a whole number of hops over the rate, the same division on both sides; the caps themselves are minima.)
                setup_nearest = min(setup_nearest, abs(k["snr_db"] - 6.0), abs(conf - 0.55), abs(snr - 10.0),
                                    abs(de_diag["detection_probability"] - de_diag["enable_probability_threshold"]))
                hops = round(float(r["active_duration_s"]) * SS.FS / SS.HOP)  # the 2 s cut compares a whole number of hops over the
                assert float(r["active_duration_s"]) == hops * SS.HOP / SS.FS, (s, hops)  # rate: the same division on both sides
                setup_classes.add(("deesser on" if de["enabled"] else "deesser off"))
                setup_classes.add((co["dynamics_intensity"], bool(co["auto_makeup_enabled"])))
            if name == "main" and s in FRAME_STREAMS:
                data[f"main/{s}/frame_db"] = db
                data[f"main/{s}/active_frame_mask"] = mask
                data[f"main/{s}/frame_indices"] = ev["frame_indices"].astype(np.int32)
                data[f"main/{s}/frame_probabilities"] = ev["frame_probabilities"]
                data[f"main/{s}/frame_feature_rows"] = ev["frame_feature_rows"]
        data[f"{name}/speech_sha256"] = np.array(SS.fingerprint(b["speech"])["sha256"])
        data[f"{name}/noise_sha256"] = np.array("" if b["noise"] is None else SS.fingerprint(b["noise"])["sha256"])
        data[f"{name}/vad_sha256"] = np.array("" if b["vad"] is None else SS.fingerprint(b["vad"])["sha256"])
        data[f"{name}/noise_rms_db"] = b["noise_rms_db"]
        data[f"{name}/counts"] = counts
        data[f"{name}/scalars"] = scalars
        print(f"{name}: {B} streams, active frames {counts[:, 1].tolist()[:8]} ..., windows {counts[:, 5].tolist()[:8]} ...")
    data["main/setup_numbers"] = np.array(setup_numbers, dtype=np.float64)
    data["main/setup_flags"] = np.array(setup_flags, dtype=np.int32)
    data["main/setup_clip_features"] = np.array(setup_clip, dtype=np.float64)
    data["setup_nearest_decision"] = np.array(setup_nearest)
    print(f"rules: nearest decision {setup_nearest:.3e}, classes {sorted(map(str, setup_classes))}")
    assert {"deesser on", "deesser off"} <= setup_classes
    assert {(p, m) for p in PROFILES for m in (False, True)} <= setup_classes, setup_classes  # every profile with auto-makeup on and off
    assert setup_nearest > SS.MARGIN, setup_nearest
    chain_fixture(V, SS, data)
    data["batches"] = np.array(list(SS.BATCHES))
    data["classes"] = np.array(sorted(k for k, v in classes.items() if v))
    data["nearest_decision"] = np.array(nearest)
    data["runner_up"] = np.array(runner_up)
    data["floor_ratio"] = np.array(floor_ratio)
    print(f"classes {classes}")
    print(f"nearest decision {nearest:.3e}, smallest arg-max lead {runner_up:.3e}, smallest band sum / rounding floor {floor_ratio:.3e}")
    assert all(classes.values()), classes
    assert nearest > SS.MARGIN, nearest
    assert runner_up > 1e-9, runner_up
    assert floor_ratio > 1e6, floor_ratio
    np.savez_compressed(OUT, **data)
    size = OUT.stat().st_size
    largest = max(p.stat().st_size for p in OUT.parent.iterdir() if p != OUT)
    print(f"wrote {OUT.name}: {size} bytes (largest other fixture {largest})")
    assert size <= largest


if __name__ == "__main__":
    main()
