#!/usr/bin/env python3
"""Build-container-only: generate tests/golden/speech_features_rates.npz by IMPORTING the reference's own
python/mic_eq/analysis/voice_setup.py and scipy, and running them over the stimuli of tests/speech_features_rates_stimulus.py.

What is written is data, never reference text:
  * per analysed batch (the main batch at 16, 32, 44.1 and 96 kHz, the small batches at 44.1 kHz) what the reference's
    _vad_masked_speech_features returned per stream -- counts and every scalar -- and for two streams of each main batch the
    per-frame arrays;
  * scipy.signal.resample_poly's output for one short stream at each of the seven resampled rates;
  * analyze_voice_setup's return for three 44.1 kHz capture pairs, fed the stimulus' posteriors in place of its native VAD
    helper and run without the Auto-EQ optimiser, exactly as tools/gen_golden_speech_features.py does at 48 kHz.

It asserts, on the reference alone, the conditions the parity tests rest on: no resampled mask value within 1e-6 of its 0.5
cut; no loudness window with exactly 10560 of its 19200 samples active and none whose active fraction is within 1e-6 of 0.55;
every frame level at least 1e-6 from the adaptive floor and the supported-energy floor, every posterior at least 1e-6 from
0.40 and 0.65; every arg-max with a runner-up at least 1e-9 relative below it; the cuts of the rules on the capture pairs at
least 1e-6 away; and the file is at most 150 KB.  Re-run:
    python tools/gen_golden_speech_features_rates.py     (needs the reference checkout; AF_REFERENCE overrides its place)
"""
from __future__ import annotations

import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
REFERENCE = pathlib.Path(os.environ.get("AF_REFERENCE", "/root/reference"))
OUT = ROOT / "tests" / "golden" / "speech_features_rates.npz"
FRAME_STREAMS = (1, 66)  # streams of every main batch whose per-frame arrays are kept

sys.path.insert(0, str(ROOT / "tools"))
from gen_golden_speech_features import BANDS, CHAIN_FLAGS, CHAIN_NUMBERS, COUNTS, EVIDENCE, PROFILES, SCALARS  # noqa: E402


def main() -> None:
    if not (REFERENCE / "python" / "mic_eq" / "analysis" / "voice_setup.py").exists():
        raise SystemExit("tools/gen_golden_speech_features_rates.py runs in the build container only (the reference is not here)")
    sys.path.insert(0, str(REFERENCE / "python"))
    sys.path.insert(0, str(ROOT / "tests"))
    from scipy.signal import resample_poly

    from mic_eq.analysis import voice_setup as V
    from mic_eq.analysis.spectrum import _interpolate_vad_probabilities

    import speech_features_rates_stimulus as RS

    data: dict[str, np.ndarray] = {}
    nearest, mask_margin, window_margin, runner_up = np.inf, np.inf, np.inf, np.inf
    classes = dict.fromkeys(("masked-mean fallback", "one momentary window", "short-term window", "short-term fallback", "posteriors used",
                             "no posteriors", "percentile-10 noise level", "noise frames", "no active frame", "non-finite",
                             "partial tail chunk", "band cap binds"), 0)
    for name in RS.ANALYZED:
        b = RS.batch(name)
        fs, B, n = b["fs"], b["speech"].shape[0], b["speech"].shape[1]
        H, N = RS.hop(fs), RS.frame(fs)
        up, down = 48_000 // int(np.gcd(fs, 48_000)), fs // int(np.gcd(fs, 48_000))
        freqs = np.fft.rfftfreq(N, 1.0 / fs)
        sib = (freqs >= 5000.0) & (freqs <= min(9500.0, fs * 0.45))
        window = np.hanning(N)
        counts = np.zeros((B, len(COUNTS)), dtype=np.int64)
        scalars = np.full((B, len(SCALARS) + len(BANDS) + len(EVIDENCE)), np.nan)
        classes["band cap binds"] += fs * 0.45 < 9500.0
        for s in range(B):
            x = b["speech"][s].astype(np.float64)
            vad = None if b["vad"] is None else b["vad"][s]
            z = None if b["noise"] is None else b["noise"][s].astype(np.float64)
            level = float(b["noise_rms_db"][s])
            if not np.all(np.isfinite(x)):
                counts[s] = -1
                classes["non-finite"] += 1
                continue
            r = V._vad_masked_speech_features(x, fs, level, vad, z)
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
            nearest = min(nearest, float(np.min(np.abs(db - floor))))
            if vad is not None:
                p = _interpolate_vad_probabilities(vad, np.arange(F) * H, N, fs)
                low = max(level + 2.0, floor - 4.0)
                nearest = min(nearest, float(np.min(np.abs(p - 0.40))), float(np.min(np.abs(p - 0.65))), float(np.min(np.abs(db - low))))
            sample_mask = np.zeros(n, dtype=bool)
            for f in np.flatnonzero(mask):
                sample_mask[f * H: min(n, f * H + N)] = True
            resampled = resample_poly(sample_mask.astype(np.float64), up, down)
            mask_margin = min(mask_margin, float(np.min(np.abs(resampled - 0.5))))
            weighted_mask = resampled >= 0.5
            n48 = weighted_mask.size
            for W, step in ((19_200, 4800), (144_000, 48_000)):
                for start in range(0, n48 - W + 1, step):
                    active = int(np.count_nonzero(weighted_mask[start:start + W]))
                    if W == 19_200:
                        assert active != 10_560, (name, s, start)
                    window_margin = min(window_margin, abs(active / W - 0.55))
            if A:
                rows = np.lib.stride_tricks.sliding_window_view(x, N)[::H][ev["frame_indices"]]
                centred = (rows - rows.mean(axis=1, keepdims=True)) * window
                power = np.abs(np.fft.rfft(centred, axis=1)) ** 2 + 1e-18
                top2 = np.sort(power[:, sib], axis=1)[:, -2:]
                runner_up = min(runner_up, float(np.min(1.0 - top2[:, 0] / top2[:, 1])))
                cand = np.sort(np.average(power, axis=0, weights=np.maximum(ev["frame_probabilities"], 1e-6))[sib])
                runner_up = min(runner_up, float(1.0 - cand[-2] / cand[-1]))
            classes["masked-mean fallback"] += n48 < 19_200
            classes["one momentary window"] += 19_200 <= n48 < 24_000
            classes["short-term window"] += n48 >= 144_000
            classes["short-term fallback"] += 19_200 <= n48 < 144_000
            classes["posteriors used" if r["vad_probability_used"] else "no posteriors"] += 1
            classes["percentile-10 noise level"] += bool(A and (z is None or z.size < N))
            classes["noise frames"] += bool(A and z is not None and z.size >= N)
            classes["no active frame"] += np.count_nonzero(mask) == 0
            classes["partial tail chunk"] += n48 % 960 != 0
            if name.startswith("main_") and s in FRAME_STREAMS:
                data[f"{name}/{s}/frame_db"] = db
                data[f"{name}/{s}/active_frame_mask"] = mask
                data[f"{name}/{s}/frame_indices"] = ev["frame_indices"].astype(np.int32)
                data[f"{name}/{s}/frame_probabilities"] = ev["frame_probabilities"]
                data[f"{name}/{s}/frame_feature_rows"] = ev["frame_feature_rows"]
        data[f"{name}/speech_sha256"] = np.array(RS.fingerprint(b["speech"])["sha256"])
        data[f"{name}/noise_rms_db"] = b["noise_rms_db"]
        data[f"{name}/counts"] = counts
        data[f"{name}/scalars"] = scalars
        print(f"{name}: {B} streams at {fs} Hz, active frames {counts[:, 1].tolist()[:6]} ..., windows {counts[:, 5].tolist()[:6]} ...")

    # ---- resample_poly itself on one short stream per rate
    for fs in RS.RATES:
        if fs == 48_000:
            continue
        g = int(np.gcd(fs, 48_000))
        x = RS.resample_input(fs)
        y = resample_poly(x.astype(np.float64), 48_000 // g, fs // g)
        assert y.size >= 2 * (48_000 // g), fs  # at least two cycles of the filter's phases
        data[f"resample/{fs}/input_sha256"] = np.array(RS.fingerprint(x)["sha256"])
        data[f"resample/{fs}/output"] = y

    # ---- analyze_voice_setup on three whole 44.1 kHz capture pairs
    c = RS.chain_batch()
    current = {}

    def stimulus_vad(audio, sample_rate, **_):
        return (current["vad"] if np.asarray(audio).size == c["speech"].shape[1] else current["noise_vad"]).copy(), "stimulus"

    def no_auto_eq(*_, **__):
        raise RuntimeError("Auto-EQ is not part of this fixture")

    V.analyze_offline_vad, V.analyze_auto_eq = stimulus_vad, no_auto_eq
    numbers, flags, profiles, statuses, chain_nearest = [], [], [], [], np.inf
    for i in range(c["speech"].shape[0]):
        current.update(vad=c["vad"][i], noise_vad=c["noise_vad"][i])
        r = V.analyze_voice_setup(c["noise"][i], c["speech"][i], c["fs"], "broadcast")
        d = r["diagnostics"]
        assert r["eq_settings"] is None and d["vad_analysis_backend"] == "stimulus" and d["vad_probability_used"]
        numbers.append([r[where][key] for key, where in CHAIN_NUMBERS])
        flags.append([int(r[where][key]) for key, where in CHAIN_FLAGS])
        profiles.append(PROFILES.index(r["compressor_settings"]["dynamics_intensity"]))
        statuses.append(d["noise_reference_quality"]["status"])
        chain_nearest = min(chain_nearest, abs(d["noise_referenced_snr_db"] - 6.0), abs(d["capture_confidence"] - 0.55),
                            abs(d["speech_snr_db"] - 10.0),
                            abs(d["deesser_detection_probability"] - d["deesser_enable_probability_threshold"]))
    data["chain/numbers"] = np.array(numbers, dtype=np.float64)
    data["chain/flags"] = np.array(flags, dtype=np.int32)
    data["chain/profiles"] = np.array(profiles, dtype=np.int32)
    data["chain/status"] = np.array(statuses)
    data["chain/nearest_decision"] = np.array(chain_nearest)
    for key in ("speech", "vad", "noise", "noise_vad"):
        data[f"chain/{key}_sha256"] = np.array(RS.fingerprint(c[key])["sha256"])

    data["batches"] = np.array(list(RS.ANALYZED))
    data["classes"] = np.array(sorted(k for k, v in classes.items() if v))
    data["nearest_decision"] = np.array(nearest)
    data["mask_margin"] = np.array(mask_margin)
    data["window_margin"] = np.array(window_margin)
    data["runner_up"] = np.array(runner_up)
    print(f"classes {classes}")
    print(f"nearest decision {nearest:.3e}, resampled mask from 0.5 {mask_margin:.3e}, windows from 0.55 {window_margin:.3e}, "
          f"arg-max lead {runner_up:.3e}, chain nearest {chain_nearest:.3e}, chain status {statuses}")
    assert all(classes.values()), classes
    assert nearest > RS.MARGIN and mask_margin > RS.MARGIN and window_margin > RS.MARGIN and chain_nearest > RS.MARGIN
    assert runner_up > 1e-9, runner_up
    np.savez_compressed(OUT, **data)
    size = OUT.stat().st_size
    print(f"wrote {OUT.name}: {size} bytes")
    assert size <= 150 * 1024, size


if __name__ == "__main__":
    main()
