#!/usr/bin/env python3
"""Build-container-only: generate tests/golden/voice_reliability.npz by IMPORTING the reference's own
python/mic_eq/analysis/spectrum.py and running its analyze_voice_spectrum over the stimuli of
tests/voice_reliability_stimulus.py.

What is written is data, never reference text: fingerprints of the stimuli, and per stream what the reference returned on
either branch -- the scalars of VoiceSpectrumResult, the counts behind them, the voiced and inlier masks, the shape distances,
16 checkpoint bins of the four spectra (robust median, repeatability, uncertainty, per-bin SNR), and those spectra in full for
the first stream of every (noise source, block-count class, closest-windows branch) combination at nperseg 256.

It asserts the conditions the parity tests rest on: no window distance within 1e-6 dB of its cutoff, at least one stream with
12 or more effective blocks, at least four with fractional effective blocks, at least two that take the closest-windows branch,
at least one with a bin of the robust per-bin SNR on its -60 dB clamp; and that the file is no larger than the largest fixture
already there.  Re-run:
    python tools/gen_golden_voice_reliability.py      (needs the reference checkout; AF_REFERENCE overrides its place)
"""
from __future__ import annotations

import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
REFERENCE = pathlib.Path(os.environ.get("AF_REFERENCE", "/root/reference"))
OUT = ROOT / "tests" / "golden" / "voice_reliability.npz"
SOURCES = ("unavailable", "explicit_capture", "in_capture_non_speech")
MARGIN_DB = 1e-6


def main() -> None:
    if not (REFERENCE / "python" / "mic_eq" / "analysis" / "spectrum.py").exists():
        raise SystemExit("tools/gen_golden_voice_reliability.py runs in the build container only (the reference is not here)")
    sys.path.insert(0, str(REFERENCE / "python"))
    sys.path.insert(0, str(ROOT / "tests"))
    from mic_eq.analysis import spectrum as R

    import voice_reliability_stimulus as RS
    import voice_spectrum_stimulus as VS

    fs = RS.FS
    data: dict[str, np.ndarray] = {}
    names, nearest = [], np.inf
    seen = {"effective >= 12": 0, "fractional effective": 0, "closest windows": 0, "snr on the clamp": 0}
    for case in RS.cases():
        name, N = case["name"], case["nperseg"]
        streams = RS.fixture_streams(case)
        audio = case["audio"][streams]
        vad, noise = case.get("vad"), case.get("noise")
        B, K, hop = audio.shape[0], N // 2 + 1, N // 2
        F = (audio.shape[1] - N) // hop + 1
        chk = VS.checkpoint_bins(K)
        scalars, counts = np.zeros((B, len(RS.SCALARS))), np.zeros((B, 5), dtype=np.int32)
        flags = np.zeros((B, 2), dtype=np.int32)  # fallback, noise source
        voiced, inlier = np.zeros((B, F), dtype=np.uint8), np.zeros((B, F), dtype=np.uint8)
        distance = np.full((B, F), np.nan)
        spectra = np.full((B, 4, K), np.nan)
        for i, s in enumerate(streams):
            kw = {"vad_probabilities": None if vad is None else vad[s], "noise_audio": None if noise is None else noise[s]}
            res = R.analyze_voice_spectrum(audio[i], fs, N, **kw)
            x = audio[i].astype(float)
            frames = np.lib.stride_tricks.sliding_window_view(x, N)[::hop]
            starts = np.arange(F, dtype=int) * hop
            m = R._voiced_frame_mask(R._frame_rms_db(frames), vad_probabilities=kw["vad_probabilities"], frame_starts=starts,
                                     frame_size=N, sample_rate=fs)
            voiced[i] = m
            fallback = bool(res.used_single_spectrum_fallback)
            flags[i] = fallback, SOURCES.index(res.noise_reference_source)
            scalars[i] = [getattr(res, k) for k in RS.SCALARS]
            spectra[i, 0], spectra[i, 1], spectra[i, 2] = res.median_spectrum_db, res.spectral_repeatability, res.measurement_uncertainty_db
            if res.spectral_snr_db is not None:
                spectra[i, 3] = res.spectral_snr_db
            if fallback:
                continue
            # what the scalars do not show: the shape distances behind the inlier decision, from the rows the reference smoothed
            smoothed = R._measurement_reliability(res.freqs, res.window_spectra_db, starts[m], N)[1]
            band = (res.freqs >= 100.0) & (res.freqs <= 8000.0)
            shape = smoothed - np.median(smoothed[:, band], axis=1)[:, None]
            d = np.sqrt(np.mean(np.square(shape[:, band] - np.median(shape, axis=0)[band]), axis=1))
            V = int(np.count_nonzero(m))
            mid = float(np.median(d))
            cutoff = mid + 4.0 * max(float(np.median(np.abs(d - mid))), 0.25)
            keep = d <= cutoff
            minimum = max(3, int(np.ceil(V * 0.5)))
            closest = int(np.count_nonzero(keep)) < minimum
            if closest:
                keep = np.zeros(V, dtype=bool)
                keep[np.argsort(d, kind="stable")[:minimum]] = True
            assert abs(np.count_nonzero(keep) / V - (1.0 - res.outlier_rejection_ratio)) < 1e-12, (name, s)
            independent, next_start = 0, -1
            for start in starts[m]:
                if start >= next_start:
                    independent, next_start = independent + 1, start + N
            blocks = independent // 3 or 1
            counts[i] = V, independent, blocks, int(np.count_nonzero(keep)), closest
            distance[i, m], inlier[i, m] = d, keep
            margin = RS.cutoff_margin(d)
            assert margin > MARGIN_DB, (name, s, margin)
            nearest = min(nearest, margin)
            eff = res.effective_measurement_blocks
            seen["effective >= 12"] += eff >= 12.0
            seen["fractional effective"] += eff != round(eff)
            seen["closest windows"] += closest
            seen["snr on the clamp"] += res.spectral_snr_db is not None and bool(np.any(res.spectral_snr_db == -60.0))
        keys, full = set(), []
        for i in range(B):
            eff = scalars[i, RS.SCALARS.index("effective_measurement_blocks")]
            key = (flags[i, 1], 0 if counts[i, 2] < 2 else (1 if eff < 12.0 else 2), counts[i, 4])
            if not flags[i, 0] and key not in keys and N == 256:
                keys.add(key)
                full.append(i)
        names.append(name)
        fp = VS.fingerprint(audio)
        data[f"{name}/sha256"] = np.array(fp["sha256"])
        data[f"{name}/shape"] = np.array(audio.shape + (N, F), dtype=np.int64)
        data[f"{name}/streams"] = streams
        data[f"{name}/scalars"] = scalars
        data[f"{name}/counts"] = counts
        data[f"{name}/flags"] = flags
        data[f"{name}/voiced_mask"] = np.packbits(voiced, axis=1)
        data[f"{name}/inlier_mask"] = np.packbits(inlier, axis=1)
        data[f"{name}/distance"] = distance
        data[f"{name}/checkpoints"] = spectra[:, :, chk]
        data[f"{name}/full_streams"] = np.array(full, dtype=np.int64)
        if full:
            data[f"{name}/full_spectra"] = spectra[full]
        main = flags[:, 0] == 0
        print(f"{name}: {B} streams x {F} frames, main branch {int(main.sum())}, closest {int(counts[:, 4].sum())}, blocks "
              f"{sorted(set(counts[main, 2].tolist()))}, effective {np.round(scalars[main, 6], 3).tolist()[:12]}, full {full}")
    data["cases"] = np.array(names)
    data["nearest_cutoff_db"] = np.array(nearest)
    data["conditions"] = np.array([seen[k] for k in sorted(seen)], dtype=np.int64)
    print("conditions:", seen, f"nearest inlier decision {nearest:.3e} dB")
    assert seen["effective >= 12"] >= 1 and seen["fractional effective"] >= 4 and seen["closest windows"] >= 2
    assert seen["snr on the clamp"] >= 1
    np.savez_compressed(OUT, **data)
    size = OUT.stat().st_size
    largest = max(p.stat().st_size for p in OUT.parent.iterdir() if p != OUT)
    print(f"wrote {OUT.name}: {size} bytes (largest other fixture {largest})")
    assert size <= largest


if __name__ == "__main__":
    main()
