#!/usr/bin/env python3
"""Build-container-only: generate tests/golden/voice_spectrum.npz by IMPORTING the reference's own
python/mic_eq/analysis/spectrum.py and running it over the stimuli of tests/voice_spectrum_stimulus.py.

What is written is data, never reference text: fingerprints of the stimuli, and per stream what the reference's functions
returned -- frame levels, masks, scalars, spectra (in full for a few streams that cover every branch, 16 checkpoint bins for
the others), one raw and smoothed window spectrum per full stream, and the fractional-octave band tables.

It asserts the condition the parity tests rest on: no frame level of any stream lies within 1e-6 dB of a gate, and no
voiced / unvoiced level difference within 1e-6 dB of 3 dB.  Re-run:
    python tools/gen_golden_voice_spectrum.py      (needs the reference checkout; AF_REFERENCE overrides its place)
"""
from __future__ import annotations

import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
REFERENCE = pathlib.Path(os.environ.get("AF_REFERENCE", "/root/reference"))
OUT = ROOT / "tests" / "golden" / "voice_spectrum.npz"
SOURCES = ("unavailable", "explicit_capture", "in_capture_non_speech")
SPECTRA = ("speech_db", "noise_db", "spectral_snr_db", "welch_db")
MARGIN_DB = 1e-6


def main() -> None:
    if not (REFERENCE / "python" / "mic_eq" / "analysis" / "spectrum.py").exists():
        raise SystemExit("tools/gen_golden_voice_spectrum.py runs in the build container only (the reference is not here)")
    sys.path.insert(0, str(REFERENCE / "python"))
    sys.path.insert(0, str(ROOT / "tests"))
    from mic_eq.analysis import spectrum as R

    import voice_spectrum_stimulus as VS

    fs = VS.FS
    data: dict[str, np.ndarray] = {}
    names, worst = [], np.inf
    for case in VS.cases():
        name, N, audio = case["name"], case["nperseg"], case["audio"]
        vad, noise = case.get("vad"), case.get("noise")
        streams = np.arange(audio.shape[0])
        if name == "main512":  # the fixture's size limit: every third stream (fallback, gated and steady ones among them)
            streams = streams[::3]
            audio = audio[streams]
        B, K, hop = audio.shape[0], N // 2 + 1, N // 2
        F = (audio.shape[1] - N) // hop + 1
        chk = VS.checkpoint_bins(K)
        scal = np.zeros((B, 9))
        rms, mask = np.zeros((B, F)), np.zeros((B, F), dtype=np.uint8)
        spectra = np.full((B, 4, K), np.nan)
        windows = np.full((B, 2, K), np.nan)
        freqs = None
        for s in range(B):
            x = audio[s].astype(float)
            kw = {"vad_probabilities": None if vad is None else vad[s], "noise_audio": None if noise is None else noise[s]}
            res = R.analyze_voice_spectrum(audio[s], fs, N, **kw)
            frames = np.lib.stride_tricks.sliding_window_view(x, N)[::hop]
            rms[s] = R._frame_rms_db(frames)
            starts = np.arange(F, dtype=int) * hop
            m = R._voiced_frame_mask(rms[s], vad_probabilities=kw["vad_probabilities"], frame_starts=starts, frame_size=N, sample_rate=fs)
            mask[s] = m
            speech = R._median_frame_spectrum_db(frames[m], fs)
            freqs, welch = R.compute_voice_spectrum(audio[s], fs, N)
            spectra[s, 3] = welch
            if speech is not None:
                spectra[s, 0] = speech[1]
                raw = R._window_spectrum_db(frames[m][0], fs)[1]
                windows[s] = raw, R.smooth_spectrum_perceptual(freqs, raw)
            fallback = bool(res.used_single_spectrum_fallback)
            if res.noise_spectrum_db is not None:
                # the per-bin SNR of :603; the result carries it on the fallback branch only (beyond it, the robust median's)
                spectra[s, 1], spectra[s, 2] = res.noise_spectrum_db, R._spectral_snr_db(speech[1], res.noise_spectrum_db)
                if fallback:
                    assert np.array_equal(res.spectral_snr_db, spectra[s, 2])
            if fallback:
                assert np.array_equal(res.median_spectrum_db, welch)
            scal[s] = (F, int(np.count_nonzero(m)), res.voiced_window_ratio, float(res.vad_probability_used),
                       res.vad_active_window_ratio, SOURCES.index(res.noise_reference_source), float(fallback),
                       res.snr_db if fallback else np.nan, res.spectral_tilt_db_per_octave if fallback else np.nan)
            margins = VS.gate_margins(rms[s], m, vad is not None, noise is not None and noise.shape[1] >= N)
            near = min(margins.values())
            assert near > MARGIN_DB, (name, s, margins)
            worst = min(worst, near)
        # the streams kept in full: the first of every (fallback, source, all-voiced) combination
        keys, full = set(), []
        for s in range(B):
            key = (scal[s, 6], scal[s, 5], scal[s, 1] == F, scal[s, 3])
            if key not in keys and N == 256 and not name.startswith("short"):
                keys.add(key)
                full.append(s)
        names.append(name)
        fp = VS.fingerprint(audio)
        data[f"{name}/sha256"] = np.array(fp["sha256"])
        data[f"{name}/ends"] = np.stack([fp["head"], fp["tail"]])
        data[f"{name}/shape"] = np.array(audio.shape + (N,), dtype=np.int64)
        for extra, arr in (("vad", vad), ("noise", noise)):
            if arr is not None:
                data[f"{name}/{extra}_sha256"] = np.array(VS.fingerprint(arr)["sha256"])
        data[f"{name}/streams"] = streams
        data[f"{name}/scalars"] = scal
        data[f"{name}/frame_rms_db"] = rms
        data[f"{name}/voiced_mask"] = np.packbits(mask, axis=1)
        data[f"{name}/checkpoints"] = spectra[:, :, chk]
        if name == "main4096":
            data["freqs4096_checkpoints"] = freqs[chk]
        data[f"{name}/full_streams"] = np.array(full, dtype=np.int64)
        if full:
            data[f"{name}/full_spectra"] = spectra[full]
            data[f"{name}/full_windows"] = windows[full[:1]]  # of the first one
        print(f"{name}: {B} streams x {F} frames, fallback {int(scal[:, 6].sum())}, sources "
              f"{[int(np.sum(scal[:, 5] == k)) for k in range(3)]}, all voiced {int(np.sum(scal[:, 1] == F))}, vad {int(scal[:, 3].sum())}, "
              f"full {full}")
    data["cases"] = np.array(names)
    data["freqs256"] = R.compute_voice_spectrum(np.zeros(256, dtype=np.float32), fs, 256)[0]
    for fraction in (2, 3, 6, 12):
        data[f"octave{fraction}"] = np.stack(R.get_octave_frequencies(fraction))
    data["nearest_gate_db"] = np.array(worst)
    np.savez_compressed(OUT, **data)
    size = OUT.stat().st_size
    largest = max(p.stat().st_size for p in OUT.parent.iterdir() if p != OUT)
    print(f"nearest decision margin {worst:.3e} dB; wrote {OUT.name}: {size} bytes (largest other fixture {largest})")
    assert size <= largest


if __name__ == "__main__":
    main()
