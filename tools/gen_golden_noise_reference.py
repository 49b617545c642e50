#!/usr/bin/env python3
"""Build-container-only: generate tests/golden/noise_reference.npz by IMPORTING the reference's own
python/mic_eq/analysis/noise_reference.py (and spectrum.py for the override) and running them over the stimuli of
tests/noise_reference_stimulus.py.

What is written is data, never reference text: fingerprints of the stimuli, and per stream what the reference returned --
status, the reason and guidance lists as bit masks over the text tables of tests/noise_reference_oracle.py (the script asserts
that the reference's lists are those texts in table order), every metric, the quality score, 16 checkpoint bins of the three
spectra, the explicit and in-capture spectra in full for the first stream of every main batch (one per sample rate; the
conservative spectrum is their maximum, which the script asserts), and for six streams of main@3000 what the reference's
analyze_voice_spectrum returns when it is handed the conservative spectrum as its noise-spectrum override.

It asserts the conditions the parity tests rest on: every status, every reason bit and every selection class is present; no
decision quantity lies within 1e-6 of its threshold or percentile cut; no compared bin lies within a factor 1e6 of the
transform's rounding floor N eps^2 sum |x w|^2 unless its frame is exactly zero; and the file is no larger than the largest
fixture already there.  Re-run:
    python tools/gen_golden_noise_reference.py      (needs the reference checkout; AF_REFERENCE overrides its place)
"""
from __future__ import annotations

import os
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
REFERENCE = pathlib.Path(os.environ.get("AF_REFERENCE", "/root/reference"))
OUT = ROOT / "tests" / "golden" / "noise_reference.npz"
OVERRIDE_BATCH, OVERRIDE_STREAMS, OVERRIDE_NPERSEG = "main@3000", (0, 5, 9, 10, 11, 13), 256


def main() -> None:
    if not (REFERENCE / "python" / "mic_eq" / "analysis" / "noise_reference.py").exists():
        raise SystemExit("tools/gen_golden_noise_reference.py runs in the build container only (the reference is not here)")
    sys.path.insert(0, str(REFERENCE / "python"))
    sys.path.insert(0, str(ROOT / "tests"))
    from mic_eq.analysis import noise_reference as R
    from mic_eq.analysis import spectrum as SP

    import noise_reference_oracle as NO
    import noise_reference_stimulus as NS

    data: dict[str, np.ndarray] = {}
    names, nearest, floor_ratio = [], np.inf, np.inf
    statuses, reason_bits, guidance_bits = set(), 0, 0
    classes = dict.fromkeys(("selected without vad", "selected with vad", "spread below 6", "too few frames with vad", "no voice",
                             "noise below a frame", "in-capture on the short grid"), 0)
    eps = np.finfo(np.float64).eps
    for b in NS.batches():
        name, fs, B = b["name"], b["fs"], b["noise"].shape[0]
        N = NS.frame_size(fs)
        window = np.hanning(N)
        Ko = NO.bins(fs, b["noise"].shape[1])
        chk = NS.checkpoint_bins(Ko)
        status = np.zeros(B, dtype=np.int32)
        flags = np.zeros((B, 4), dtype=np.int32)  # usable, conservative, identity_metadata_available, in-capture frame count
        masks = np.zeros((B, 2), dtype=np.uint32)
        metrics = np.full((B, len(NO.METRICS)), np.nan)
        quality = np.zeros(B)
        spectra = np.full((B, 3, Ko), np.nan)
        for s in range(B):
            speech = None if b["speech"] is None else b["speech"][s]
            nv = None if b["noise_vad"] is None else b["noise_vad"][s]
            sv = None if b["speech_vad"] is None else b["speech_vad"][s]
            r = R.analyze_noise_reference(b["noise"][s], speech, fs, noise_metadata=b["metadata"][s][0], speech_metadata=b["metadata"][s][1],
                                          noise_vad_probabilities=nv, speech_vad_probabilities=sv)
            status[s] = NO.STATUS.index(r.status)
            masks[s] = sum(1 << NO.REASONS.index(t) for t in r.reasons), sum(1 << NO.GUIDANCE.index(t) for t in r.guidance)
            assert r.reasons == NO.texts(int(masks[s, 0]), NO.REASONS) and r.guidance == NO.texts(int(masks[s, 1]), NO.GUIDANCE), (name, s)
            assert r.usable == (r.status != "invalid") and r.conservative_noise_rms_db == r.metrics["conservative_noise_rms_db"]
            flags[s] = r.usable, r.conservative, r.metrics["identity_metadata_available"], r.metrics["in_capture_noise_frame_count"]
            metrics[s] = [np.nan if r.metrics[k] is None else r.metrics[k] for k in NO.METRICS]
            quality[s] = r.quality_score
            assert r.frequencies.shape == (Ko,), (name, s)
            spectra[s, 0], spectra[s, 1] = r.explicit_spectrum_db, r.conservative_spectrum_db
            if r.in_capture_spectrum_db is not None:
                spectra[s, 2] = r.in_capture_spectrum_db
            # the age and mismatch arguments say what the metadata says
            reasons, age = R._metadata_mismatches(R.CaptureMetadata.coerce(b["metadata"][s][0]), R.CaptureMetadata.coerce(b["metadata"][s][1]), fs)
            assert (age is None) == bool(np.isnan(b["age"][s])) and (age is None or age == max(0.0, b["age"][s])), (name, s)
            assert sum(1 << (NO.REASONS.index(t) - 12) for t in reasons) == int(b["mismatch"][s]), (name, s)

            # how close the decisions are, and how far the compared bins are from the rounding floor
            clean = lambda x: np.where(np.isfinite(x), x, 0.0).astype(float)  # noqa: E731
            nf = R._frame_analysis(clean(b["noise"][s]), fs)
            sf = None if speech is None else R._frame_analysis(clean(speech), fs)
            n_post = None if nf is None else R._interpolate_vad(nv, nf.frame_rms_db.size)
            s_post = None if sf is None else R._interpolate_vad(sv, sf.frame_rms_db.size)
            nearest = min(nearest, NS.margins(r.metrics, None if sf is None else sf.frame_rms_db, s_post, n_post))
            compared = np.arange(Ko) if s == 0 and name.startswith("main@") else chk
            for capture, fa in ((clean(b["noise"][s]), nf), (None if speech is None else clean(speech), sf)):
                if fa is None or (fa is sf and r.in_capture_spectrum_db is None) or nf is None:
                    continue
                frames = np.lib.stride_tricks.sliding_window_view(capture, N)[:: N // 2]
                centred = (frames - frames.mean(axis=1, keepdims=True)) * window
                floor = N * eps * eps * np.sum(centred * centred, axis=1) / np.sum(window * window)
                power = 10.0 ** (fa.spectra_db[:, compared] / 10.0)
                live = floor > 0.0
                if np.any(live):
                    floor_ratio = min(floor_ratio, float(np.min(power[live] / floor[live, None])))
            if sf is None:
                classes["no voice"] += speech is None
            elif r.in_capture_spectrum_db is not None:
                classes["selected with vad" if sv is not None else "selected without vad"] += 1
                classes["in-capture on the short grid"] += nf is None
            elif sv is not None:
                classes["too few frames with vad"] += 0 < r.metrics["in_capture_noise_frame_count"]
            else:
                rms = sf.frame_rms_db
                classes["spread below 6"] += float(np.percentile(rms, 90.0) - np.percentile(rms, 10.0)) < 6.0
            classes["noise below a frame"] += nf is None
            statuses.add(r.status)
            reason_bits |= int(masks[s, 0])
            guidance_bits |= int(masks[s, 1])
        names.append(name)
        data[f"{name}/noise_sha256"] = np.array(NS.fingerprint(b["noise"])["sha256"])
        data[f"{name}/speech_sha256"] = np.array("" if b["speech"] is None else NS.fingerprint(b["speech"])["sha256"])
        data[f"{name}/shape"] = np.array(b["noise"].shape + (0 if b["speech"] is None else b["speech"].shape[1], fs), dtype=np.int64)
        data[f"{name}/status"] = status
        data[f"{name}/flags"] = flags
        data[f"{name}/masks"] = masks
        data[f"{name}/metrics"] = metrics
        data[f"{name}/quality"] = quality
        data[f"{name}/checkpoints"] = spectra[:, :, chk]
        if name.startswith("main@"):  # conservative is the larger of the two wherever the third exists (:453), the first elsewhere
            data[f"{name}/full_spectra"] = spectra[0, [0, 2]]
            assert np.array_equal(spectra[0, 1], np.fmax(spectra[0, 0], spectra[0, 2])), name
        print(f"{name}: {B} streams, statuses {np.bincount(status, minlength=3).tolist()}, reasons {sorted(set(masks[:, 0].tolist()))[:8]} ...")

        if name == OVERRIDE_BATCH:  # voice_setup.py:1122-1162: the conservative spectrum as analyze_voice_spectrum's noise reference
            K = OVERRIDE_NPERSEG // 2 + 1
            vchk = NS.checkpoint_bins(K)
            scalars, points = np.zeros((len(OVERRIDE_STREAMS), 2)), np.full((len(OVERRIDE_STREAMS), 2, 16), np.nan)
            sources = []
            for i, s in enumerate(OVERRIDE_STREAMS):
                r = R.analyze_noise_reference(b["noise"][s], b["speech"][s], fs, noise_metadata=b["metadata"][s][0],
                                              speech_metadata=b["metadata"][s][1])
                v = SP.analyze_voice_spectrum(b["speech"][s], fs, OVERRIDE_NPERSEG, noise_audio=b["noise"][s],
                                              noise_spectrum_override=(r.frequencies, r.conservative_spectrum_db),
                                              noise_reference_source_override="validated_conservative")
                sources.append(v.noise_reference_source)
                scalars[i] = v.snr_db, v.used_single_spectrum_fallback
                points[i, 0], points[i, 1] = v.noise_spectrum_db[vchk], v.spectral_snr_db[vchk]
            data["override/streams"] = np.array(OVERRIDE_STREAMS, dtype=np.int64)
            data["override/sources"] = np.array(sources)
            data["override/scalars"] = scalars
            data["override/checkpoints"] = points
            assert set(sources) == {"validated_conservative"}, sources
            print("override:", sources[0], np.round(scalars[:, 0], 3).tolist(), "fallback", scalars[:, 1].tolist())

    data["batches"] = np.array(names)
    data["nearest_decision"] = np.array(nearest)
    data["floor_ratio"] = np.array(floor_ratio)
    print(f"statuses {sorted(statuses)}, reason bits {reason_bits:#x}, guidance bits {guidance_bits:#x}, classes {classes}")
    print(f"nearest decision {nearest:.3e}, smallest compared bin / rounding floor {floor_ratio:.3e}")
    assert statuses == set(NO.STATUS)
    assert reason_bits == (1 << len(NO.REASONS)) - 1, f"{reason_bits:#x}"
    assert guidance_bits == (1 << len(NO.GUIDANCE)) - 1, f"{guidance_bits:#x}"
    assert all(classes.values()), classes
    assert nearest > NS.MARGIN, nearest
    assert floor_ratio > 1e6, floor_ratio
    np.savez_compressed(OUT, **data)
    size = OUT.stat().st_size
    largest = max(p.stat().st_size for p in OUT.parent.iterdir() if p != OUT)
    print(f"wrote {OUT.name}: {size} bytes (largest other fixture {largest})")
    assert size <= largest


if __name__ == "__main__":
    main()
