"""The stimuli of the room-noise reference tests are the arrays the reference saw (fingerprints in
tests/golden/noise_reference.npz), their age and mismatch arguments say what their metadata says, and between them they hold
every class the parity tests rest on."""
import numpy as np

import noise_reference_oracle as NO
import noise_reference_stimulus as NS


def test_fingerprints_match_the_fixture():
    fx = NS.fixture()
    assert list(fx["batches"]) == [b["name"] for b in NS.batches()]
    for b in NS.batches():
        name = b["name"]
        assert str(fx[f"{name}/noise_sha256"]) == NS.fingerprint(b["noise"])["sha256"], name
        assert str(fx[f"{name}/speech_sha256"]) == ("" if b["speech"] is None else NS.fingerprint(b["speech"])["sha256"]), name
        shape = b["noise"].shape + (0 if b["speech"] is None else b["speech"].shape[1], b["fs"])
        assert tuple(fx[f"{name}/shape"]) == shape, name
        assert b["noise"].dtype == np.float32 and (b["speech"] is None or b["speech"].dtype == np.float32)


def test_sizes_are_the_ones_the_issue_sets():
    by_rate = {b["fs"]: b for b in NS.batches() if b["name"].startswith("main@")}
    assert tuple(by_rate) == NS.RATES == (2560, 3000, 3150, 4410, 48_000)
    assert [NS.frame_size(fs) for fs in NS.RATES] == [512, 600, 630, 882, 9600]
    assert by_rate[3000]["noise"].shape[0] == 67 and by_rate[48_000]["noise"].shape[0] <= 6
    for fs, b in by_rate.items():
        assert NO.frames(fs, b["noise"].shape[1]) == NS.NOISE_FRAMES and NO.frames(fs, b["speech"].shape[1]) == NS.VOICE_FRAMES
        assert b["noise"].shape[1] / fs >= 1.5  # long enough for a usable verdict


def test_arguments_say_what_the_metadata_says():
    from mic_eq_mi import mic_eq_core as core

    for b in NS.batches():
        for s, (noise_meta, voice_meta) in enumerate(b["metadata"]):
            age, mask, _ = core._metadata_arguments(noise_meta, voice_meta, b["fs"])
            assert mask == int(b["mismatch"][s]), (b["name"], s)
            assert (np.isnan(age) and np.isnan(b["age"][s])) or age == b["age"][s], (b["name"], s)


def test_the_fixture_holds_every_class():
    fx = NS.fixture()
    statuses, reasons, guidance = set(), 0, 0
    for name in fx["batches"]:
        statuses |= set(fx[f"{name}/status"].tolist())
        reasons |= int(np.bitwise_or.reduce(fx[f"{name}/masks"][:, 0]))
        guidance |= int(np.bitwise_or.reduce(fx[f"{name}/masks"][:, 1]))
    assert statuses == {0, 1, 2}
    assert reasons == (1 << len(NO.REASONS)) - 1 and guidance == (1 << len(NO.GUIDANCE)) - 1
    assert float(fx["nearest_decision"]) > NS.MARGIN and float(fx["floor_ratio"]) > 1e6
    assert list(fx["override/sources"]) == ["validated_conservative"] * 6
