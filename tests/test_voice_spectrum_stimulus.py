"""The stimuli of the voice spectrum tests are the arrays the fixture was generated from (SHA-256, head, tail), and the
condition the parity tests rest on holds for them: no frame level of any fixture stream lies within 1e-6 dB of a gate, and no
voiced / unvoiced level difference within 1e-6 dB of the 3 dB noise-reference condition.  Re-asserted here from the fixture's
own frame levels and masks (the generator asserted it on the reference's)."""
import numpy as np

import voice_spectrum_stimulus as VS

MARGIN_DB = 1e-6


def test_stimuli_match_the_fingerprints_in_the_fixture():
    fx = VS.fixture()
    assert list(fx["cases"]) == [c["name"] for c in VS.cases()]
    for case in VS.cases():
        name, audio = case["name"], case["audio"]
        if name == "main512":
            audio = audio[fx[f"{name}/streams"]]
        fp = VS.fingerprint(audio)
        assert tuple(fx[f"{name}/shape"]) == audio.shape + (case["nperseg"],), name
        assert np.array_equal(fx[f"{name}/ends"], np.stack([fp["head"], fp["tail"]])), name
        assert str(fx[f"{name}/sha256"]) == fp["sha256"], name
        for extra in ("vad", "noise"):
            if extra in case:
                assert str(fx[f"{name}/{extra}_sha256"]) == VS.fingerprint(case[extra])["sha256"], (name, extra)


def test_main_batch_shape():
    for nperseg in (256, 512):
        assert VS.main_length(nperseg) == 24 * nperseg + 37
        assert (VS.main_length(nperseg) - nperseg) // (nperseg // 2) + 1 == 47
    assert VS.MAIN_STREAMS == 67


def test_no_frame_level_is_within_1e_6_db_of_a_gate():
    nearest, streams = np.inf, 0
    for case in VS.cases():
        fx = VS.fixture_case(case)
        explicit = "noise" in case and case["noise"].shape[1] >= case["nperseg"]
        for i in range(fx["scalars"].shape[0]):  # every stream: none is excluded
            margins = VS.gate_margins(fx["frame_rms_db"][i], fx["voiced_mask"][i], "vad" in case, explicit)
            for what, margin in margins.items():
                assert margin > MARGIN_DB, (case["name"], int(fx["streams"][i]), what, margin)
                nearest = min(nearest, margin)
            streams += 1
    print(f"{streams} streams, nearest decision {nearest:.3e} dB from flipping")
    assert streams >= 67 + 23 + 3 + 1 + 4 + 6 + 5
    assert nearest == float(VS.fixture()["nearest_gate_db"])
