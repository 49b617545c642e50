"""The stimuli of the speech-feature tests are the arrays the fixture's generator ran the reference over: same batches, shapes,
fingerprints and noise levels, and the classes the generator found present are the ones the tests count on."""
import numpy as np

import speech_features_stimulus as SS

CLASSES = ("masked-mean fallback", "short-term fallback", "two short-term windows", "posteriors used", "no posteriors", "energy mask kept",
           "posterior mask taken", "percentile-10 noise level", "noise frames", "no active frame", "evidence available",
           "evidence unavailable", "non-finite", "partial tail chunk", "frame below the spectral list",
           "sibilant frames outside the posterior mask")


def test_batches_are_the_ones_the_fixture_was_made_from():
    fx = SS.fixture()
    assert list(fx["batches"]) == list(SS.BATCHES)
    for name, (B, n, m, with_vad, kinds) in SS.BATCHES.items():
        b = SS.batch(name)
        assert b["speech"].shape == (B, n) and b["speech"].dtype == np.float32
        assert (b["noise"] is None) == (m == 0) and (b["noise"] is None or b["noise"].shape == (B, m))
        assert (b["vad"] is None) == (not with_vad) and (b["vad"] is None or b["vad"].shape == (B, -(-n // SS.VAD_WINDOW)))
        assert str(fx[f"{name}/speech_sha256"]) == SS.fingerprint(b["speech"])["sha256"], name
        assert str(fx[f"{name}/noise_sha256"]) == ("" if b["noise"] is None else SS.fingerprint(b["noise"])["sha256"]), name
        assert str(fx[f"{name}/vad_sha256"]) == ("" if b["vad"] is None else SS.fingerprint(b["vad"])["sha256"]), name
        assert np.array_equal(fx[f"{name}/noise_rms_db"], b["noise_rms_db"]), name
        assert fx[f"{name}/counts"].shape[0] == B


def test_every_class_is_present():
    fx = SS.fixture()
    assert sorted(fx["classes"]) == sorted(CLASSES)
    main = SS.BATCHES["main"]
    assert main[0] == 67 and main[1] == 201_600 and SS.frames(main[1]) == 209  # one past the 64-lane tile; two short-term windows
    assert [SS.BATCHES[k][1] for k in ("one_frame", "tail", "one_window", "no_short_term")] == [1920, 2879, 19_200, 120_000]
    special = SS.batch("special")
    assert special["kinds"] == ("voice", "all_zero", "steady", "nan", "voice")
    assert not special["speech"][1].any() and np.isnan(special["speech"][3]).sum() == 1
    counts = fx["special/counts"]
    assert counts[1, 1] == 0 and counts[2, 1] == 0 and counts[3, 0] == -1  # no active frame in the zero and steady streams
    # broadband bursts on some streams and none on others
    assert sum(SS.sibilance_db(s) is None for s in range(67)) == 23


def test_whole_capture_pairs_are_the_ones_the_fixture_was_made_from():
    fx, c = SS.fixture(), SS.chain_batch()
    assert c["speech"].shape == (6, 201_600) and c["noise"].shape == (6, SS.CHAIN_NOISE_SAMPLES) and c["noise"].dtype == np.float32
    assert c["vad"].shape == (6, 132) and c["noise_vad"].shape == (6, 63)
    assert np.array_equal(c["speech"], SS.batch("main")["speech"][list(SS.CHAIN_STREAMS)])
    for key in ("speech", "vad", "noise", "noise_vad"):
        assert str(fx[f"chain/{key}_sha256"]) == SS.fingerprint(c[key])["sha256"], key
    for a in range(len(SS.CHAIN_ARGUMENTS)):
        assert fx[f"chain/{a}/numbers"].shape == (6, 32) and fx[f"chain/{a}/flags"].shape == (6, 4)
        assert set(fx[f"chain/{a}/flags"][:, 2]) == {0, 1} and set(fx[f"chain/{a}/flags"][:, 3]) == {0, 1}  # de-esser, auto-makeup
    assert set(fx["chain/1/profiles"]) == {3} and set(fx["chain/0/profiles"]) == {1}
    assert float(fx["chain/nearest_decision"]) > SS.MARGIN
