"""The stimulus of the EQ headroom validation tests exercises the feature, judged by the reference alone:
tests/golden/headroom_validation.npz holds what the reference's apply_headroom_validation returned for
tests/headroom_stimulus.py (tools/gen_golden_headroom.py, its renders answered by the CPU oracle).  No GPU."""
import hashlib
import pathlib

import numpy as np
import pytest

import headroom_stimulus as HS

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden" / "headroom_validation.npz"
DECISION_MARGIN_DB = 1e-3  # 30 x the DB_ALLOWED the fold is held to (tests/test_gpu_compressor_sweep.py): no decision hangs on rounding


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_file_belongs_to_this_stimulus(golden):
    audio = HS.captures()
    assert audio.shape == (10, 19_533) and audio.dtype == np.float32
    assert HS.N == 20 * 960 + 333 and HS.N_CAPTURES * len(HS.SCALES) == 64 + 6
    assert bytes(golden["sha256"]) == hashlib.sha256(audio.tobytes()).digest()
    assert golden["decisive"].shape == (10, 7, 3) and golden["band_gains"].shape == (10, 10)


def test_stimulus_covers_every_outcome(golden):
    scale, status, flags = golden["gain_scale"], golden["status"], golden["flags"]
    evaluated = ~np.isnan(golden["decisive"][:, :, 0])
    assert scale[0] == 1.0 and status[0] == "safe" and evaluated[0].sum() == 1                 # safe as it comes
    interior = {float(s) for s in scale if 0.0 < s < 1.0}
    assert len(interior) >= 2, interior                                                        # two different interior scales
    assert scale[3] == 0.0 and status[3] == "risk" and flags[3, 0] == 0 and evaluated[3].all()  # hot input: never safe
    assert HS.CHAINS[4]["deesser"]["enabled"] is True
    assert golden["numeric_keys"].tolist().index("deesser_gain_reduction_db") >= 0
    k = golden["numeric_keys"].tolist().index("deesser_gain_reduction_db")
    assert golden["before"][4, k] > 0.5 and np.all(golden["before"][[0, 1, 2, 3], k] == 0.0)     # the de-esser works on capture 4 only
    assert HS.GAINS[5] == [0.0] * 10                                                           # all-zero gains
    limiters = {repr(sorted((c or {}).get("limiter", {}).items())) for c in HS.CHAINS if (c or {}).get("compressor", {}).get("enabled", True)}
    assert len(limiters) >= 2 and HS.CHAINS[6]["limiter"]["ceiling_db"] == -3.0                # a second sweep group
    assert HS.CHAINS[7]["compressor"]["enabled"] is False                                      # the engine route
    for c in range(HS.N_CAPTURES):  # the scaled gains are the f64 products
        index = HS.SCALES.index(float(scale[c]))
        assert golden["band_gains"][c].tolist() == (np.asarray(HS.GAINS[c], dtype=float) * HS.SCALES[index]).tolist()
        assert evaluated[c].sum() == (index + 1 if flags[c, 0] else 7)


def test_no_decision_hangs_on_rounding(golden):
    margins = golden["margins"]
    evaluated = ~np.isnan(margins)
    assert evaluated.sum() == 3 * int((~np.isnan(golden["decisive"][:, :, 0])).sum())
    assert np.nanmin(margins) >= DECISION_MARGIN_DB, (np.nanmin(margins), np.unravel_index(int(np.nanargmin(margins)), margins.shape))
