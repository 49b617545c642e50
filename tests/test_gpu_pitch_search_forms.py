"""supp_pitchsearch4_kernel against a recording of its own earlier form, bit for bit.

tests/golden/pitch_search_parent.npz was taken once on an MI355X (tools/record_pitch_search.py) from the build before the
coarse correlation went from 96 to 64 matrix steps and the fine stage from 294 scanned lags to its at most ten candidates:
the search's own index of every cell and a 64-bit hash of every cell's whitened buffer, on the stimulus of
tests/pitch_search_forms_stimulus.py -- the synthetic spans at 1, 3, 4 and 6 frames, the 31 streams x 43 frames of the
pitch-stage stimulus (the largest run) and the single-frame spans that steer the coarse winner into every row and column of
the matrix form.  tests/test_pitch_search_forms_ref.py proves on the CPU what that stimulus reaches.  Both changes keep every
surviving operation's operands and order, so nothing may differ: not an index, not a bit of a buffer.  DESIGN.md 4.5 says
what three mutated builds did to this test.
"""
import os

import numpy as np
import pytest

import pitch_search_forms_stimulus as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pitch_search_parent.npz")


@pytest.fixture(scope="module")
def recording():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def device():
    import mic_eq_mi

    assert mic_eq_mi.CORE_AVAILABLE
    run = {}
    for name, spans, frames in F.parts():
        ds, index = mic_eq_mi.Engine.suppressor_debug_pitch_search(spans)
        assert ds.shape == (frames, spans.shape[0], 864) and index.shape == ds.shape[:2]
        run[name] = (ds, index)
    return run


def test_recording_covers_the_stimulus(recording):
    names = [p[0] for p in F.parts()]
    assert sorted(recording) == sorted([f"{n}_index" for n in names] + [f"{n}_hash" for n in names])
    for name, spans, frames in F.parts():
        assert recording[f"{name}_index"].shape == (frames, spans.shape[0]) and recording[f"{name}_index"].dtype == np.int16
        assert recording[f"{name}_hash"].shape == (frames, spans.shape[0]) and recording[f"{name}_hash"].dtype == np.uint64
    assert max(frames * spans.shape[0] for _, spans, frames in F.parts()) == 31 * 43


@pytest.mark.parametrize("name", [p[0] for p in F.parts()])
def test_index_and_whitened_buffer_bit_for_bit(recording, device, name):
    ds, index = device[name]
    want = recording[f"{name}_index"].astype(np.int64)
    bad = np.argwhere(index != want)
    print(f"{name}: {index.size} cells, {len(bad)} indices differ")
    assert bad.size == 0, [(int(f), int(s), int(index[f, s]), int(want[f, s])) for f, s in bad[:8]]
    got = F.buffer_hashes(ds)
    bad = np.argwhere(got != recording[f"{name}_hash"])
    assert bad.size == 0, ("whitened buffer", [(int(f), int(s)) for f, s in bad[:8]])


def test_the_device_saw_the_edges(device):
    """The classes of the CPU coverage test, as the device's own indices show them: lag 0 and the last fine lags, all three
    offsets, and 768 where nothing passes."""
    ds, index = device["steer"]
    kinds = [c[0] for c in F.steer_cases()]
    assert index[0, kinds.index("negative")] == 768 and np.any(ds[0, kinds.index("negative")] != 0)
    every = np.concatenate([v[1].ravel() for v in device.values()])
    assert 768 in every and int(every.min()) <= 768 - 2 * 292
    assert {int(v) & 1 for v in every} == {0, 1}  # odd indices: an interpolation offset was taken
