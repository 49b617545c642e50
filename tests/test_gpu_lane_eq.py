"""The per-lane EQ (csrc/af_lane_eq.hip) on the GPU: the ten captures of tests/headroom_stimulus.py x the seven gain scales,
70 lanes = one wave and six lanes, the zero-gain lanes (scale 0.0, and every scale of capture 5) among them.

Every lane's output equals, bit for bit, the compressor input compressor_input_batch returns for the lane's capture with the
lane's bands: an engine run with nothing but the EQ.  The same holds for rows of 1, 63, 64, 65, 71, 72, 73 and 1 293 samples (a
tile is 64 samples, the crossfade 72: its end inside, at and after a tile edge; 1 293 = 20 tiles and 13), for device input,
and a lane's output does not depend on its neighbours (the batch reversed, in two unequal halves, a reused handle)."""
import numpy as np
import pytest

import headroom_stimulus as HS

pytestmark = pytest.mark.gpu

SHORT_LANES = (0, 6, 15, 24, 38, 69)  # lane = 7 capture + scale index: captures 0 (scales 1.0 and 0.0), 2, 3, 5 (zero gains), 9 (scale 0.0)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


class Lanes:
    def __init__(self):
        import mic_eq_mi
        from mic_eq_mi import headroom as H

        self.mi = mic_eq_mi
        self.audio = HS.captures()
        self.lane_capture = np.repeat(np.arange(HS.N_CAPTURES, dtype=np.int32), len(HS.SCALES))
        self.bands = [H._scaled_bands(H._bands_from_settings(HS.eq_settings(c)), scale) for c in range(HS.N_CAPTURES) for scale in HS.SCALES]
        self.eq = mic_eq_mi.LaneEq(float(HS.FS))
        self.eq.run(self.audio, self.lane_capture, self.bands)
        self.out = self.eq.output()

    def engine(self, lanes, n=HS.N):
        """The compressor input of an EQ-only engine per lane."""
        audio = np.ascontiguousarray(self.audio[self.lane_capture[list(lanes)], :n])
        return self.mi.compressor_input_batch(audio, HS.FS, [self.bands[l] for l in lanes], [{} for _ in lanes])[0]


@pytest.fixture(scope="module")
def lanes():
    s = Lanes()
    yield s
    s.eq.close()


def test_every_lane_equals_an_eq_only_engine_run(lanes):
    assert lanes.out.shape == (70, HS.N) and len(lanes.bands) % 64 == 6
    want = lanes.engine(range(70))
    for lane in range(70):
        assert same_bits(lanes.out[lane], want[lane]), (lane, int(np.flatnonzero(lanes.out[lane] != want[lane])[0]))
    zero = [l for l in range(70) if all(g == 0.0 for _, g, _ in lanes.bands[l])]
    assert len(zero) == 10 + 6  # scale 0.0 of every capture, and the other six scales of capture 5
    assert not same_bits(lanes.out[0], lanes.out[1]) and not same_bits(lanes.out[0], lanes.audio[0])  # the scales differ; the EQ works
    pointer, stride = lanes.eq.device_output()
    assert pointer % 256 == 0 and stride >= HS.N and stride % 64 == 0 and lanes.eq.last_kernel_ms() > 0.0


@pytest.mark.parametrize("n", (1, 63, 64, 65, 71, 72, 73, 1293))
def test_row_lengths_around_tile_and_crossfade_edges(lanes, n):
    picked = list(SHORT_LANES)
    eq = lanes.mi.LaneEq(float(HS.FS))
    try:
        eq.run(lanes.audio[:, :n], lanes.lane_capture[picked], [lanes.bands[l] for l in picked])
        got = eq.output()
    finally:
        eq.close()
    want = lanes.engine(picked, n)
    assert got.shape == (len(picked), n)
    for k, lane in enumerate(picked):
        assert same_bits(got[k], want[k]), (n, lane)
        assert same_bits(got[k], lanes.out[lane, :n]), (n, lane)  # causal: the prefix of the long row


def test_a_lanes_output_does_not_depend_on_its_neighbours(lanes):
    eq = lanes.eq
    order = np.arange(70)[::-1]
    eq.run(lanes.audio, lanes.lane_capture[order], [lanes.bands[l] for l in order])
    assert same_bits(eq.output()[::-1], lanes.out)
    for lo, hi in ((0, 41), (41, 70)):
        eq.run(lanes.audio, lanes.lane_capture[lo:hi], lanes.bands[lo:hi])
        assert same_bits(eq.output(), lanes.out[lo:hi]), (lo, hi)
    eq.run(lanes.audio, lanes.lane_capture, lanes.bands)  # a reused handle, and the full batch after smaller ones
    assert same_bits(eq.output(), lanes.out)


def test_device_input_with_a_stride_and_non_finite_samples(lanes):
    import torch

    stride = HS.N + 37
    host = np.zeros((HS.N_CAPTURES, stride), dtype=np.float32)
    host[:, :HS.N] = lanes.audio
    host[:, HS.N:] = 7.0  # beyond the rows: never read
    d_audio = torch.from_numpy(host).cuda()
    eq = lanes.mi.LaneEq(float(HS.FS))
    try:
        eq.run_device(d_audio.data_ptr(), HS.N, HS.N_CAPTURES, stride, lanes.lane_capture, lanes.bands)
        assert same_bits(eq.output(), lanes.out)
        # the engine zeroes a non-finite input sample (python_api.rs:517-520), so the lane EQ does
        dirty = lanes.audio[:1, :200].copy()
        dirty[0, [3, 70, 150]] = [np.nan, np.inf, -np.inf]
        clean = np.where(np.isfinite(dirty), dirty, np.float32(0.0)).astype(np.float32)
        eq.run(dirty, [0], [lanes.bands[0]])
        got = eq.output()
        eq.run(clean, [0], [lanes.bands[0]])
        assert same_bits(got, eq.output()) and np.isfinite(got).all()
    finally:
        eq.close()
