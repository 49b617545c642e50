"""The suppressor's pre-pass (supp_prefilter_kernel) on its own: the model-input buffer it leaves, bit for bit.

af_suppressor_debug_read_model_input copies one stream's row of the LAST window's model-input buffer to the host: the 1728
history samples the pre-pass put in front, then the window's.  66 streams (a full 64-stream group and a group of two, whose
other rows are clamped), rows of streams 0, 63, 64 and 65 read after each of four calls on one engine at control block 480:

    1 frame     one window, history from the zeroed state
    4 frames    one window, history from the state the call before saved
    12 frames   one window (a window holds up to 16 frames at this control block), the same
    20 frames   two windows, 16 + 4: the tapped one takes its history from the previous window's BUFFER -- asserted to have
                happened by the tapped row being shorter than the call

Input (tests/prepass_ref.py): gains up to 2.6 that drive the soft clip far beyond +-1, DC offsets, a silent stream, and on the
clamped variants one NaN, one +inf and one -inf.  Variants: all eight instantiations of the kernel, i.e. the input clamp, the
DC block + high-pass and the raw protocol each on and off.  Expected values come from the oracle alone (afo_sanitize_and_clamp,
oracle.prefilter, oracle.scale_sample_for_model / raw_model_input, the model's high-pass restated in numpy float32), with
state carried over the whole timeline.  Rows are compared BIT FOR BIT.

The dry copy's own store path has no tap: with strength 0.6 it is audible in the output, which is compared with
oracle.suppressor_process(front_end(x), 0.6, seed) for every stream at the budget of test_gpu_suppressor.py (RMS and worst
sample <= 1e-5; an addressing error is orders of magnitude above that).
"""
import numpy as np
import pytest

import prepass_ref as P

pytestmark = pytest.mark.gpu

SEED = 0x5EED


def _engine(name: str, strength: float = 1.0):
    import mic_eq_mi

    assert mic_eq_mi.CORE_AVAILABLE
    clamp, dc_hp, raw = P.VARIANTS[name]
    eng = mic_eq_mi.Engine(48_000.0, P.N_STREAMS)
    eng.set_eq_enabled(0)
    eng.set_compressor_enabled(0)
    eng.set_limiter_enabled(0)
    eng.set_input_clamp_enabled(int(clamp))
    eng.set_prefilter_enabled(int(dc_hp), int(dc_hp))
    eng.set_suppressor_enabled(1)
    eng.set_suppressor_strength(strength)
    eng.suppressor_set_raw_protocol(int(raw))
    eng.suppressor_set_synthetic_weights(SEED)
    eng.set_control_block_samples(480)
    return eng


def _bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(P.VARIANTS))
def test_model_input_rows_bit_for_bit(name, oracle):
    want = P.expected_rows(name, oracle)
    x = P.stimulus(P.VARIANTS[name][0])
    eng = _engine(name)
    try:
        with pytest.raises(Exception):  # AF_ERR_STATE: no window has run
            eng.suppressor_debug_read_model_input(0)
        f0 = 0
        for n in P.CALLS:
            out = eng.process(x[:, f0 * 480:(f0 + n) * 480])
            assert out.shape == (P.N_STREAMS, n * 480)
            f0 += n
            for i, s in enumerate(P.READ):
                row = eng.suppressor_debug_read_model_input(s)
                frames, rest = divmod(row.size - P.HISTORY, 480)
                assert rest == 0 and 1 <= frames <= n, (name, n, s, row.size)
                if n <= 16:
                    assert frames == n, (name, n, s, frames)
                else:  # the tapped window is not the call's first: its history came from the previous window's buffer
                    assert frames < n, (name, n, s, frames)
                end = P.HISTORY + f0 * 480  # the window is the call's last `frames` frames
                ref = want[i, end - row.size:end]
                diff = np.flatnonzero(_bits(row) != _bits(ref))
                print(f"{name}: call of {n} frames, stream {s}: window of {frames} frames, {diff.size} of {row.size} words differ")
                assert diff.size == 0, (name, n, s, int(diff[0]), float(row[diff[0]]), float(ref[diff[0]]))
        with pytest.raises(Exception):  # out of range
            eng.suppressor_debug_read_model_input(P.N_STREAMS)
    finally:
        eng.close()
    assert np.abs(want[P.READ.index(P.SILENT)]).max() == 0.0  # (the silent stream stayed silent)


def test_dry_copy_through_the_wet_dry_mix(oracle):
    name, strength = "clamp-dc-hp", 0.6
    clamp, dc_hp, _ = P.VARIANTS[name]
    x = P.stimulus(clamp)
    eng = _engine(name, strength)
    try:
        f0, outs = 0, []
        for n in P.CALLS:
            outs.append(eng.process(x[:, f0 * 480:(f0 + n) * 480]))
            f0 += n
    finally:
        eng.close()
    got = np.concatenate(outs, axis=1)
    want = np.stack([oracle.suppressor_process(P.front_end(x[s], clamp, dc_hp, oracle), strength, SEED) for s in range(P.N_STREAMS)])
    assert got.shape == want.shape and np.all(np.isfinite(got))
    d = got.astype(np.float64) - want.astype(np.float64)
    rms = np.sqrt(np.mean(d * d, axis=1))
    worst = np.abs(d).max(axis=1)
    print(f"dry copy at strength {strength}: worst stream RMS {rms.max():.3e} (stream {int(rms.argmax())}), "
          f"worst sample {worst.max():.3e} (stream {int(worst.argmax())})")
    assert float(rms.max()) <= 1e-5, (int(rms.argmax()), float(rms.max()))
    assert float(worst.max()) <= 1e-5, (int(worst.argmax()), float(worst.max()))
