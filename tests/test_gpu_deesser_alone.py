"""The de-esser ALONE on the device -- EQ, compressor, limiter and suppressor off, the input scrub as always -- in both of its
forms, on every one of the 67 streams of tests/deesser_stimulus.py and every block row, against the oracle's block processor
with the same stages off (tests/chain_oracle.py):

  stages   the stage pipeline (af_stages.hip, De0 .. De6c), which AUTO takes with the de-esser at any batch
  lane     the lane-per-stream pass (af_deesser.hip) ahead of the pinned token-ring kernel (KERNEL_PHASED, ring 16 x 4)

Both forms took the de-esser-only chain as it is; neither needed the EQ switched on.  Every test first asserts which form ran.
The cases (parameters, rates, lengths, ragged calls -- one of 1 sample, one that is no multiple of 4, 64 or the control block,
one longer than two stage windows; G's first calls end inside the 72-sample crossfade of the moved cuts) are `DS.CASES`;
tests/test_deesser_stimulus.py shows on the oracle alone which branches each of them reaches.

Tolerances are the project's for the de-esser (tests/test_gpu_deesser.py): audio max |err| <= 5e-7 and RMS <= 5e-8
per stream, the block's reduction within 1e-4 dB, `input_square_sum` within rtol 1e-12, `input_sample_peak` exact.  The de-esser
takes discrete decisions (the 0.001 dB hold, narrow_support, voice_active, ratio_conf > 0.12): a device libm result one ulp from
glibc's could flip one for a sample and show as a burst far over the tolerance.  That is no reason to widen a bound or drop a
stream: show from the oracle's per-sample trace (tests/deesser_trace.py) that a predicate sits within 1e-12 of its threshold at
the first bad sample, and only then change `DS.SEED`, saying so here.  (Not needed so far.)"""
import numpy as np
import pytest

import af_oracle_py as O
import chain_oracle as CO
import deesser_stimulus as DS
import signals as S

pytestmark = pytest.mark.gpu

MAX_ABS, MAX_RMS, ROW_DB = 5e-7, 5e-8, 1e-4
KERNEL_PHASED, KERNEL_STAGED = 2, 4
FORMS = ("stages", "lane")
CASES = list(DS.CASES)
INERT = ("F-max0", "F-ratio1")
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (case, form), (max_abs, s_abs, rms, s_rms, row, at) in sorted(REPORT.items()):
        print(f"de-esser alone {case:9s} {form:22s}: worst max abs {max_abs:.3e} (stream {s_abs}), worst rms {rms:.3e} (stream {s_rms}), "
              f"worst row difference {row:.3e} dB (block, stream {at})")


_AUDIO, _ORACLE, _DEVICE = {}, {}, {}


def _audio(case, dc=False):
    if (case, dc) not in _AUDIO:
        _AUDIO[(case, dc)] = DS.batch(case, dc=dc)
    return _AUDIO[(case, dc)]


def _oracle(case):
    """(scrubbed input, output, rows [blocks, streams]) of the oracle with only the de-esser on, once per module."""
    if case not in _ORACLE:
        fs, _, calls, settings = DS.CASES[case]
        out, rows = CO.run_batch(_audio(case), fs, S.LIMITER_BANDS, settings, calls, eq_enabled=False)
        _ORACLE[case] = (CO.sanitize(_audio(case), False), out, rows)
    return _ORACLE[case]


def _engine(fs, settings, form, eq_enabled=False):
    from mic_eq_mi import _lib
    from mic_eq_mi import mic_eq_core as core

    eng = core.Engine(float(fs), DS.N_STREAMS)
    if form == "lane":
        eng.set_kernel(_lib.KERNEL_PHASED)
        eng.set_ring_variant(16, 4)
    else:
        eng.set_kernel(_lib.KERNEL_AUTO)
        eng.set_ring_variant(0, 0)
    core.configure_auto_eq_chain(eng, float(fs), S.LIMITER_BANDS, settings)
    if not eq_enabled:
        eng.set_eq_enabled(0)
    if form == "lane" and fs > 48_000:
        # the token-ring kernel lays its LDS out for the limiter's lookahead whether the limiter is on or not, and refuses the
        # default 2 ms at 96 kHz (192 samples): 1 ms is the 96 samples it holds at 48 kHz.  The limiter stays off.
        eng.limiter_set_lookahead_ms(1.0)
    eng.set_timing_enabled(1)
    return eng


def _run(eng, audio, calls, time_major=False, device_stride_pad=None):
    """`calls` through `eng`: (output, rows [blocks, streams], (kernel, chain launches, launches) per call)."""
    outs, rows, forms = [], [], []
    at = 0
    for n in calls:
        x = audio[:, at : at + n]
        at += n
        if device_stride_pad is not None:  # device pointers through torch, rows `n + pad` apart
            import torch

            stride = n + device_stride_pad
            xin = torch.zeros((x.shape[0], stride), dtype=torch.float32, device="cuda")
            xin[:, :n] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
            yout = torch.full_like(xin, 7.0)
            eng.process_device(xin.data_ptr(), yout.data_ptr(), n, stride, 0, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert bool((yout[:, n:] == 7.0).all()), "the engine wrote between the rows"
            y = yout[:, :n].cpu().numpy()
        elif time_major:
            y = np.ascontiguousarray(eng.process(np.ascontiguousarray(x.T), 1).T)
        else:
            y = eng.process(x)
        assert y.shape == x.shape, (y.shape, x.shape)
        outs.append(y)
        rows.append(eng.block_stats().copy())
        forms.append((eng.last_kernel(), eng.last_chain_launch_ms()[2], eng.last_kernel_ms()[1]))
    return np.concatenate(outs, axis=1), np.concatenate(rows, axis=0), forms


def _assert_form(form, forms, launches_per_call=3):
    if form == "stages":  # a launch step per stage window and pipeline depth
        assert all(f[0] == KERNEL_STAGED and f[1] > 1 for f in forms), forms
    else:  # one chain span per call: the de-esser pass, the token-ring launch, the merge of the side rows
        assert all(f == (KERNEL_PHASED, 1, launches_per_call) for f in forms), forms


def _device(case, form, mode="ragged"):
    """The de-esser-only engine over the case, once per module: mode `ragged` (the case's calls), `one` (a single call),
    `time-major` or `device` (process_device, rows n + 3 apart)."""
    key = (case, form, mode)
    if key not in _DEVICE:
        fs, n, calls, settings = DS.CASES[case]
        eng = _engine(fs, settings, form)
        try:
            got = _run(eng, _audio(case), (n,) if mode == "one" else calls, time_major=mode == "time-major",
                       device_stride_pad=3 if mode == "device" else None)
        finally:
            eng.close()
        _assert_form(form, got[2])
        _DEVICE[key] = got
    return _DEVICE[key]


def _block_square_sums(x, calls, cb):
    sums, at = [], 0
    for n in calls:
        for b0 in range(at, at + n, cb):
            seg = x[:, b0 : min(b0 + cb, at + n)].astype(np.float64)
            sums.append((seg * seg).sum(axis=1))
        at += n
    return np.stack(sums)


def _compare(name, got, got_rows, want_in, want, want_rows, calls, cb, tol=(MAX_ABS, MAX_RMS), input_rows=True):
    assert got.shape == want.shape and got_rows.shape == want_rows.shape, (got.shape, want.shape, got_rows.shape, want_rows.shape)
    d = got.astype(np.float64) - want.astype(np.float64)
    max_abs = np.abs(d).max(axis=1)
    rms = np.sqrt(np.mean(d * d, axis=1))
    row = np.abs(got_rows["deesser_gain_reduction_db"].astype(np.float64) - want_rows["deesser_gain_reduction_db"].astype(np.float64))
    at = np.unravel_index(int(np.argmax(row)), row.shape)
    REPORT[name] = (float(max_abs.max()), int(np.argmax(max_abs)), float(rms.max()), int(np.argmax(rms)), float(row.max()),
                    (int(at[0]), int(at[1])))
    print(f"{name}: max abs {max_abs.max():.3e} (stream {int(np.argmax(max_abs))}), rms {rms.max():.3e} (stream {int(np.argmax(rms))}), "
          f"row {row.max():.3e} dB at {at}")
    bad = np.flatnonzero((max_abs > tol[0]) | (rms > tol[1]) | ~np.isfinite(max_abs))
    first = int(np.argmax((np.abs(d) > tol[0]).any(axis=0))) if bad.size else None
    assert bad.size == 0, f"{name}: streams {bad[:8].tolist()} exceed {tol}: max abs {max_abs.max():.3e}, rms {rms.max():.3e}, first sample {first}"
    where = np.argwhere(~(row <= ROW_DB))
    assert where.size == 0, f"{name}: the block's reduction differs by {row.max():.3e} dB; first (block, stream) {where[:4].tolist()}"
    if input_rows:
        assert np.array_equal(got_rows["input_sample_peak"], want_rows["input_sample_peak"]), name
        sums = _block_square_sums(want_in, calls, cb)
        assert np.allclose(got_rows["input_square_sum"], sums, rtol=1e-12, atol=0.0), name


def _assert_same_bits(a, b, what):
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (what, float(np.nanmax(np.abs(a[0] - b[0]))))
    assert a[1].shape == b[1].shape, what
    for field in a[1].dtype.names:
        assert a[1][field].tobytes() == b[1][field].tobytes(), (what, field)


# ------------------------------------------------------------------------------------------ 1. each form against the oracle
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES)
def test_form_against_the_oracle(case, form):
    fs, n, calls, _ = DS.CASES[case]
    want_in, want, want_rows = _oracle(case)
    got, got_rows, _ = _device(case, form)
    _compare((case, form), got, got_rows, want_in, want, want_rows, calls, DS.control_block(fs))
    roles = DS.roles()
    inert = list(range(DS.N_STREAMS)) if case in INERT else [s for s in range(DS.N_STREAMS) if case == "D" and roles[s] == "quiet"]
    if inert:  # on but inert: the oracle hands its input through bit for bit with rows of 0 -- and so does the device
        assert want[inert].tobytes() == want_in[inert].tobytes() and not want_rows["deesser_gain_reduction_db"][:, inert].any()
        assert got[inert].tobytes() == want[inert].tobytes()
        assert got_rows["deesser_gain_reduction_db"][:, inert].tobytes() == want_rows["deesser_gain_reduction_db"][:, inert].tobytes()
    elif case != "E-6":
        assert float(got_rows["deesser_gain_reduction_db"].max()) > 1.0  # the de-esser really acted


# ------------------------------------------------------------------------------------------ 2. form against form, bit for bit
@pytest.mark.parametrize("case", CASES)
def test_stages_equal_the_lane_pass_bit_for_bit(case):
    _assert_same_bits(_device(case, "stages"), _device(case, "lane"), case)


def test_lane_pass_time_major_equals_stream_major():
    _assert_same_bits(_device("B", "lane", "time-major"), _device("B", "lane"), "time-major")


@pytest.mark.parametrize("form", FORMS)
def test_device_pointers_unaligned_stride(form):
    """process_device with rows n + 3 apart gives the host path's bits; nothing is written between the rows (asserted in _run)."""
    _assert_same_bits(_device("B", form, "device"), _device("B", form), form)


# ------------------------------------------------------------------------------------------ 3. call boundaries
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", ["B", "D"])
def test_one_call_equals_ragged_calls(case, form):
    """Nothing in the de-esser's audio depends on where a call (and with it a control block) starts: the state rows survive a save
    and reload after 7001 samples, after one more, inside a block and inside a stage window."""
    one, ragged = _device(case, form, "one"), _device(case, form)
    assert np.array_equal(one[0].view(np.uint32), ragged[0].view(np.uint32)), float(np.nanmax(np.abs(one[0] - ragged[0])))


# ------------------------------------------------------------------------------------------ 4. position independence
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("case", CASES)
def test_twins_equal_their_originals(case, form):
    got, rows, _ = _device(case, form)
    for copy, original in DS.TWINS.items():
        assert got[copy].tobytes() == got[original].tobytes(), (copy, original)
        for field in rows.dtype.names:
            assert rows[field][:, copy].tobytes() == rows[field][:, original].tobytes(), (copy, original, field)


# ------------------------------------------------------------------------------------------ 5. other entries of the lane pass
_EQ_BANDS = list(S.DEFAULT_TYPED_BANDS)
_EQ_BANDS[4] = ("bell", 1280.0, 6.0, 2.0, 12, True)
_EQ_BANDS[7] = ("bell", 8000.0, 4.0, 1.41, 12, True)
_EQ_BANDS[9] = ("high_shelf", 16000.0, -3.0, 1.41, 12, True)
_B_SETTINGS = {k: v for k, v in DS.CASES["B"][3].items() if k.startswith("deesser_")}
ALIGNED_CALLS = (7_680, 960, 2_880, 12_480, 24_960)  # whole control blocks of 960 (see test_gpu_chain_forms.py: auto-makeup's loudness window)


def _compare_chain_rows(name, got_rows, want_rows):
    for field in CO.ROW_FIELDS:
        if field in ("true_peak_limited_events", "deesser_gain_reduction_db"):
            continue
        a, b = got_rows[field].astype(np.float64), want_rows[field].astype(np.float64)
        where = np.argwhere(np.abs(a - b) - 1e-4 * np.maximum(1.0, np.abs(b)) > 0.0)
        assert where.size == 0, f"{name}: row field {field} differs in {len(where)} rows, first (block, stream) {where[:4].tolist()}"


@pytest.mark.parametrize("auto_makeup", [False, True])
def test_lane_pass_behind_the_eq(auto_makeup):
    """eq_before_deesser on the pinned ring, the EQ not flat: the pass runs between the ring's pre-pass and its second launch
    (`front_end = false`), and with auto-makeup it also writes the block powers the compressor's makeup reads
    (`write_out_power`).  The whole chain is on; case B's de-esser; all 67 streams; with auto-makeup calls of whole control
    blocks."""
    fs, n, calls, _ = DS.CASES["B"]
    settings = dict(S.limiter_settings(2.0), eq_bands_v2=_EQ_BANDS, eq_before_deesser=True, **_B_SETTINGS)
    audio = _audio("B")
    if auto_makeup:
        settings.update(compressor_auto_makeup_enabled=True, compressor_target_lufs=-16.0)
        calls = ALIGNED_CALLS
        audio = audio[:, : sum(calls)]
    eng = _engine(fs, settings, "lane", eq_enabled=True)
    try:
        got, got_rows, forms = _run(eng, audio, calls)
    finally:
        eng.close()
    _assert_form("lane", forms, launches_per_call=4)  # pre-pass, de-esser pass, second ring launch, merge
    want, want_rows = CO.run_batch(audio, fs, S.LIMITER_BANDS, settings, calls)
    name = ("B", "lane behind EQ" + (" + makeup" if auto_makeup else ""))
    _compare(name, got, got_rows, CO.sanitize(audio, False), want, want_rows, calls, DS.control_block(fs))
    _compare_chain_rows(name, got_rows, want_rows)
    assert float(got_rows["deesser_gain_reduction_db"].max()) > 1.0
    if auto_makeup:
        assert float(np.abs(got_rows["compressor_makeup_gain_db"]).max()) > 1.0, "the auto-makeup gain never moved"


def test_lane_pass_owns_the_prefilter():
    """The prefilter on without the suppressor: the pass runs the DC block and the 80 Hz high-pass and owns their memories across
    the ragged calls (the `dc` role: `ess` + 0.03).  The oracle side is `prefilter` first."""
    fs, n, calls, settings = DS.CASES["B"]
    audio = _audio("B", dc=True)
    assert "dc" in DS.roles(dc=True)
    eng = _engine(fs, settings, "lane")
    eng.set_prefilter_enabled(1, 1)
    try:
        got, got_rows, forms = _run(eng, audio, calls)
    finally:
        eng.close()
    _assert_form("lane", forms)
    scrubbed = CO.sanitize(audio, False)
    filtered = np.stack([O.prefilter(scrubbed[s], float(fs)) for s in range(DS.N_STREAMS)])
    want, want_rows = CO.run_batch(filtered, fs, S.LIMITER_BANDS, settings, calls, eq_enabled=False)
    cb = DS.control_block(fs)
    _compare(("B", "lane + prefilter"), got, got_rows, scrubbed, want, want_rows, calls, cb, input_rows=False)
    # the block input statistics are taken ahead of the prefilter (routing.rs: scrub, statistics, DC block, high-pass)
    at, block_peaks = 0, []
    for m in calls:
        for b0 in range(at, at + m, cb):
            block_peaks.append(np.abs(scrubbed[:, b0 : min(b0 + cb, at + m)]).max(axis=1))
        at += m
    assert np.array_equal(got_rows["input_sample_peak"], np.stack(block_peaks))
    assert np.allclose(got_rows["input_square_sum"], _block_square_sums(scrubbed, calls, cb), rtol=1e-12, atol=0.0)
    assert float(got_rows["deesser_gain_reduction_db"].max()) > 1.0


@pytest.mark.parametrize("form", FORMS)
def test_input_clamp(form):
    """The input clamp on with the `loud` role present (and the non-finite samples of `nonfinite`): `afo_sanitize_and_clamp` first."""
    fs, n, calls, settings = DS.CASES["B"]
    audio = _audio("B")
    assert float(np.abs(audio[63]).max()) > 1.0
    eng = _engine(fs, settings, form)
    eng.set_input_clamp_enabled(1)
    try:
        got, got_rows, forms = _run(eng, audio, calls)
    finally:
        eng.close()
    _assert_form(form, forms)
    want, want_rows = CO.run_batch(audio, fs, S.LIMITER_BANDS, settings, calls, clamp=True, eq_enabled=False)
    _compare(("B", form + " + clamp"), got, got_rows, CO.sanitize(audio, True), want, want_rows, calls, DS.control_block(fs))
    assert float(got_rows["input_sample_peak"].max()) == 1.0
