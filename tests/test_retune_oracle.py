"""The CPU side of the live-control comparisons (tests/retune_oracle.py) against what the oracle can state exactly: without a
schedule it IS tests/chain_oracle.py; a retune changes nothing before the call it is scheduled for; setters scheduled for a
call that processes nothing land at the next one; and the shared stimulus keeps the compressor and both limiters working in
every block, so a silent chain cannot pass the GPU comparisons.

The oracle offers no band change with the crossfade suppressed (`afo_eq_reset` commits every band's target but also clears
every filter memory), so "equal from the end of the crossfade on" has no exact statement here and is left out."""
import numpy as np

import chain_oracle as CO
import live_control_cases as LC
import retune_oracle as RO

STREAMS = 3


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_empty_schedule_is_the_chain_oracle():
    audio = LC.audio(STREAMS)
    for s in range(STREAMS):
        want, want_rows = CO.run_calls(audio[s], LC.FS, LC.BANDS, LC.SETTINGS, LC.CALLS)
        got, got_rows = RO.run_calls(audio[s], LC.FS, LC.BANDS, LC.SETTINGS, LC.CALLS, {})
        assert np.array_equal(_bits(got), _bits(want))
        for field in CO.ROW_FIELDS:
            assert got_rows[field].tobytes() == want_rows[field].tobytes(), field
    batch, batch_rows = RO.run_batch(audio, LC.FS, LC.BANDS, LC.SETTINGS, LC.CALLS)
    assert np.array_equal(_bits(batch[STREAMS - 1]), _bits(got)) and batch_rows.shape == (len(got_rows), STREAMS)


def test_a_band_change_is_heard_from_its_call_on_only():
    audio = LC.audio(STREAMS)
    base, base_rows = RO.run_batch(audio, LC.FS, LC.BANDS, LC.SETTINGS, LC.CALLS)
    for call in (1, 3):
        first = sum(LC.CALLS[:call])
        got, rows = RO.run_batch(audio, LC.FS, LC.BANDS, LC.SETTINGS, LC.CALLS, {call: [("eq_set_band_gain", (3, 6.0))]})
        assert np.array_equal(_bits(got[:, :first]), _bits(base[:, :first]))
        assert (got[:, first:] != base[:, first:]).any(axis=1).all()
        blocks_before = sum(-(-n // CO.control_block(LC.FS)) for n in LC.CALLS[:call])
        assert rows[:blocks_before].tobytes() == base_rows[:blocks_before].tobytes()


def test_setters_of_a_call_without_samples_wait_for_the_next():
    audio = LC.audio(1)[0]
    calls = (960, 0, 50, 0, 30)
    sched = {1: [("eq_set_band_gain", (3, 6.0))], 3: [("compressor_set_threshold", (-16.0,))]}
    moved = {2: sched[1], 4: sched[3]}
    a, rows_a = RO.run_calls(audio, LC.FS, LC.BANDS, LC.SETTINGS, calls, sched)
    b, rows_b = RO.run_calls(audio, LC.FS, LC.BANDS, LC.SETTINGS, calls, moved)
    assert np.array_equal(_bits(a), _bits(b)) and rows_a.tobytes() == rows_b.tobytes()


def test_the_schedule_reaches_every_stage_and_the_stimulus_is_loud():
    audio = LC.audio(67)
    got, rows = RO.run_batch(audio, LC.FS, LC.BANDS, LC.SETTINGS, LC.CALLS, LC.SCHEDULE)
    LC.assert_loud(rows)
    # every scheduled group of setters changes the output from its call on, and not before
    for call in sorted(LC.SCHEDULE):
        upto = {k: v for k, v in LC.SCHEDULE.items() if k < call}
        without, _ = RO.run_batch(audio[:4], LC.FS, LC.BANDS, LC.SETTINGS, LC.CALLS, upto)
        with_it, _ = RO.run_batch(audio[:4], LC.FS, LC.BANDS, LC.SETTINGS, LC.CALLS, {**upto, call: LC.SCHEDULE[call]})
        first = sum(LC.CALLS[:call])
        assert np.array_equal(_bits(with_it[:, :first]), _bits(without[:, :first])), call
        assert (with_it[:, first:] != without[:, first:]).any(axis=1).all(), call


def test_deesser_configuration_and_retune():
    deesser = {"eq_first": False, "setters": LC.DEESSER_SETTERS}
    audio = LC.audio(2, skip=LC.SIBILANT_SKIP)
    base, base_rows = RO.run_batch(audio, LC.FS, LC.BANDS, LC.SETTINGS, LC.CALLS, None, deesser=deesser)
    assert float(base_rows["deesser_gain_reduction_db"].min()) > 0.5  # the de-esser acts on this stimulus in every block
    sched = LC.merged(LC.DEESSER_SCALARS, LC.DEESSER_CUTS)
    got, _ = RO.run_batch(audio, LC.FS, LC.BANDS, LC.SETTINGS, LC.CALLS, sched, deesser=deesser)
    first = sum(LC.CALLS[:min(sched)])
    assert np.array_equal(_bits(got[:, :first]), _bits(base[:, :first]))
    assert (got[:, first:] != base[:, first:]).any(axis=1).all()
