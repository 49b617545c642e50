"""CPU checks of the resampler case table (tests/resampler_forms.py): every row reaches the launch form it names, for the
one-shot and the streaming object, the table reaches all seven forms with both, and the input lengths give the output tails
the GPU tests rely on.  The form is read from the library (`launch_form`, the launcher's own choice), the frame counts from
`Resampler.plan` and, independently, from the oracle's chunk loop.  No GPU is touched."""
import math

import numpy as np
import pytest

import resampler_forms as F


@pytest.fixture(scope="module")
def core():
    import mic_eq_mi
    from mic_eq_mi import mic_eq_core

    assert mic_eq_mi.CORE_AVAILABLE, "build the library first: python -c 'import __graft_entry__ as g; g.build()'"
    return mic_eq_core


@pytest.fixture(scope="module")
def frames(core, oracle):
    """{(row id, n): n_out}, from the host plan, each confirmed by the oracle's own chunk loop"""
    table = {}
    for row in F.ROWS:
        r = F.make_resampler(core, row)
        for n in row.lengths:
            n_out, blocks = r.plan(n)
            y, _, _, b = oracle.simulate_product_resampler(np.zeros(n), row.fi, row.fo, row.chunk, row.sinc_len, row.window)
            assert (n_out, blocks) == (y.size, b), (row.id, n)
            table[row.id, n] = n_out
        r.close()
    return table


@pytest.mark.parametrize("row", F.ROWS, ids=lambda r: r.id)
def test_row_reaches_its_form(core, row):
    import os

    before = os.environ.get(F.VARIANT_ENV)
    r = F.make_resampler(core, row)
    s = F.make_stream_resampler(core, row)
    assert os.environ.get(F.VARIANT_ENV) == before  # the override does not leak
    assert r.launch_form == row.form, (row.id, row.why)
    assert s.launch_form == row.form, (row.id, row.why)
    assert r.launch_form == row.form  # a read-out, not a state change
    r.close()
    s.close()


def test_table_reaches_every_form_with_both_objects(core):
    one_shot, stream = set(), set()
    for row in F.ROWS:
        r, s = F.make_resampler(core, row), F.make_stream_resampler(core, row)
        one_shot.add(r.launch_form)
        stream.add(s.launch_form)
        r.close()
        s.close()
    assert one_shot == F.ALL_FORMS and stream == F.ALL_FORMS
    # the stream file pushes audio through every form as well: its older tests reach (matrix 64) and the vector segments of
    # 64, 32 and 16 outputs at chunk 1024; the rows with `calls` add the rest
    assert {row.form for row in F.ROWS if row.calls} | {(1, 128, 64), (0, 64, 64), (0, 32, 64), (0, 16, 64)} == F.ALL_FORMS
    assert {row.window for row in F.ROWS} == F.ALL_WINDOWS
    assert len({row.id for row in F.ROWS}) == len(F.ROWS)


def test_the_variant_switch_is_read_at_create_only(core):
    row = F.ROWS[0]
    with F.variant_env("valu"):
        r = F.make_resampler(core, row)  # the row's own (unset) value wins inside
        forced = core.Resampler(row.fi, row.fo)
    assert r.launch_form == (F.MATRIX, 128, 64) and forced.launch_form == (F.VECTOR, 128, 64)
    with F.variant_env("mfma32"):
        assert forced.launch_form == (F.VECTOR, 128, 64)
    # the switch never turns a shape the matrix-core tile cannot hold into a matrix-core launch
    with F.variant_env("mfma32"):
        v = core.Resampler(96_000, 48_000)
    assert v.launch_form == (F.VECTOR, 64, 64)
    for x in (r, forced, v):
        x.close()


def test_refused_ratio_raises_in_both_classes(core):
    fi, fo = F.REFUSED
    with F.variant_env(None):
        with pytest.raises(NotImplementedError, match="LDS tile"):
            core.Resampler(fi, fo)
        with pytest.raises(NotImplementedError, match="LDS tile"):
            core.StreamResampler(fi, fo, n_streams=F.N_STREAMS)


def test_geometry_edges_of_the_rows():
    """The rows that are there for an edge of the tile geometry sit exactly on it."""
    by_id = {row.id: row for row in F.ROWS}
    full = by_id["50000-44100-sinc128"]
    assert math.ceil(128.0 / (full.fo / full.fi)) + full.sinc_len + 14 == 288
    spread = by_id["48000-28800-sinc32"]
    assert 3.0 / (spread.fo / spread.fi) + 3.0 == 8.0
    pair = by_id["48000-9600-sinc128"]
    assert 1.0 / (pair.fo / pair.fi) == 5.0
    assert 1.0 / (F.REFUSED[1] / F.REFUSED[0]) > 5.0
    for row in F.ROWS:  # plane_stride of the stream object
        if row.chunk != 1024:
            assert 2 * row.sinc_len + row.chunk - 1 in (103, 287)


def test_lengths_hit_the_tails(frames):
    matrix = {n_out % 4 for (rid, n), n_out in frames.items() if _row(rid).body == F.MATRIX}
    assert matrix == {0, 1, 2, 3}, "a matrix-core tile takes four outputs: every partial last tile"
    for streams in (64, 32):
        got = {n_out % 4 for (rid, n), n_out in frames.items() if _row(rid).form == (F.MATRIX, 128, streams)}
        assert {0, 2, 3} <= got, streams
    vector = {n_out % 2 for (rid, n), n_out in frames.items() if _row(rid).body == F.VECTOR}
    assert vector == {0, 1}, "the vector body takes outputs in pairs: with and without an odd last one"
    for body in (F.MATRIX, F.VECTOR):  # a last segment of a single output
        assert any(n_out % 128 == 1 for (rid, n), n_out in frames.items() if _row(rid).form[:2] == (body, 128)), body
    assert frames["44100-48000-sinc64-chunk160", 3589] == 3969
    assert frames["44100-48000-sinc32-chunk40", 1] == 24  # a whole job shorter than one segment
    assert frames["44100-48000-sinc128", 1] == 1043 and frames["44100-48000-sinc128", 1024] == 2158
    assert frames["44100-48000-sinc128", 2048] == 3272 and frames["48000-44100-sinc128", 1024] == 1821
    assert frames["48000-40000-sinc128", 1024] == 1651
    # more than one segment and a ragged last one, per row
    for row in F.ROWS:
        seg = row.form[1]
        assert any(frames[row.id, n] > seg and frames[row.id, n] % seg for n in row.lengths), row.id
        assert 2 <= len(row.lengths) <= 3 and set(row.lengths) <= F.LENGTHS, row.id
        assert max(frames[row.id, n] for n in row.lengths) <= 12_500, row.id  # a few seconds per GPU case, oracle included
        if (row.fi, row.fo) == (8_000, 48_000):
            assert max(row.lengths) <= 1025
    assert any(0 in row.lengths for row in F.ROWS), "a pure flush"


def test_stream_partitions(core):
    """Per row with a partition: some calls complete no chunk and some do, the second partition covers the same frames, and
    the case stays near 12 k output frames."""
    for row in F.ROWS:
        if row.calls is None:
            continue
        assert sum(row.calls) == sum(row.other), row.id
        s = F.make_stream_resampler(core, row)
        made = sum(row.calls) // row.chunk * s.output_frames(row.chunk)  # (close enough for a size bound)
        assert made <= 12_500, (row.id, made)
        assert min(row.calls) < row.chunk <= max(row.calls), row.id
        s.close()


def test_oracle_keeps_subnormals(oracle):
    """The CPU side of the GPU tests' subnormal row: the oracle's build flushes nothing to zero, its outputs for samples of
    1e-308 are non-zero subnormals."""
    y = oracle.simulate_product_resampler(np.full(3000, 1e-308), 44_100, 48_000)[0]
    mid = y[500:2500]
    assert np.all(mid != 0.0) and np.all(np.abs(mid) < np.finfo(np.float64).tiny)


def _row(rid):
    return next(row for row in F.ROWS if row.id == rid)
