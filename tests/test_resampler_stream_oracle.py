"""The streaming helper (tests/resampler_stream_oracle.py) held to the pinned one-shot oracle: driving
`afo_resampler_process_chunk` through the realtime loop's queue gives the first blocks of `simulate_product_resampler`
exactly, whatever the partition of the input into calls.  CPU only."""
import numpy as np
import pytest

import resampler_stream_oracle as RS

RATES = [(44_100, 48_000), (48_000, 44_100), (16_000, 48_000), (48_000, 16_000)]


def _signal(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(n) * 0.25).astype(np.float32)


@pytest.mark.parametrize("fi,fo", RATES)
def test_whole_chunks_equal_the_one_shot_oracles_first_blocks(oracle, fi, fo):
    k = 5
    x = _signal(k * 1024, fi ^ fo)
    o = RS.StreamOracle(fi, fo)
    got = o.push_f64(x)
    assert o.pending_input == 0
    want, delay, expected, blocks = oracle.simulate_product_resampler(x.astype(np.float64), fi, fo)
    assert blocks >= k and 0 < got.size <= want.size
    assert np.array_equal(got, want[: got.size])  # f64, exact: the same routine on the same chunks
    # the k blocks are all of what the one-shot driver made from the input itself: the rest is its flush
    assert want.size - got.size >= delay
    o.close()


@pytest.mark.parametrize("fi,fo", RATES)
def test_any_partition_gives_the_same_concatenation(fi, fo):
    n = 6 * 1024 + 300
    x = _signal(n, 3 * fi + fo)
    whole = RS.run_calls(x, [n], fi, fo)[0]
    partitions = [
        [1, 479, 1023, 1024, 1025, n - (1 + 479 + 1023 + 1024 + 1025)],
        [1025, 1024, 1023, 479, 1] + [441] * 4 + [n - (1025 + 1024 + 1023 + 479 + 1 + 4 * 441)],
        [1] * 7 + [n - 7],
    ]
    for calls in partitions:
        assert sum(calls) == n and min(calls) > 0
        outs = RS.run_calls(x, calls, fi, fo)
        got = np.concatenate(outs)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), whole.view(np.uint32)), calls
        assert any(o.size == 0 for o in outs)  # some wake-ups complete no chunk


def test_reset_and_clear_pending():
    x = _signal(3000, 11)
    o = RS.StreamOracle(44_100, 48_000)
    first = o.push(x[:1500])
    assert o.pending_input == 1500 - 1024
    o.clear_pending()  # the queue goes, history and position stay: the next chunk continues from the first one's state
    assert o.pending_input == 0
    after = o.push(x[1500:2524])
    ref = RS.run_calls(np.concatenate([x[:1024], x[1500:2524]]), [1024, 1024], 44_100, 48_000)
    assert np.array_equal(first, ref[0]) and np.array_equal(after, ref[1])
    o.reset()
    again = o.push(x[:1500])
    assert np.array_equal(again, first) and o.pending_input == 476
    o.close()
