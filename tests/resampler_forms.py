"""The case table of the resampler's launch forms, shared by tests/test_resampler_forms.py (CPU: every row reaches the form
it names, the lengths hit the tails they are there for) and the two GPU files (bit-exact against the oracle on every row).
Helper for the tests, not a test.

A job runs one of seven forms with either I/O policy (one-shot f64, streaming f32): the matrix-core body with 64 or 32
streams per workgroup, or the vector body with segments of 128, 64, 32, 16 or 8 outputs.  The `form` column is what
`Resampler.launch_form` / `StreamResampler.launch_form` must return: (0 vector | 1 matrix-core, outputs per workgroup,
streams per workgroup).  It is written down here, not computed, so that a change of the dispatch rule shows up as a failing
row and not as silently lost coverage.

Input lengths come from {0, 1, 1024, 2048, 3589} (1025 at most for 8 -> 48 kHz, which makes six frames per input frame);
which tail each one gives is asserted by the CPU test against the oracle's frame count.
"""
from __future__ import annotations

import contextlib
import os
from dataclasses import dataclass

MATRIX, VECTOR = 1, 0
VARIANT_ENV = "AF_RESAMPLER_VARIANT"
N_STREAMS = 67  # two workgroups of 64 in y (the second with 3 live streams), three of 32 for mfma32

# the existing partition of tests/test_gpu_resampler_stream.py and a second one of the same total
CALLS = [100, 441, 3000, 1, 1023, 1024, 1025, 479, 2000, 7, 1100]
OTHER_PARTITION = [3000, 1024, 1, 1, 2500, 441, 441, 441, 441, sum(CALLS) - (3000 + 1024 + 2 + 2500 + 4 * 441)]
# chunks of 40 / 160 frames: several calls complete no chunk, and the split between the carried plane and the call's input
# lands somewhere else in a tile on every call
SMALL_CALLS = [7, 40, 39, 41, 1, 160, 500, 3]
SMALL_OTHER = [160, 1, 1, 300, 41, sum(SMALL_CALLS) - (160 + 1 + 1 + 300 + 41)]
# 8 -> 48 kHz makes 6144 frames per chunk: two chunks (completed by one call) keep the case near 12 k output frames
UP6_CALLS = [100, 441, 2000, 1, 7]
UP6_OTHER = [1, 1023, 1024, sum(UP6_CALLS) - 2048]


@dataclass(frozen=True)
class Row:
    fi: int
    fo: int
    sinc_len: int
    variant: str | None      # value of AF_RESAMPLER_VARIANT around the constructor (None: unset)
    form: tuple              # (body, outputs per workgroup, streams per workgroup)
    window: str
    lengths: tuple           # one-shot input lengths
    why: str
    chunk: int = 1024
    calls: tuple | None = None   # stream test: the partition to push (None: the row's form is reached by the file's older tests)
    other: tuple | None = None   # the same frames under another partition

    @property
    def id(self) -> str:
        tail = "" if self.chunk == 1024 else f"-chunk{self.chunk}"
        return f"{self.fi}-{self.fo}-sinc{self.sinc_len}{tail}" + (f"-{self.variant}" if self.variant else "")

    @property
    def body(self) -> int:
        return self.form[0]


_C, _O = tuple(CALLS), tuple(OTHER_PARTITION)
_S, _SO = tuple(SMALL_CALLS), tuple(SMALL_OTHER)

ROWS = (
    Row(44_100, 48_000, 128, None, (MATRIX, 128, 64), "blackman", (1, 1024, 2048), "the product default"),
    Row(44_100, 48_000, 128, "mfma32", (MATRIX, 128, 32), "blackman_harris", (0, 1024, 2048),
        "32 streams per workgroup: three workgroups in y at 67 streams", calls=_C, other=_O),
    Row(44_100, 48_000, 128, "valu", (VECTOR, 128, 64), "blackman_squared", (1, 1024, 3589),
        "the <16,8> vector kernel, forced", calls=_C, other=_O),
    Row(48_000, 40_000, 128, None, (VECTOR, 128, 64), "hann", (1024, 2048, 3589),
        "the <16,8> vector kernel, reached without the switch", calls=_C, other=_O),
    Row(50_000, 44_100, 128, None, (MATRIX, 128, 64), "hann_squared", (1, 1024, 2048),
        "ceil(128 / ratio) + sinc_len + 14 == 288: the tile fills every LDS row", calls=_C, other=_O),
    Row(48_000, 28_800, 32, None, (MATRIX, 128, 64), "blackman_harris_squared", (0, 1024, 3589),
        "3 / ratio + 3 == 8: the widest window spread inside a tile", calls=_C, other=_O),
    Row(8_000, 48_000, 128, None, (MATRIX, 128, 64), "blackman", (1, 1024),
        "six outputs per window: every delta inside a tile is 0", calls=tuple(UP6_CALLS), other=tuple(UP6_OTHER)),
    Row(16_000, 48_000, 128, None, (MATRIX, 128, 64), "blackman_harris", (1024, 3589), "the voice rate of the engine test"),
    Row(8_000, 48_000, 256, None, (VECTOR, 128, 64), "blackman_harris_squared", (0, 1025),
        "the matrix-core tile is refused by four rows", calls=tuple(UP6_CALLS), other=tuple(UP6_OTHER)),
    Row(96_000, 48_000, 128, None, (VECTOR, 64, 64), "blackman_squared", (1, 2048, 3589), "the <16,4> vector kernel"),
    Row(48_000, 16_000, 128, None, (VECTOR, 32, 64), "hann", (1024, 2048, 3589), "the <16,2> vector kernel"),
    Row(48_000, 9_600, 128, None, (VECTOR, 16, 64), "hann_squared", (1024, 2048, 3589),
        "1 / ratio == 5: a pair's second window starts 4 to 6 frames after the first", calls=_C, other=_O),
    Row(48_000, 44_100, 256, None, (VECTOR, 16, 64), "blackman_harris_squared", (1, 1024, 2048), "the <8,2> vector kernel on a batch"),
    Row(96_000, 48_000, 256, None, (VECTOR, 8, 64), "blackman", (0, 1024, 3589), "the <4,2> vector kernel", calls=_C, other=_O),
    Row(44_100, 48_000, 32, None, (MATRIX, 128, 64), "hann", (1, 1024, 3589),
        "a whole job shorter than one segment (n = 1); plane_stride 103", chunk=40, calls=_S, other=_SO),
    Row(44_100, 48_000, 64, None, (MATRIX, 128, 64), "blackman_squared", (1, 2048, 3589),
        "many chunk boundaries; a last segment of one output (n = 3589); plane_stride 287", chunk=160, calls=_S, other=_SO),
    # no further form: the vector body's last segment of a single output, and the two ratios the GPU files ran before the table
    Row(44_100, 48_000, 64, "valu", (VECTOR, 128, 64), "hann_squared", (1, 3589),
        "the vector body with a last segment of one output (n = 3589)", chunk=160),
    Row(48_000, 44_100, 128, None, (MATRIX, 128, 64), "blackman", (1024, 3589), "the product default downwards; n_out = 1 mod 4"),
    Row(32_000, 48_000, 128, None, (MATRIX, 128, 64), "blackman", (1, 3589), "ratio 1.5"),
)

REFUSED = (48_000, 8_000)  # 1 / ratio == 6: beyond the row padding of a vector pair; both classes raise at construction

ALL_FORMS = {(MATRIX, 128, 64), (MATRIX, 128, 32), (VECTOR, 128, 64), (VECTOR, 64, 64), (VECTOR, 32, 64), (VECTOR, 16, 64),
             (VECTOR, 8, 64)}
ALL_WINDOWS = {"blackman_harris", "blackman_harris_squared", "blackman", "blackman_squared", "hann", "hann_squared"}
LENGTHS = {0, 1, 1024, 1025, 2048, 3589}


@contextlib.contextmanager
def variant_env(variant: str | None):
    """AF_RESAMPLER_VARIANT as the row wants it (the library reads it when a resampler is created), restored afterwards."""
    previous = os.environ.get(VARIANT_ENV)
    if variant is None:
        os.environ.pop(VARIANT_ENV, None)
    else:
        os.environ[VARIANT_ENV] = variant
    try:
        yield
    finally:
        if previous is None:
            os.environ.pop(VARIANT_ENV, None)
        else:
            os.environ[VARIANT_ENV] = previous


def make_resampler(core, row: Row):
    with variant_env(row.variant):
        return core.Resampler(row.fi, row.fo, row.chunk, row.sinc_len, row.window)


def make_stream_resampler(core, row: Row, n_streams: int = N_STREAMS):
    with variant_env(row.variant):
        return core.StreamResampler(row.fi, row.fo, n_streams=n_streams, chunk_size=row.chunk, sinc_len=row.sinc_len, window=row.window)
