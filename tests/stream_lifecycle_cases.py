"""Engine configurations, stimulus and the blob layout shared by the stream-lifecycle tests (tests/test_abi_stream_lifecycle.py on
the CPU, tests/test_gpu_stream_lifecycle.py on the GPU).  Not a test module.

The layout below restates DESIGN.md 4.24 / csrc/af_stream_state.h in Python on purpose: the tests check the library against the
document, not against its own header."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np

import live_control_cases as LC

FS = 48_000
BLOCK = 960
CALL = 4800          # 4800 % 97 = 47, 4800 % 21 = 12: the limiter's phase is never 0 after the first call
N_STREAMS = 130      # two full 64-stream groups and a two-stream tail
SHORT_LOOKAHEAD_MS = 20.0 / 48.0  # 20 samples: W = 21

MAGIC, VERSION, HEADER_BYTES = 0x53534641, 1, 72
HEADER = struct.Struct("<IIIIdiiiiIiiiiiq")
HEADER_FIELDS = ("magic", "version", "header_bytes", "blob_bytes", "sample_rate", "control_block", "n_eq_sections", "lookahead",
                 "meter_slots", "stage_flags", "suppressor", "gate_plane", "live_rows", "rows64", "rows32", "samples")
SHAPE_FIELDS = HEADER_FIELDS[5:15]
F64_FIXED, F32_FIXED, GATE_WORDS, SUPP_FLOATS = 93, 68, 11, 2580
FLAG_DEESSER, FLAG_EQ, FLAG_COMP, FLAG_LIM, FLAG_SCRUB, FLAG_AUTO_MAKEUP = 1, 2, 4, 8, 32, 1 << 16
assert HEADER.size == HEADER_BYTES


def rows64(n_eq_sections: int, meter_slots: int, live: bool = False) -> int:
    return F64_FIXED + 4 * n_eq_sections + ((5 + meter_slots) if meter_slots else 0) + (15 if live else 0)


def blob_bytes(n_rows64: int, ring_capacity: int, gate: bool, suppressor: bool) -> int:
    b = HEADER_BYTES + 8 * (n_rows64 + (GATE_WORDS if gate else 0)) + 4 * (F32_FIXED + ring_capacity) + (4 * SUPP_FLOATS if suppressor else 0)
    return (b + 7) // 8 * 8


def header_of(blob: bytes) -> dict:
    return dict(zip(HEADER_FIELDS, HEADER.unpack_from(blob)))


def with_header(blob: bytes, **changes) -> bytes:
    h = header_of(blob)
    h.update(changes)
    return HEADER.pack(*(h[f] for f in HEADER_FIELDS)) + blob[HEADER_BYTES:]


# ---- configurations ---------------------------------------------------------------------------------------------------------
def _dynamics(eng, core, lookahead_ms):
    core.configure_auto_eq_chain(eng, float(FS), LC.BANDS, dict(LC.SETTINGS, limiter_lookahead_ms=lookahead_ms))


def _deesser_makeup(eng, core, lookahead_ms):
    _dynamics(eng, core, lookahead_ms)
    eng.set_deesser_enabled(1)
    for name, args in LC.DEESSER_SETTERS:
        # The cut setters schedule a coefficient crossfade that a FRESH engine plays in its first 72 samples (the reference's
        # Biquad does the same before its first sample).  Its counters belong to the preset, so a restarted stream starts from
        # the configured target instead -- the reference's reset() -- and would not equal a fresh engine there: default cuts.
        if name not in ("deesser_set_low_cut_hz", "deesser_set_high_cut_hz"):
            getattr(eng, name)(*args)
    eng.compressor_set_auto_makeup_enabled(1)
    eng.compressor_set_adaptive_release(1)


def _preset_variant(eng, core, lookahead_ms, k):
    """Three presets that differ in parameter values and, for k = 2, in the compressor's release mode."""
    _dynamics(eng, core, lookahead_ms)
    if k == 1:
        eng.compressor_set_threshold(-26.0)
        eng.eq_set_band_gain(3, 4.0)
    if k == 2:
        eng.compressor_set_ratio(2.5)
        eng.compressor_set_adaptive_release(1)
        eng.limiter_set_release_time(80.0)
    # An EQ setter schedules a 72-sample crossfade, which a fresh engine plays from its first sample (flat -> +4 dB in preset
    # 1; tests/signals.py's bands are flat, so elsewhere it is inaudible).  A restarted stream starts from the configured
    # target, like the reference's reset(); eq_reset makes the fresh engine start there too.
    eng.eq_reset()


CONFIGS = ("dynamics", "suppressor-gate", "deesser-makeup", "presets")


def engine(config: str, n_streams: int = N_STREAMS, lookahead_ms: float = 2.0, group_presets=None, lifecycle: bool = True,
           live: bool = False):
    """A configured engine, not started.  `group_presets` (config "presets"): the preset of each 64-stream group."""
    from mic_eq_mi import mic_eq_core as core

    eng = core.Engine(float(FS), n_streams)
    if config == "presets":
        eng.set_preset_count(3)
        for k in range(3):
            eng.select_preset(k)
            _preset_variant(eng, core, lookahead_ms, k)
        groups = (n_streams + 63) // 64
        gp = np.asarray(group_presets if group_presets is not None else [g % 3 for g in range(groups)], dtype=np.int32)
        assert gp.size == groups
        core._lib.check(eng._lib.af_engine_assign_presets(eng._h, gp.ctypes.data_as(C.POINTER(C.c_int32)), groups))
    elif config == "deesser-makeup":
        _deesser_makeup(eng, core, lookahead_ms)
    else:
        _dynamics(eng, core, lookahead_ms)
        if config == "suppressor-gate":
            eng.set_suppressor_enabled(1)
            eng.set_gate_enabled(1)  # threshold mode is the default
    if live:
        eng.set_live_control(True)
    eng.set_stream_lifecycle(lifecycle)
    return eng


def audio(n_streams: int, n: int) -> np.ndarray:
    """[n_streams, n] float32: the loud per-stream voices of tests/live_control_cases.py (limiter busy in every block)."""
    return LC.audio(n_streams, n)
