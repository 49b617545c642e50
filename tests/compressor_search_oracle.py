"""Loader and driver of tests/ref/compressor_search_ref.c: the fold and the calibration search of
csrc/af_compressor_search_math.h run on the CPU, on the per-block rows of the CPU oracle's block processor."""
from __future__ import annotations

import ctypes as C
import pathlib
import subprocess

import numpy as np

from voice_spectrum_oracle import CFLAGS

HERE = pathlib.Path(__file__).resolve().parent
SRC = HERE / "ref" / "compressor_search_ref.c"
SHARED = [HERE.parent / "audio-forge_amd" / "csrc" / "af_compressor_search_math.h"]  # shared with the library
LIB = HERE / "ref" / "libcompressor_search_ref.so"
CONTROLS = ("threshold_db", "ratio", "attack_ms", "release_ms")


class Settings(C.Structure):
    _fields_ = [("compressor", C.c_double * 4), ("auto_makeup_enabled", C.c_int), ("target_lufs", C.c_double),
                ("measured_short_term_lufs", C.c_double), ("target_p95_db", C.c_double), ("target_median_db", C.c_double),
                ("peak_cap_db", C.c_double)]


class Simulation(C.Structure):
    _fields_ = [(name, C.c_double) for name in ("peak", "median", "p95", "active_ratio", "active_gain", "output_true_peak", "ceiling",
                                                "pre_limiter_headroom", "pumping", "silence_gain")] + [("non_finite", C.c_int)]


class Choice(C.Structure):
    _fields_ = [(name, C.c_int) for name in ("feasible", "best", "expanded", "threshold_only", "expanded_selected")] + [
        ("threshold_only_objective", C.c_double), ("incumbent_objective", C.c_double)]


class FoldRows(C.Structure):
    _fields_ = ([(name, C.POINTER(C.c_double)) for name in ("input_square_sum", "output_square_sum")]
                + [(name, C.POINTER(C.c_float)) for name in ("input_sample_peak", "output_sample_peak", "tp_limiter_input_peak", "output_true_peak",
                                                             "limiter_gr_db", "tp_limiter_gr_db", "compressor_gr_db", "deesser_gr_db")]
                + [(name, C.POINTER(C.c_uint32)) for name in ("tp_limited_events", "non_finite_output")])


FOLD_FLOATS = ("input_sample_peak_db", "input_rms_db", "output_sample_peak_db", "pre_limiter_true_peak_db", "output_true_peak_db",
               "output_rms_db", "limiter_effective_ceiling_db", "sample_headroom_db", "pre_limiter_true_peak_headroom_db",
               "true_peak_headroom_db", "limiter_gain_reduction_db", "true_peak_limiter_gain_reduction_db", "compressor_gain_reduction_db",
               "deesser_gain_reduction_db", "compressor_gain_reduction_median_db", "compressor_gain_reduction_p95_db",
               "compressor_gain_reduction_active_ratio", "active_output_gain_db", "silence_output_gain_db", "silence_level_delta_db",
               "compressor_pumping_score_db", "deesser_gain_reduction_median_db", "deesser_gain_reduction_p95_db",
               "active_analysis_threshold_db")
FOLD_INTS = ("true_peak_limited_events", "non_finite_output", "active_analysis_block_count", "reserved")


class FoldResult(C.Structure):
    _fields_ = [(name, C.c_float) for name in FOLD_FLOATS] + [(name, C.c_int32) for name in FOLD_INTS]


# the engine's row names behind csm_fold_rows' fields
ROW_OF_FIELD = {"input_sample_peak": "input_sample_peak", "output_sample_peak": "output_sample_peak",
                "tp_limiter_input_peak": "true_peak_limiter_input_peak", "output_true_peak": "output_true_peak",
                "limiter_gr_db": "limiter_peak_gain_reduction_db", "tp_limiter_gr_db": "true_peak_limiter_gain_reduction_db",
                "compressor_gr_db": "compressor_gain_reduction_db", "deesser_gr_db": "deesser_gain_reduction_db"}

SIMULATION_KEYS = ("compressor_gain_reduction_db", "compressor_gain_reduction_median_db", "compressor_gain_reduction_p95_db",
                   "compressor_gain_reduction_active_ratio", "active_output_gain_db", "output_true_peak_db", "limiter_effective_ceiling_db",
                   "pre_limiter_true_peak_headroom_db", "compressor_pumping_score_db", "silence_output_gain_db")


def build(force: bool = False) -> pathlib.Path:
    """Compile the restatement next to its source (git-ignored) unless it is there and newer than its sources."""
    newest = max(p.stat().st_mtime for p in [SRC, *SHARED])
    if force or not LIB.exists() or LIB.stat().st_mtime < newest:
        subprocess.run(["gcc", *CFLAGS, "-shared", "-o", str(LIB), str(SRC), "-lm"], check=True)
    return LIB


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        L = C.CDLL(str(build()))
        dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        L.csr_new.restype = C.c_void_p
        L.csr_new.argtypes = [C.POINTER(Settings)]
        L.csr_free.argtypes = [C.c_void_p]
        for name in ("csr_phase1", "csr_phase2"):
            getattr(L, name).argtypes = [C.c_void_p]
        L.csr_waiting.argtypes = [C.c_void_p, dp]
        L.csr_score.argtypes = [C.c_void_p, C.POINTER(Simulation), C.c_int]
        L.csr_choose.argtypes = [C.c_void_p, C.POINTER(Choice)]
        L.csr_entries.argtypes = [C.c_void_p, dp, dp]
        L.csr_capture_masks.argtypes = [dp, C.c_int, C.c_int64, C.c_int, fp, C.POINTER(C.c_uint8), fp]
        L.csr_pumping_alphas.argtypes = [C.c_float, fp, fp]
        L.csr_fold.argtypes = [C.POINTER(FoldRows), C.c_int, C.c_int64, C.c_int, C.c_float, C.POINTER(FoldResult)]
        L.csr_round6.restype = C.c_double
        L.csr_round6.argtypes = [C.c_double]
        _LIB = L
    return _LIB


def capture_masks(input_square_sum, n_samples: int, control_block: int) -> dict:
    sq = np.ascontiguousarray(input_square_sum, dtype=np.float64)
    in_db, mask, threshold = np.zeros(sq.size, dtype=np.float32), np.zeros(sq.size, dtype=np.uint8), C.c_float(0.0)
    active = lib().csr_capture_masks(sq.ctypes.data_as(C.POINTER(C.c_double)), sq.size, n_samples, control_block,
                                     in_db.ctypes.data_as(C.POINTER(C.c_float)), mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(threshold))
    return {"in_db": in_db, "active": (mask & 1) != 0, "audible": (mask & 2) != 0, "active_threshold_db": np.float32(threshold.value),
            "active_count": active}


def oracle_rows(audio: np.ndarray, sample_rate: float, bands, settings: dict) -> dict:
    """One capture through the CPU oracle's block processor, configured as simulate_auto_eq_chain configures it: the per-block
    rows, with the two square sums accumulated sample by sample in f64 around each block (python_api.rs:515-553)."""
    import chain_oracle

    chain = chain_oracle.make_chain(sample_rate, bands, settings)
    y = chain_oracle.sanitize(audio, False)
    cb = chain_oracle.control_block(sample_rate)
    n = -(-y.size // cb)
    rows = {name: np.zeros(n, dtype=np.float64) for name in ("input_square_sum", "output_square_sum")}
    rows.update({name: np.zeros(n, dtype=np.float32) for name in ROW_OF_FIELD})
    rows.update({name: np.zeros(n, dtype=np.uint32) for name in ("tp_limited_events", "non_finite_output")})
    for i in range(n):
        block = y[i * cb : (i + 1) * cb]
        rows["input_square_sum"][i] = np.cumsum(np.square(block.astype(np.float64)))[-1]  # (cumsum: left to right)
        rows["input_sample_peak"][i] = np.max(np.abs(block))
        st = chain.process_block(block)
        finite = np.isfinite(block)
        rows["output_square_sum"][i] = np.cumsum(np.square(np.where(finite, block, 0.0).astype(np.float64)))[-1]
        rows["non_finite_output"][i] = 0 if finite.all() else 1
        for field, name in ROW_OF_FIELD.items():
            if field != "input_sample_peak":
                rows[field][i] = getattr(st, name)
        rows["tp_limited_events"][i] = st.true_peak_limited_events
    rows["n_samples"] = y.size
    rows["control_block"] = cb
    return rows


def fold(rows: dict, ceiling_db: float = -1.5) -> dict:
    """csm_fold on rows as oracle_rows returns them: the reference's result dict (its numeric keys)."""
    arguments = FoldRows(*[rows[name].ctypes.data_as(kind) for name, kind in FoldRows._fields_])
    out = FoldResult()
    rc = lib().csr_fold(C.byref(arguments), rows["input_square_sum"].size, rows["n_samples"], rows["control_block"], ceiling_db, C.byref(out))
    assert rc == 0
    d = {name: float(getattr(out, name)) for name in FOLD_FLOATS}
    d.update({name: int(getattr(out, name)) for name in FOLD_INTS if name != "reserved"})
    d["non_finite_output"] = bool(d["non_finite_output"])
    d["processed_samples"] = int(rows["n_samples"])
    return d


def run_search(compressor: dict, targets, simulate) -> dict:
    """The search for one capture.  ``simulate(values [n, 4]) -> list of result dicts`` (the reference's keys) stands for the
    chain simulations: the search's fixed limiter, auto-makeup off."""
    L = lib()
    st = Settings((C.c_double * 4)(*[float(compressor[k]) for k in CONTROLS]), int(bool(compressor.get("auto_makeup_enabled", False))),
                  float(compressor.get("target_lufs", -18.0)), float(compressor.get("measured_short_term_lufs", -18.0)),
                  float(targets[0]), float(targets[1]), float(targets[2]))
    h = C.c_void_p(L.csr_new(C.byref(st)))
    sims: list = []
    try:
        for phase in (L.csr_phase1, L.csr_phase2):
            if phase(h) <= 0:
                continue
            values = np.zeros((67, 4))
            n = L.csr_waiting(h, values.ctypes.data_as(C.POINTER(C.c_double)))
            results = simulate(values[:n])
            sims.extend(results)
            arr = (Simulation * n)()
            for i, r in enumerate(results):
                arr[i] = Simulation(*[float(r[k]) for k in SIMULATION_KEYS], int(bool(r["non_finite_output"])))
            L.csr_score(h, arr, n)
        choice = Choice()
        L.csr_choose(h, C.byref(choice))
        values, scores = np.zeros((67, 4)), np.zeros(67)
        n = L.csr_entries(h, values.ctypes.data_as(C.POINTER(C.c_double)), scores.ctypes.data_as(C.POINTER(C.c_double)))
    finally:
        L.csr_free(h)
    return {"evaluated": values[:n].copy(), "scores": scores[:n].copy(), "simulations": sims, "feasible": bool(choice.feasible),
            "winner": choice.best if choice.feasible else -1, "expanded": choice.expanded, "threshold_only": choice.threshold_only,
            "expanded_selected": bool(choice.expanded_selected), "threshold_only_objective": choice.threshold_only_objective,
            "incumbent_objective": choice.incumbent_objective}
