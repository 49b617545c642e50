"""Argument contract of the compressor candidate sweep's entry points (include/audioforge_mi.h, "compressor candidate sweep"):
everything here is refused before any HIP call, so no GPU is needed."""
import pathlib
import re

import numpy as np
import pytest

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "audioforge_mi.h"


@pytest.fixture(scope="module")
def cs():
    import mic_eq_mi
    from mic_eq_mi import compressor_search

    assert mic_eq_mi.CORE_AVAILABLE
    return compressor_search


def test_every_entry_point_is_declared_bound_and_cites_the_reference(cs):
    from mic_eq_mi import _lib

    text = HEADER.read_text()
    section = text[text.index("compressor candidate sweep"):text.index("NoiseSuppressor: rust-core")]
    names = set(re.findall(r"\b(af_compressor_search_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", section, flags=re.S)))
    assert {"af_compressor_search_create", "af_compressor_search_destroy", "af_compressor_search_set_limiter", "af_compressor_search_load_host",
            "af_compressor_search_load_device", "af_compressor_search_sweep", "af_compressor_search_run"} <= names
    L = _lib.load()
    for name in names:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None, name
    assert "voice_setup.py:742-1079" in section and "python_api.rs:649-712" in section


def test_structures_match_the_header(cs):
    import ctypes as C

    from mic_eq_mi import _lib

    assert C.sizeof(_lib.ChainSimulation) == 144 and cs.SIMULATION_DTYPE.itemsize == 144
    assert C.sizeof(_lib.CompressorCandidate) == 40 and C.sizeof(_lib.CompressorBase) == 24
    assert C.sizeof(_lib.CompressorSearchSettings) == 6 * 8 + 4 * 4 + 5 * 8
    assert C.sizeof(_lib.CompressorSearchResult) == 8 * 4 + 17 * 8 + 67 * 4 * 8 + 67 * 8


def test_refusals_before_any_device_work(cs):
    with pytest.raises(ValueError, match="sample_rate"):
        cs.CompressorSearch(0.0)
    with pytest.raises(ValueError, match="sample_rate"):
        cs.CompressorSearch(float("nan"))
    search = cs.CompressorSearch(48_000.0)
    try:
        with pytest.raises(RuntimeError, match="no captures are loaded"):
            search.n_captures = 1
            search.sweep([(0, -20.0, 4.0, 5.0, 100.0)], [(0.0, 50.0, False, True)])
        search.n_captures = 0
        with pytest.raises(RuntimeError, match="no captures are loaded"):
            search.run([])
        with pytest.raises(ValueError, match="limiter settings must be finite"):
            search.set_limiter(float("inf"))
        from mic_eq_mi import mic_eq_core as core

        blocks = cs.MAX_BLOCKS + 1
        with pytest.raises(NotImplementedError, match="control blocks per capture"):
            search.load(np.zeros((1, blocks * 960), dtype=np.float32), np.zeros((blocks, 1), dtype=core.STATS_DTYPE))
        bad = np.zeros((1, 2000), dtype=np.float32)
        bad[0, 7] = np.nan
        with pytest.raises(ValueError, match="finite"):
            search.load(bad, np.zeros((3, 1), dtype=core.STATS_DTYPE))
        with pytest.raises(ValueError, match="rows per capture"):
            search.load(np.zeros((1, 2000), dtype=np.float32), np.zeros((2, 1), dtype=core.STATS_DTYPE))
    finally:
        search.close()


def test_operator_refusals(cs):
    import signals as S

    audio = np.zeros((2, 960), dtype=np.float32)
    settings = S.limiter_settings(2.0)
    with pytest.raises(NotImplementedError, match="auto-makeup"):
        cs.simulate_compressor_candidates_batch(audio, 48_000, S.LIMITER_BANDS, dict(settings, compressor_auto_makeup_enabled=True), [])
    with pytest.raises(ValueError, match="limiter settings must be the same"):
        cs.simulate_compressor_candidates_batch(audio, 48_000, S.LIMITER_BANDS, [settings, dict(settings, limiter_release_ms=60.0)], [])
    with pytest.raises(ValueError, match="10 frequencies"):
        cs.calibrate_compressor_batch(audio, 48_000, {"band_freqs": [100.0]}, {}, {"threshold_db": -20.0, "ratio": 2.0, "attack_ms": 5.0,
                                                                                    "release_ms": 100.0}, 3.5, 1.5, 8.0)
