"""af_dsp.h's device math against mpmath at 45 digits, on the GPU (tests/device_math_probe.hip, built with the library's
flags into libaf_device_math_probe.so): the claims the gated pre-pass's F1 step and the chain rest on.

* `div_known(x, 20, 0.05)` is bit-identical to `x / 20.0`;
* `fast_log10_pos` is within 2 ulp (log-uniform x in [1e-10, 1e10], x near 1, near sqrt(1/2) 2^k and 2^k, the floor);
* `exp10`, as db2lin calls it (on div_known(dB, 20, 0.05) for dB in [-200, 40]), is within EXP10_BOUND_ULPS: the device
  library's exp10 is not faithfully rounded everywhere (measured worst 1.02 ulp, af_dsp.h);
* F1's gain, db2lin(-clamp((thr - lin2db(sqrt(g), 1e-10)) 0.75, 0, 36)), is within F1_BOUND_ULPS of the same f64 steps
  with correctly rounded log10 and 10^x.

Each case prints its worst error and the input where it occurs."""
import ctypes as C
import multiprocessing
import pathlib
import subprocess

import numpy as np
import pytest

import device_math_ref as R

pytestmark = pytest.mark.gpu

ROOT = pathlib.Path(__file__).resolve().parents[1]
PROBE = ROOT / "audio-forge_amd" / "libaf_device_math_probe.so"
LOG10, EXP10, DIV_KNOWN, DB2LIN, F1, F1_LEVEL = range(6)
# F1's bound: fast_log10_pos's 2 ulp on log10(sqrt g) (|value| < 8 over the thresholds' range: 2 ulp <= 2^-49), times 20
# and 0.75, plus a differently rounded 20 * log10 (1 ulp of the level, <= 2^-46) and a differently rounded d and d / 20,
# moves 10^(-d / 20) by ln(10) / 20 * 0.75 * (20 * 2^-49 + 2^-46 + ...) ~ 4.5e-15 relative, ~20 ulp; and exp10's 1 ulp.
F1_BOUND_ULPS = 32.0
EXP10_BOUND_ULPS = 1.05
SEED = 20261016


@pytest.fixture(scope="module")
def probe():
    if not PROBE.exists():
        subprocess.run(["make", "-C", str(ROOT / "audio-forge_amd" / "csrc"), "ARCH=gfx950", "../libaf_device_math_probe.so"],
                       check=True)
    import mic_eq_mi  # (the HIP runtime the library loads: torch's, when torch went first)

    assert mic_eq_mi.CORE_AVAILABLE
    lib = C.CDLL(str(PROBE))
    lib.af_probe_eval.restype = C.c_int
    lib.af_probe_eval.argtypes = [C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int64, C.c_double]

    def run(fn, x, thr=0.0):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty_like(x)
        rc = lib.af_probe_eval(fn, x.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double)),
                               x.size, float(thr))
        assert rc == 0, f"probe failed: hipError {rc}"
        return out

    return run


@pytest.fixture(scope="module")
def pool():
    # a fresh interpreter per worker (spawn, not fork: nothing of this process's GPU state is inherited)
    with multiprocessing.get_context("spawn").Pool(8) as p:
        yield p


def _parallel(pool, fn, *arrays, parts=64):
    chunks = list(zip(*(np.array_split(a, parts) for a in arrays)))
    return pool.map(fn, chunks)


def _near(x, ulps):
    """Every x and its neighbours up to `ulps` steps either way."""
    x = np.asarray(x, dtype=np.float64)
    out = [x]
    up, down = x.copy(), x.copy()
    for _ in range(ulps):
        up, down = np.nextafter(up, np.inf), np.nextafter(down, -np.inf)
        out += [up, down]
    return np.concatenate(out)


def _log10_inputs():
    rng = np.random.default_rng(SEED)
    k = np.arange(-34, 35, dtype=np.float64)
    return np.concatenate([
        10.0 ** rng.uniform(-10.0, 10.0, 700_000),       # log-uniform over [1e-10, 1e10]
        rng.uniform(0.5, 2.0, 200_000),                  # the reduction's whole range around 1
        _near([1.0], 256),                               # log10 ~ 0: the relative error is what counts
        _near(np.sqrt(0.5) * 2.0 ** k, 32),              # the m < sqrt(1/2) edge, every exponent
        _near(2.0 ** k, 32),                             # powers of two
        _near([1e-10, 1e10], 64),                        # the floor the callers clamp to, and the top
    ])


def _report(name, err, x):
    i = int(np.argmax(err))
    print(f"device math {name}: {err.size} inputs, worst {err[i]:.3f} ulp at x = {x[i]!r}")
    return float(err[i])


def test_div_known_is_the_correctly_rounded_quotient(probe):
    rng = np.random.default_rng(SEED + 1)
    db = np.concatenate([rng.uniform(-200.0, 40.0, 800_000), np.arange(-200.0, 40.25, 0.25),
                         rng.choice([-1.0, 1.0], 200_000) * 10.0 ** rng.uniform(-10.0, 10.0, 200_000), _near([-24.0, -36.0, 0.0], 16)])
    got = probe(DIV_KNOWN, db)
    want = db / 20.0
    differ = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    print(f"device math div_known(x, 20, 0.05): {db.size} inputs, {differ.size} differ from x / 20")
    assert differ.size == 0, f"div_known(x, 20, 0.05) != x / 20 at x = {db[differ[:4]].tolist()}"


def test_fast_log10_pos_within_2_ulp(probe, pool):
    x = _log10_inputs()
    got = probe(LOG10, x)
    err = np.concatenate(_parallel(pool, R.log10_ulps, x, got))
    worst = _report("fast_log10_pos", err, x)
    assert worst <= 2.0, f"fast_log10_pos is {worst:.3f} ulp off (af_dsp.h claims < 2)"


def test_exp10_in_db2lin_within_its_bound(probe, pool):
    rng = np.random.default_rng(SEED + 2)
    db = np.concatenate([rng.uniform(-200.0, 40.0, 900_000), np.arange(-200.0, 40.0 + 1e-9, 0.01)])
    y = probe(DIV_KNOWN, db)                           # what db2lin hands to exp10
    got = probe(EXP10, y)
    assert np.array_equal(probe(DB2LIN, db).view(np.uint64), got.view(np.uint64))  # db2lin is exactly that composition
    err = np.concatenate(_parallel(pool, R.exp10_ulps, y, got))
    worst = _report("exp10 in db2lin", err, y)
    assert worst <= EXP10_BOUND_ULPS, f"exp10 is {worst:.3f} ulp off"


@pytest.mark.parametrize("thr", [-80.0, -60.0, -40.0, -20.0, -10.0])
def test_f1_gain_within_its_bound(probe, pool, thr):
    """The threshold's whole range (the setter clamps to [-80, -10]); levels from 52 dB under it (d = 36 from 48 dB on) to
    6 over, the 1e-10 floor, and the decision edges (thr, thr - 4, d = 24, d = 36) a few ulp either way."""
    rng = np.random.default_rng(SEED + int(-thr))
    edges = 10.0 ** (np.array([thr, thr - 4.0, thr - 32.0, thr - 48.0]) / 10.0)
    g = np.concatenate([10.0 ** (rng.uniform(thr - 52.0, thr + 6.0, 50_000) / 10.0), _near(edges, 64), [0.0, 1e-20, 1e-21]])
    got = probe(F1, g, thr)
    chunks = _parallel(pool, R.f1_reference, g, np.full(g.size, thr))
    want = np.concatenate([c[1] for c in chunks])
    err = np.abs(got - want) / np.spacing(np.abs(want))
    worst = _report(f"F1 gain (thr {thr:g})", err, g)
    assert worst <= F1_BOUND_ULPS, f"F1 gain is {worst:.3f} ulp off at threshold {thr}"
    # the level the gate's decisions read agrees with the correctly rounded one except within a few ulp of it
    level = probe(F1_LEVEL, g)
    want_level = np.concatenate([c[0] for c in chunks])
    assert np.all(np.abs(level - want_level) <= 4.0 * np.spacing(np.abs(want_level)))
