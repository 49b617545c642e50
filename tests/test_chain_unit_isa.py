"""Static checks of the token-ring chain kernel's serial units (tools/chain_unit_isa.py): no GPU, skipped without hipcc."""
import json
import os
import pathlib
import shutil
import subprocess
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")


@pytest.fixture(scope="module")
def report():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "chain_unit_isa.py"), "--kernel", "16,4,false", "--json"],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_every_unit_is_marked(report):
    names = {u["unit"] for u in report["units"]}
    for unit in ("input", "eq-group", "sidechain(A)", "peak-envelope(C)", "gain-smoothing(E)", "limiter", "true-peak",
                 "final-fold"):
        assert unit in names, f"{unit} not found in the listing"


def test_no_global_loads_inside_serial_units(report):
    # a load from the parameter block at a per-lane address inside a unit is an L2 round trip while the token is held
    for u in report["units"]:
        assert u["global_load"] == 0, u


def test_peak_envelope_unit_has_no_spill_reloads(report):
    for u in report["units"]:
        if u["unit"] == "peak-envelope(C)":
            assert u["scratch_load"] == 0 and u["readlane"] == 0, u


def test_spills_below_the_previous_build(report):
    usage = report["resource_usage"]
    assert int(usage["VGPRs"]) <= 128  # sixteen waves per workgroup
    assert int(usage["VGPRs Spill"]) < 62  # the build before the units were shortened: 62 VGPRs, 101 SGPRs spilled
    assert int(usage["SGPRs Spill"]) <= 101
