"""The MSDA host layer (csrc/msda_entry.hip: one problem record, one check, one route choice per direction) against the table
recorded by tools/record_msda_routes.py into tests/golden/msda_routes.json: on the smallest problems that reach each route, every
entry point must name the same kernels, log the same profiler records and byte counts, count the same routes and write the same
bits as when the fixture was recorded.  Outputs that no build reproduces bit for bit (float-atomic sums, runs summed in arrival
order, the spill) must meet the library's own generic<double> result under the bounds of tests/test_msda_gpu.py; an amax slot
must bound its tensor within one fp32 rounding."""
import json

import pytest
import torch

from tools.record_msda_routes import CASES, FIXTURE, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases_of_the_table(recorded):
    assert sorted(recorded["cases"]) == sorted(c["id"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_kernels_records_and_bits_as_recorded(case, recorded):
    want = recorded["cases"][case["id"]]
    got = run_case(case, torch.device("cuda:0"), hashed=sorted(want["hashes"]))
    print(case["id"], got["kernels"], got["prof"], got["stats"], got["bounds"], got["amax"])
    assert got["kernels"] == want["kernels"]
    assert got["prof"] == want["prof"]
    for name, count in want["stats"].items():
        assert got["stats"][name] == count, f"route counter {name}"
    for name, h in want["hashes"].items():
        assert got["hashes"][name] == h, f"{name} differs from the recorded bits"
    # against generic<double> on the same inputs: |got - ref| / (atol + rtol |ref|) <= 1
    assert sorted(got["bounds"]) == want["bounds"]
    assert all(r <= 1.0 for r in got["bounds"].values()), got["bounds"]
    assert got["amax"] == want["amax"]          # "tight": slot >= max |tensor|, within one fp32 rounding; else the recorded bits
    for flag in ("all_nan", "second_call_same_bits", "gap_rows_zero", "spill_entries_positive"):
        assert (flag in got) == (flag in want)
        if flag in want:
            assert got[flag] and want[flag], flag
    assert got.get("geometry_ok") == want.get("geometry_ok")
    if case.get("layout") == "overlap":
        assert got["geometry_ok"] == 0
