"""The gemm3 host layer (csrc/gemm3.hip: fill the parameter struct, choose a route, launch) against the route table recorded
by tools/record_gemm3_routes.py into tests/golden/gemm3_routes.json: for the smallest shapes on each side of each routing
threshold, every entry point must log the same algorithmic bytes and flops and write the same bits as when the fixture was
recorded (the per-split column sums, which no build reproduces bit for bit, must be the exact sums within fp32 rounding);
where the device has the recorded number of CUs it must also pick the same kernel (the thresholds count CUs, and
test_gemm3_gpu.py establishes that the routes are bit-identical to each other)."""
import json

import pytest
import torch

from tools.record_gemm3_routes import CASES, DEVICE_DEPENDENT, FIXTURE, cu_count, route_ok, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases_of_the_table(recorded):
    assert sorted(recorded["cases"]) == sorted(c["id"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_route_bytes_flops_and_bits_as_recorded(case, recorded):
    dev = torch.device("cuda:0")
    want = recorded["cases"][case["id"]]
    got = run_case(case, dev)            # (restores every option it sets in a finally)
    same_chip = cu_count(dev) == recorded["cu_count"]
    print(case["id"], got["kernel"], got["bytes"], got["flops"])
    assert got["records"] == want["records"] == 1
    assert got["bytes"] == want["bytes"] and got["flops"] == want["flops"], (got, want)
    assert sorted(got["hashes"]) == sorted(want["hashes"])
    for name, h in got["hashes"].items():
        if same_chip or name not in DEVICE_DEPENDENT:
            assert h == want["hashes"][name], f"{name} differs from the recorded bits (kernel {got['kernel']}, recorded {want['kernel']})"
    # column sums: float atomics in LDS, not reproducible bit for bit -> within the rounding of an fp32 sum of the exact ones
    assert sorted(got["sums"]) == want["sums"]
    assert all(r <= 1.0 for r in got["sums"].values()), got["sums"]
    if same_chip:
        assert got["kernel"] == want["kernel"]
        assert route_ok(case, got["kernel"]) is None, route_ok(case, got["kernel"])
