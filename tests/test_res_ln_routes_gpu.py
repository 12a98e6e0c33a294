"""The residual LayerNorm host layer (csrc/elementwise.hip: one grid rule, one operand check, one launcher) against the table
recorded by tools/record_res_ln_routes.py into tests/golden/res_ln_routes.json: for the smallest row counts that reach each
code path, every entry point must name the same kernel and write the same bits as when the fixture was recorded.  The
float-atomic dgamma / dbeta of mpf_res_ln256_backward, which no build reproduces bit for bit, must be the fp64 sum of the
partials within the rounding of an fp32 sum; mpf_res_ln256_backward_det must leave its ticket word zero and write the same
bits when called again on the same workspace."""
import json

import pytest
import torch

from tools.record_res_ln_routes import CASES, FIXTURE, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases_of_the_table(recorded):
    assert sorted(recorded["cases"]) == sorted(c["id"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_kernel_and_bits_as_recorded(case, recorded):
    want = recorded["cases"][case["id"]]
    got = run_case(case, torch.device("cuda:0"))
    print(case["id"], got["kernel"], got["sums"])
    assert got["kernel"] == want["kernel"]
    assert sorted(got["hashes"]) == sorted(want["hashes"])
    for name, h in got["hashes"].items():
        assert h == want["hashes"][name], f"{name} differs from the recorded bits"
    # float atomics: within blocks * 2^-24 * sum|partial| per column of the fp64 sum of the partials
    assert sorted(got["sums"]) == want["sums"]
    assert all(r <= 1.0 for r in got["sums"].values()), got["sums"]
    if case["entry"] == "det":
        assert got["ticket_after"] == 0 == want["ticket_after"]
        assert got["second_call_same_bits"] and want["second_call_same_bits"]
