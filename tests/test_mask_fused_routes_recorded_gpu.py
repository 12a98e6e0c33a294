"""The fused mask product host layer (csrc/mask_fused_host.h: one problem record, one check, one launcher per kernel) against the
table recorded by tools/record_mask_fused_routes.py into tests/golden/mask_fused_routes.json: on the smallest problems that reach
each host decision — all seven chunk widths of the cost kernel at Tmax = 2 TCH and 2 TCH + 1, image and clip form, 127 / 128 / 129
queries, one to three tiles per workgroup, a group without targets, runs of tiles that cross a frame boundary, forward planes of
2 x 2 and 8 x 16 pixels, the pair backward at KS 1 / 2 / 16 / 64 and one to three slot groups with d_embed bf16 and fp32 and each
gradient NULL in turn — every entry point must name the same kernel, log the same profiler records with the same bytes and flops
and write the same bits, into every output buffer and the whole workspace, as when the fixture was recorded.  Every cost case makes
its call twice in this process: the first and a later launch of one kernel instantiation.  All kernels of the family are
fixed-order without atomics, so everything is compared exactly."""
import json

import pytest
import torch

from tools.record_mask_fused_routes import CASES, FIXTURE, geometry, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases_of_the_table(recorded):
    assert sorted(recorded["cases"]) == sorted(CASES)


def test_the_cases_reach_the_host_decisions_they_name():
    geo = {cid: geometry(c) for cid, c in CASES.items()}
    for kind in ("cost", "clip"):
        assert {g["TCH"] for cid, g in geo.items() if CASES[cid]["kind"] == kind and "Tmax" in cid} == {4, 8, 12, 16, 24, 32, 64}
    assert {g["TCH"] for cid, g in geo.items() if "Tmax" in cid and int(cid.split("=")[1]) % 2} == {8, 12, 16, 24, 32, 64}
    assert {g["tiles_per_wg"] for cid, g in geo.items() if CASES[cid]["kind"] == "cost"} == {1, 2, 3}
    assert {CASES[cid]["F"] for cid in geo if CASES[cid]["kind"] == "clip"} == {1, 2, 3} and geo["clip F=3 crossing"]["crossing"] > 0
    assert any(0 in CASES[cid]["counts"] for cid in geo if CASES[cid]["kind"] == "cost")
    assert {g["KS"] for g in geo.values() if "KS" in g} >= {1, 64} and {g["mgroups"] for g in geo.values() if "KS" in g} >= {1, 3}


@pytest.mark.parametrize("cid", list(CASES))
def test_kernels_records_and_bits_as_recorded(cid, recorded):
    want = recorded["cases"][cid]
    got = run_case(CASES[cid], torch.device("cuda:0"))
    print(cid, got["kernels"], got["prof"])
    assert got["kernels"] == want["kernels"]
    assert got["prof"] == want["prof"]
    assert sorted(got["hashes"]) == sorted(want["hashes"])
    for name, h in want["hashes"].items():
        assert got["hashes"][name] == h, f"{name} differs from the recorded bits"
    if CASES[cid]["kind"] in ("cost", "clip"):
        assert got["hashes"]["0.cost"] == got["hashes"]["1.cost"] and got["hashes"]["0.workspace"] == got["hashes"]["1.workspace"]
