"""The attention host layer (csrc/attn_host.h: one problem record, one check, one split launcher, one prep launcher) against the
table recorded by tools/record_attn_routes.py into tests/golden/attn_routes.json: on the smallest problems that reach each host
decision — operands that ask for the aligned and for the unaligned forms, attn_occ 4 and 2, every mask kind, 1, 3 and 10 workgroup
splits, the strided, aux, transpose and delta entry points — every entry point must name the same kernels, log the same profiler
records and byte counts and write the same bits as when the fixture was recorded.  All forms of a kernel carry one label and
write equal bits wherever more than one of them is valid, so WHICH form ran is not observable here (only an aligned form on
Lk % 8 != 0 would show, in the bits); the choice between valid forms is checked by reading launch_split.  The strided and aux
routes must also write the bits of the dense route on the same values (EQUAL), and the columns between the halves of a packed
dK / dV buffer keep their prefill."""
import json

import pytest
import torch

from tools.record_attn_routes import CASES, EQUAL, FIXTURE, FLAGS, run_case, unequal

pytestmark = pytest.mark.gpu

_results = {}


def _result(case, recorded):
    if case["id"] not in _results:
        _results[case["id"]] = run_case(case, torch.device("cuda:0"), hashed=sorted(recorded["cases"][case["id"]]["hashes"]))
    return _results[case["id"]]


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases_of_the_table(recorded):
    assert sorted(recorded["cases"]) == sorted(c["id"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_kernels_records_and_bits_as_recorded(case, recorded):
    want = recorded["cases"][case["id"]]
    got = _result(case, recorded)
    print(case["id"], got["kernels"], got["prof"])
    assert got["kernels"] == want["kernels"]
    assert got["prof"] == want["prof"]
    assert want["hashes"]
    for name, h in want["hashes"].items():
        assert got["hashes"][name] == h, f"{name} differs from the recorded bits"
    for flag in FLAGS:
        assert (flag in got) == (flag in want)
        if flag in want:
            assert got[flag] and want[flag], flag


def test_strided_and_aux_routes_write_the_bits_of_the_dense_route(recorded):
    assert not unequal(recorded["cases"])
    by_id = {c["id"]: c for c in CASES}
    needed = {i for x, y, _ in EQUAL for i in (x, y)}
    got = {i: _result(by_id[i], recorded) for i in sorted(needed)}
    assert not unequal(got)
