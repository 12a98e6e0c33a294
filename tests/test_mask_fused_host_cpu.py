"""The pure-host answers of the fused mask product host layer (csrc/mask_fused_host.h and the entry points of csrc/mask_fused.hip)
against the table recorded by tools/record_mask_fused_host.py into tests/golden/mask_fused_host.json: the three workspace size
queries over every single and pairwise variation of a typical call (zeros, negatives, the sizes at which tiles_per_wg, KS, mgroups
and KP change, large values short of where `int` geometry overflowed) and, for the four launching entries, the status code and the
mpf_last_error text of every single argument fault that is rejected before any HIP call — sizes, codes and texts exactly.  Needs no
GPU: the pointers are made-up addresses that nothing dereferences, and a case that got as far as the runtime would come back with
a non-negative status, which the recorder's own check rejects.  The tables also agree with the mirrors of
tests/_mask_fused_cases.py and tests/_mask_fused_clip_cases.py wherever a mirror applies."""
import json

import pytest

import _mask_fused_cases as MC
import _mask_fused_clip_cases as KC
from tools.record_mask_fused_host import ENTRIES, FIXTURE, QUERIES, faults, workspace_sizes


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    from mp_former_amd import _lib
    return _lib.lib()


def _differences(got, want):
    assert sorted(got) == sorted(want)
    return {k: (v, want[k]) for k, v in got.items() if v != want[k]}


def test_workspace_sizes_as_recorded(lib, recorded):
    got = workspace_sizes(lib)
    assert sorted(got) == sorted(QUERIES) == sorted(recorded["workspace"])
    for query, table in got.items():
        wrong = _differences(table, recorded["workspace"][query])
        assert not wrong, (query, wrong)
        assert any(v == 0 for v in table.values()) and any(v > 0 for v in table.values())


def test_the_recorded_sizes_are_the_mirrors(recorded):
    mirror = {"mpf_match_cost_fused_workspace_bytes": MC.mc_workspace_bytes, "mpf_match_cost_fused_clip_workspace_bytes": KC.clip_workspace_bytes,
              "mpf_pair_planes_backward_workspace_bytes": MC.pb_workspace_bytes}
    for query, table in recorded["workspace"].items():
        for key, want in table.items():
            args = {k: int(v) for k, v in (kv.split("=") for kv in key.split())}
            assert mirror[query](**args) % 2 ** 64 == want, (query, key)


def test_single_faults_give_the_recorded_code_and_text(lib, recorded):
    got = faults(lib)
    assert {k.split(":")[0] for k in got} == set(ENTRIES) and len(ENTRIES) == 4
    wrong = _differences({k: list(v) for k, v in got.items()}, recorded["faults"])
    assert not wrong, wrong
    assert all(code < 0 for code, _ in got.values())                 # the library's own codes: nothing reached the runtime
