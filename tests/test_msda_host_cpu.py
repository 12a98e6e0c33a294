"""The pure-host answers of the MSDA host layer (csrc/msda_entry.hip and the two size queries) against the table recorded by
tools/record_msda_host.py into tests/golden/msda_host.json: workspace sizes over a list of level geometries, and for all ten entry
points the status code and the mpf_last_error text of every single argument fault that is rejected before any HIP call — codes
exactly, texts exactly.  Needs no GPU: the pointers are made-up addresses that nothing dereferences, and a case that got as far as
the runtime would come back with a positive (HIP) status, which the recorder's own check rejects."""
import json

import pytest

from tools.record_msda_host import ENTRIES, FIXTURE, faults, size_queries


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    from mp_former_amd import _lib
    return _lib.lib()


def test_workspace_sizes_as_recorded(lib, recorded):
    got = size_queries(lib)
    assert sorted(got) == sorted(recorded["sizes"])
    wrong = {k: (v, recorded["sizes"][k]) for k, v in got.items() if v != recorded["sizes"][k]}
    assert not wrong, wrong
    assert any(v > 0 for v in got.values()) and any(v == 0 for v in got.values())


def test_single_faults_return_the_recorded_code_and_text(lib, recorded):
    got = faults(lib)
    assert sorted(got) == sorted(recorded["faults"])
    assert {k.split(":")[0] for k in got} == set(ENTRIES)
    wrong = {k: (v, recorded["faults"][k]) for k, v in got.items() if v != recorded["faults"][k]}
    assert not wrong, wrong
    assert all(code < 0 for code, _ in got.values())          # the library's own codes: nothing reached the runtime
