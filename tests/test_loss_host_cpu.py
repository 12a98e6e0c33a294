"""The pure-host answers of the loss host layer (csrc/loss_host.h and the entry points of csrc/loss.hip) against the table recorded
by tools/record_loss_host.py into tests/golden/loss_host.json: mpf_match_cost_clip_workspace_bytes over a table of (n_rows, F, Tmax)
and, for all ten entry points, the status code and the mpf_last_error text of every single argument fault that is rejected before
any HIP call and of the "nothing to do" zero returns — codes exactly, texts exactly.  Needs no GPU: the pointers are made-up
addresses that nothing dereferences, and a case that got as far as the runtime would come back with a positive (HIP) status, which
the recorder's own check rejects."""
import json

import pytest

from tools.record_loss_host import ENTRIES, FIXTURE, faults, workspace_sizes


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
    wrong = _differences(got, recorded["workspace"])
    assert not wrong, wrong
    assert got["n_rows=12 F=3 Tmax=5"] == 12 * 3 * (2 + 3 * 5) * 4 and any(v == 0 for v in got.values())


def test_single_faults_and_zero_returns_give_the_recorded_code_and_text(lib, recorded):
    got = faults(lib)
    assert {k.split(":")[0] for k in got} == set(ENTRIES) and len(ENTRIES) == 9        # the tenth entry is the size query above
    wrong = _differences({k: list(v) for k, v in got.items()}, recorded["faults"])
    assert not wrong, wrong
    assert all(code <= 0 for code, _ in got.values())                # the library's own codes: nothing reached the runtime
