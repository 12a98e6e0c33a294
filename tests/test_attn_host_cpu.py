"""The pure-host answers of the attention host layer (csrc/attn_host.h and the entry points of csrc/attn.hip) against the table
recorded by tools/record_attn_host.py into tests/golden/attn_host.json: the two size queries over a table of shapes under three
settings of the split options, the return code of every attention option value, and for all ten entry points the status code and
the mpf_last_error text of every single argument fault that is rejected before any HIP call — codes exactly, texts exactly.
Needs no GPU: the pointers are made-up addresses that nothing dereferences, and a case that got as far as the runtime would come
back with a positive (HIP) status, which the recorder's own check rejects."""
import json

import pytest

from tools.record_attn_host import ENTRIES, FIXTURE, OPTION_DEFAULTS, faults, options, size_queries


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    from mp_former_amd import _lib
    l = _lib.lib()
    yield l
    for k, v in OPTION_DEFAULTS.items():
        _lib.set_option(k, v)


def _differences(got, want):
    assert sorted(got) == sorted(want)
    return {k: (v, want[k]) for k, v in got.items() if v != want[k]}


def test_sizes_as_recorded(lib, recorded):
    got = size_queries(lib)
    wrong = _differences(got, recorded["sizes"])
    assert not wrong, wrong
    assert any(v > 0 for v in got.values()) and any(v == 0 for v in got.values())


def test_option_values_return_the_recorded_code(lib, recorded):
    wrong = _differences(options(lib), recorded["options"])
    assert not wrong, wrong


def test_single_faults_return_the_recorded_code_and_text(lib, recorded):
    got = faults(lib)
    assert {k.split(":")[0] for k in got} == set(ENTRIES)
    wrong = _differences({k: list(v) for k, v in got.items()}, recorded["faults"])
    assert not wrong, wrong
    assert all(code < 0 for code, _ in got.values())          # the library's own codes: nothing reached the runtime
