"""The pure-host answers of the small-row GEMM host layer (csrc/small_gemm_host.h, the entry points of csrc/small_gemm.hip, the size
queries of csrc/decoder_layer.hip) against the table recorded by tools/record_small_gemm_host.py into
tests/golden/small_gemm_host.json: for mpf_small_gemm_bf16, mpf_small_gemm_bf16_blocked, mpf_small_gemm_bf16_group,
mpf_transpose_group_bf16 and mpf_tall_gemm_bf16 the status code and the mpf_last_error text of every single argument fault that is
rejected before any HIP call, the 0 of the empty problems, every pair of faults of the blocked and the tall entry (the order of
their checks), and the three scratch size queries over zeros, negatives, Qt = 31 | 32 | 33, ffn_dim = 32 | 2048, forward and
backward — codes, texts and sizes exactly.  Needs no GPU: the pointers are made-up addresses that nothing dereferences, and a case
that got as far as the runtime would come back with a positive status, which the recorder's own check rejects."""
import json

import pytest

from tools.record_small_gemm_host import FAULTS, FIXTURE, GROUP_FAULTS, PAIRED, QUERIES, TRANSPOSE_FAULTS, faults, scratch_sizes


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


def test_scratch_sizes_as_recorded(lib, recorded):
    got = scratch_sizes(lib)
    assert sorted(got) == sorted(QUERIES) == sorted(recorded["scratch"])
    for query, table in got.items():
        wrong = _differences(table, recorded["scratch"][query])
        assert not wrong, (query, wrong)
        assert any(v == 0 for v in table.values()) and any(v > 0 for v in table.values())
    layer, pos = got["mpf_decoder_layer_scratch_bytes"], got["mpf_decoder_layer_pos_scratch_bytes"]
    assert all(pos[k] == v for k, v in layer.items() if k.endswith("backward=0"))          # positions add backward scratch only
    assert all(pos[k] > v for k, v in layer.items() if k.endswith("backward=1") and v)


def test_faults_give_the_recorded_code_and_text(lib, recorded):
    got = faults(lib)
    entries = set(FAULTS) | {"mpf_small_gemm_bf16_group", "mpf_transpose_group_bf16"}
    assert {k.split(":")[0] for k in got} == entries and len(entries) == 5
    wrong = _differences({k: list(v) for k, v in got.items()}, recorded["faults"])
    assert not wrong, wrong
    assert all(code <= 0 for code, _ in got.values())                # the library's own codes: nothing reached the runtime
    # every single fault of every entry and every pair on different arguments of the two entries whose check order is pinned
    singles = sum(len(t) for t in FAULTS.values()) + len(GROUP_FAULTS) + len(TRANSPOSE_FAULTS)
    assert sum(" + " not in k for k in got) == singles
    for entry in PAIRED:
        n = len(FAULTS[entry])
        assert sum(k.startswith(entry + ":") and " + " in k for k in got) > n * (n - 1) // 2 * 3 // 4
    assert {code for code, _ in got.values()} == {0, -2, -3, -4}          # empty, MPF_E_SHAPE, MPF_E_NULL, MPF_E_TOO_LARGE
