"""The small-row GEMM host layer (csrc/small_gemm_host.h: one problem record, one check, one launcher per entry of
csrc/small_gemm.hip) and the decoder layer that sequences it (csrc/decoder_layer.hip) against the table recorded by
tools/record_small_gemm_routes.py into tests/golden/small_gemm_routes.json: on the smallest problems that reach each host decision —
the three tile widths on both sides of the 256-block rule, the four operand forms with and without gate and contraction tail, the
three blocked forms, grouped launches of 1 and 8 problems in both operand forms with an empty item, transposes of 1, 2 and 16 matrices,
the tall entry on both sides of M = 1024 at K = 64 | 256 | 768 with its two options, and one decoder layer forward and backward
under every setting of decoder_dw_group and decoder_row_chain, packed and unpacked, with and without query positions — every entry
must name the same kernel, log the same profiler records with the same bytes and flops and write the same bits, into every output
buffer (canaries included) and the layer's scratch workspace, as when the fixture was recorded.  The kernels are fixed-order without
atomics, so everything is compared exactly."""
import json

import pytest
import torch

from tools.record_small_gemm_routes import CASES, FIXTURE, TILE_WIDTH, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases_of_the_table(recorded):
    assert sorted(recorded["cases"]) == sorted(CASES)
    assert recorded["unstable"] == {}           # every buffer of every case reproduced when the fixture was recorded


def test_the_cases_reach_the_host_decisions_they_name(recorded):
    from test_small_gemm_forms_gpu import _nj
    assert all(_nj(I, J) == nj for I, J, nj in TILE_WIDTH) and {nj for _, _, nj in TILE_WIDTH} == {1, 2, 4}
    kernels = {cid: set(c["kernels"]) for cid, c in recorded["cases"].items()}
    assert all(k == {"small_gemm_kernel"} for cid, k in kernels.items() if CASES[cid]["kind"] == "gemm")
    assert all("small_gemm_group_kernel" in k for cid, k in kernels.items() if CASES[cid]["kind"] == "group")
    # the transpose entry with 16, 2 and 1 matrices (the last: its own case, nothing but the transpose)
    assert [recorded["cases"][cid]["kernels"] for cid, c in CASES.items() if c["kind"] == "transpose"] == [["transpose_group_kernel"]]
    assert {2 * len(c["which"]) for c in CASES.values() if c["kind"] == "group" and c.get("Rp")} == {2, 16}
    tall = {cid: k for cid, k in kernels.items() if CASES[cid]["kind"] == "tall"}
    for cid, k in tall.items():
        ws = all(M >= 1024 and K in (256, 768) for M, _, K, _ in CASES[cid]["calls"]) and CASES[cid].get("options", {}).get("tall_ws", 1)
        assert k == ({"tall_ws_bf16_kernel"} if ws else {"tall_gemm_bf16_kernel"}), cid
    assert sum(k == {"tall_ws_bf16_kernel"} for k in tall.values()) >= 6
    layers = [c for c in CASES.values() if c["kind"] == "layer"]
    assert {(c["pos"], c["packed"], c["options"].get("decoder_dw_group")) for c in layers if not c.get("forward_only")} == {
        (p, k, v) for p in (False, True) for k in (False, True) for v in (0, 1, 2)}


@pytest.mark.parametrize("cid", list(CASES))
def test_kernels_records_and_bits_as_recorded(cid, recorded):
    want = recorded["cases"][cid]
    got = run_case(CASES[cid], torch.device("cuda:0"))
    assert got["kernels"] == want["kernels"]
    assert got["prof"] == want["prof"]
    assert sorted(got["hashes"]) == sorted(want["hashes"])
    for name, h in want["hashes"].items():
        assert got["hashes"][name] == h, f"{name} differs from the recorded bits"
    if CASES[cid]["kind"] == "tall" and len(set(CASES[cid]["calls"])) == 1:
        assert got["hashes"]["0.c"] == got["hashes"]["1.c"]
