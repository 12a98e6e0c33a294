"""The loss host layer (csrc/loss_host.h: one problem record, one check, one route choice, one dynamic-LDS launcher) against the
table recorded by tools/record_loss_routes.py into tests/golden/loss_routes.json: on the smallest problems that reach each host
decision — both sides of every LDS limit (12 800 points, 128 and 136 KiB planes, 256 chunks), the row-group rules of the image and
clip cost, byte and bit masks, one and three bands, the steps of 16 / 37 / 40 keys per thread — every entry point must name the same
kernel, log the same profiler record and byte count and write the same bits as when the fixture was recorded.  The two-step cases
launch one kernel with a larger and then a smaller dynamic-LDS size in this process.  The fp32 gradient of mpf_mask_loss_backward
(global atomics) does not reproduce bit for bit and is held to the fp64 restatement at the bound of tests/test_loss_routes_gpu.py
(rtol 1e-4, atol 1e-4)."""
import json

import pytest
import torch

import _loss_restate as LR
from tools.record_loss_routes import ATOMIC, CASES, FIXTURE, pairs_problem, run_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_holds_exactly_the_cases_of_the_table(recorded):
    assert sorted(recorded["cases"]) == sorted(CASES)


@pytest.mark.parametrize("cid", list(CASES))
def test_kernels_records_and_bits_as_recorded(cid, recorded):
    want, steps = recorded["cases"][cid], CASES[cid]
    got, bufs = run_case(steps, torch.device("cuda:0"), hashed=sorted(want["hashes"]))
    print(cid, got["kernels"], got["prof"])
    assert got["kernels"] == want["kernels"]
    assert got["prof"] == want["prof"]
    loose = sorted(k for k in bufs if k not in want["hashes"])
    assert loose == [k for k in sorted(bufs) if k.endswith(ATOMIC)], "only the atomic gradient may be left unhashed"
    for name, h in want["hashes"].items():
        assert got["hashes"][name] == h, f"{name} differs from the recorded bits"
    for name in loose:
        p = pairs_problem(steps[int(name.split(".")[0])])
        ref = LR.mask_loss_grad(p["maps"][p["slots"]], p["gt"][p["gt_rows"]], p["coords"], p["gs"])
        out = bufs[name].cpu()
        rest = [i for i in range(out.shape[0]) if i not in p["slots"]]
        assert torch.equal(out[rest], p["base"][rest]), "a plane of no pair was touched"
        want_g = p["base"][p["slots"]].double() + ref
        err = (out[p["slots"]].double() - want_g).abs()
        frac = float((err / (1e-4 + 1e-4 * want_g.abs())).max())
        print(f"[loss-routes-recorded] {cid} | {name} | max abs err {float(err.max()):.3e} | worst err/bound {frac:.3e}")
        assert frac <= 1.0, (name, float(err.max()), frac)
