"""The shifted-window attention checks of tests/_win_attn_cases.py, tested without a GPU: the torch emulation of the kernel's
arithmetic stays inside every bound on every case with no element left out, and every single fault of `_win_attn_cases.FAULTS`
leaves a bound on every case where it can apply — the assertions of tests/test_win_attn_gpu.py are sharp without a wrong kernel
ever running on a device."""
import pytest
import torch

import _win_attn_cases as W


@pytest.fixture(scope="module")
def problems():
    out = {}
    for c, cid in zip(W.CASES, W.CASE_IDS):
        prob = W.build(c)
        out[cid] = (prob, W.reference(prob))
    return out


def test_case_table_covers_the_token_tails_and_the_mask_regions():
    assert {c.ws * c.ws for c in W.CASES} == {9, 49, 64, 144}
    assert any(c.Hp == c.ws and c.Wp == c.ws and c.shift for c in W.CASES)
    assert any(c.heads % 2 == 1 and c.heads > 1 for c in W.CASES) and any(c.heads == 1 for c in W.CASES)
    for c in W.CASES:
        assert c.Hp % c.ws == 0 and c.Wp % c.ws == 0 and 0 <= c.shift < c.ws
    nine = [c for c in W.CASES if c.shift and len(torch.unique(W.token_geometry(c)[2])) == 9]
    assert nine, "no case in which all nine mask regions occur"


@pytest.mark.parametrize("ws", [2, 3, 7, 8, 12])
def test_closed_forms_equal_the_reference_constructions(ws):
    """the kernel's index and region arithmetic against the buffer and the mask built as the reference builds them"""
    case = W.Case(1, 2 * ws, 3 * ws, 1, ws, ws // 2)
    pos, code, region = W.token_geometry(case)
    assert torch.equal(code[:, None] - code[None, :] + (ws - 1) * 2 * ws, W.index_buffer(ws))
    differ = region[:, :, None] != region[:, None, :]
    assert torch.equal(differ, W.slice_mask(case.Hp, case.Wp, ws, case.shift) != 0)
    # the gather by `pos` is the roll and the partition
    m = torch.arange(case.Hp * case.Wp, dtype=torch.float64).view(1, case.Hp, case.Wp, 1)
    assert torch.equal(m.view(-1)[pos], W._to_windows(m, ws, case.shift)[0, :, :, 0])


@pytest.mark.parametrize("cid", W.CASE_IDS)
def test_emulation_stays_inside_the_bounds(problems, cid):
    prob, ref = problems[cid]
    res = W.emulate(prob)
    C = prob["case"].heads * W.HD
    assert res["out"].shape == prob["dout"].shape and res["dqkv"].shape == prob["qkv"].shape and res["dqkv"].shape[-1] == 3 * C
    ratios = W.evaluate(prob, res, ref)
    assert set(ratios) == {"out", "dq", "dk", "dv", "dtable"}
    assert all(0 < r <= 1 for r in ratios.values()), ratios          # (a ratio of 0 would mean a tensor that was never compared)


@pytest.mark.parametrize("fault", W.FAULTS)
@pytest.mark.parametrize("cid", W.CASE_IDS)
def test_every_fault_leaves_a_bound(problems, cid, fault):
    prob, ref = problems[cid]
    case = prob["case"]
    if not W.fault_applies(prob, fault):
        # said from the case data: an unshifted block has no roll and no mask, one head has no next column
        assert (fault in ("roll", "region_edge", "mask_zero") and case.shift == 0) or (fault == "bias_next_head" and case.heads == 1)
        assert fault != "roll" or torch.equal(W.token_geometry(case)[0], W.token_geometry(case, roll=0)[0])
        return
    with pytest.raises(AssertionError, match="leaves its bound"):
        W.evaluate(prob, W.emulate(prob, fault), ref)
