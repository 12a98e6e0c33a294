"""csrc/win_attn.hip on the device: forward and backward on every case of tests/_win_attn_cases.py against the fp64 reference — out,
the three thirds of dqkv and the table gradient, all elements — a bit-identical second backward, the kernel's name, and the
argument error of an unsupported window."""
import pytest
import torch

import _win_attn_cases as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def swin():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import swin
    return swin


def _run(swin, prob, dev):
    qkv = prob["qkv"].to(dev).bfloat16().requires_grad_(True)
    table = prob["table"].to(dev).requires_grad_(True)
    out = swin.window_attention(qkv, table, prob["case"].ws, prob["case"].shift, W.SCALE)
    dout = prob["dout"].to(dev).bfloat16()
    out.backward(dout, retain_graph=True)
    first = dict(out=out.detach().cpu(), dqkv=qkv.grad.cpu(), dtable=table.grad.cpu())
    qkv.grad = table.grad = None
    out.backward(dout)
    torch.cuda.synchronize()
    return first, dict(dqkv=qkv.grad.cpu(), dtable=table.grad.cpu())


@pytest.mark.parametrize("case", W.CASES, ids=W.CASE_IDS)
def test_forward_and_backward_against_fp64(swin, case):
    from mp_former_amd import _lib
    prob = W.build(case)
    first, second = _run(swin, prob, torch.device("cuda:0"))
    assert "win_attn" in _lib.last_kernel(), _lib.last_kernel()
    ratios = W.evaluate(prob, first)
    print(case, {k: round(v, 3) for k, v in ratios.items()})
    assert torch.equal(first["dqkv"].view(torch.int16), second["dqkv"].view(torch.int16)), "dqkv differs between two runs"
    assert torch.equal(first["dtable"].view(torch.int32), second["dtable"].view(torch.int32)), "dtable differs between two runs"


def test_kernel_names(swin):
    from mp_former_amd import _lib
    dev = torch.device("cuda:0")
    prob = W.build(W.CASES[-1])
    qkv = prob["qkv"].to(dev).bfloat16().requires_grad_(True)
    out = swin.window_attention(qkv, prob["table"].to(dev), 3, 1, W.SCALE)
    assert _lib.last_kernel() == "win_attn_fwd_kernel"
    out.backward(prob["dout"].to(dev).bfloat16())
    assert _lib.last_kernel() == "win_attn_bwd_kernel"


def test_unsupported_sizes_raise(swin):
    dev = torch.device("cuda:0")
    qkv = torch.zeros(1, 13, 13, 96, dtype=torch.bfloat16, device=dev)
    with pytest.raises(RuntimeError, match="mpf_win_attn_forward failed with code -2"):
        swin.window_attention(qkv, torch.zeros(25 * 25, 1, device=dev), 13, 0, W.SCALE)
    with pytest.raises(RuntimeError, match="mpf_win_attn_forward failed with code -2"):
        swin.window_attention(torch.zeros(1, 7, 8, 96, dtype=torch.bfloat16, device=dev), torch.zeros(169, 1, device=dev), 7, 0, W.SCALE)
    with pytest.raises(RuntimeError, match="bf16"):
        swin.window_attention(qkv.float(), torch.zeros(25 * 25, 1, device=dev), 13, 0, W.SCALE)
