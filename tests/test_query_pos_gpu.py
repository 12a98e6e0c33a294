"""The two query-position kernels (csrc/query_pos.hip) called through the C ABI: the forward operand bf16(x + qpos[q]) and the
backward (d_x0 += float(dxq0); d_qpos[q] = sum over the query's N rows, in order, of float(dxq0) + float(dxq1)), bit for bit
against torch / a CPU loop in the stated order, at one row, ragged counts, more than one workgroup of the backward (Q * 32 > 256)
and of the forward; the memory behind the last row stays as it was."""
import pytest
import torch

gpu = pytest.mark.gpu

C = 256
CASES = [(1, 1), (7, 3), (33, 2), (230, 1), (100, 4)]
GUARD = 1024                         # elements behind every output, filled with a pattern and compared afterwards


def _guarded(t, dev, fill):
    """t on the device in front of a guard band of its own allocation -> (view of t's shape, guard view)"""
    buf = torch.full((t.numel() + GUARD,), fill, dtype=t.dtype, device=dev)
    buf[:t.numel()].copy_(t.flatten())
    return buf[:t.numel()].view(t.shape), buf[t.numel():]


def _problem(Q, N):
    g = torch.Generator().manual_seed(1000 * Q + N)
    x = torch.randn(Q, N, C, generator=g)
    qpos = torch.randn(Q, C, generator=g)
    dxq0 = torch.randn(Q, N, C, generator=g).bfloat16()
    dxq1 = (torch.randn(Q, N, C, generator=g) * 3).bfloat16()
    d_x0 = torch.randn(Q, N, C, generator=g)
    return x, qpos, dxq0, dxq1, d_x0


@gpu
@pytest.mark.parametrize("Q,N", CASES)
def test_operand_forward_is_the_rounded_fp32_sum(Q, N):
    from mp_former_amd import _lib
    dev = torch.device("cuda:0")
    x, qpos, *_ = _problem(Q, N)
    out, guard = _guarded(torch.zeros(Q, N, C, dtype=torch.bfloat16), dev, 7.0)
    xd, pd = x.to(dev), qpos.to(dev)
    _lib.call("mpf_qpos_operand_forward", dev, xd.data_ptr(), pd.data_ptr(), out.data_ptr(), Q, N, _lib.stream_ptr(dev))
    torch.cuda.synchronize()
    want = (x + qpos[:, None]).bfloat16()
    assert torch.equal(out.cpu(), want)
    assert torch.equal(out, (xd + pd[:, None]).bfloat16())
    assert bool((guard == 7.0).all())


@gpu
@pytest.mark.parametrize("Q,N", CASES)
def test_backward_sums_in_row_order_and_is_reproducible(Q, N):
    from mp_former_amd import _lib
    dev = torch.device("cuda:0")
    _, _, dxq0, dxq1, d_x0 = _problem(Q, N)
    a, b = dxq0.to(dev), dxq1.to(dev)
    runs = []
    for _ in range(2):
        dx, gx = _guarded(d_x0, dev, 5.0)
        dq, gq = _guarded(torch.full((Q, C), float("nan")), dev, 5.0)          # fully written: no NaN may survive
        _lib.call("mpf_qpos_backward", dev, a.data_ptr(), b.data_ptr(), dx.data_ptr(), dq.data_ptr(), Q, N, _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        assert bool((gx == 5.0).all()) and bool((gq == 5.0).all())
        runs.append((dx.cpu(), dq.cpu()))
    assert torch.equal(runs[0][0], d_x0 + dxq0.float())
    acc = torch.zeros(Q, C)
    for n in range(N):                                    # n = 0 .. N - 1, left to right, fp32
        acc = acc + (dxq0[:, n].float() + dxq1[:, n].float())
    assert torch.equal(runs[0][1], acc)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@gpu
def test_argument_checks_launch_nothing():
    from mp_former_amd import _lib
    lib = _lib.lib()
    one = 4096
    assert lib.mpf_qpos_operand_forward(one, None, one, 2, 2, None) == -3
    assert lib.mpf_qpos_operand_forward(one, one, one, 0, 2, None) == -2
    assert lib.mpf_qpos_operand_forward(one, one + 4, one, 2, 2, None) == -2          # not 16-byte aligned
    assert lib.mpf_qpos_backward(one, one, one, None, 2, 2, None) == -3
    assert lib.mpf_qpos_backward(one, one, one, one, 2, -1, None) == -2
