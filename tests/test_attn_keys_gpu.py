"""csrc/attn.hip key by key: the sparse problems of tests/_attn_cases.py (every open key carries O(1) weight, masked decoys sit
around every split, tail and block edge and at the clamped-load positions) through the C ABI on every split shape — one wave,
several waves, workgroups with empty wave slots, more than 8 workgroups, kpw 512, the library's own policy — with the workspace
filled with 0xFF bytes and every output pre-filled with NaN.  The assertions are `_attn_cases.evaluate`, the ones that
tests/test_attn_keys_cpu.py proves sharp against single index faults.

Measured on an MI355X (the [attn keys] lines this test prints: worst err / bound per tensor and case): the bit-exact lines hold as
equalities; lse of the one-key rows <= 0.023 of its bound; few-key rows out <= 0.84, dq <= 0.57, dk <= 0.59, dv <= 0.92."""
import pytest
import torch

import _attn_cases as A

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _reset_split_options():
    from mp_former_amd import _lib
    yield
    _lib.set_option("attn_kpw", 0)
    _lib.set_option("attn_nw", 8)


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _device_mask(prob, dev):
    """the mask on the device: a fresh allocation, or a contiguous view at an odd byte offset of a larger buffer"""
    m = prob["mask"]
    if m is None:
        return None
    if not prob["case"].odd:
        return m.to(dev)
    buf = torch.ones(m.numel() + 16, dtype=torch.bool, device=dev)
    view = buf[1:1 + m.numel()].view(m.shape)
    view.copy_(m)
    assert view.is_contiguous() and view.data_ptr() % 2 == 1
    return view


def wg_splits_of_library(lib, Lq, Lk, N):
    """the workgroup-level splits the library will use, from its own sizes: the workspace holds `splits` partials of (32 + 2) floats
    per (image, head, query), rounded up to 256 bytes, and the aux operands of a backward with a per-image mask"""
    part = lib.mpf_attn_workspace_bytes(Lq, Lk, N, A.H) - lib.mpf_attn_bwd_aux_bytes(Lq, Lk, N, A.H, N)
    per_split = N * A.H * Lq * (A.HD + 2) * 4
    assert per_split >= 256 and part % 256 == 0
    return part // per_split


def run_native(prob):
    """forward and backward through the C ABI -> out, lse, dq, dk, dv on the CPU"""
    from mp_former_amd import _lib
    lib = _lib.lib()
    c = prob["case"]
    Lq, Lk, N = c.Lq, c.Lk, c.N
    LqP = (Lq + 31) // 32 * 32
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.set_option("attn_kpw", c.kpw)
    _lib.set_option("attn_nw", c.nw)
    assert wg_splits_of_library(lib, Lq, Lk, N) == c.wg, "the case does not reach the split class it is meant for"
    q, k, v, do = (prob[n].bfloat16().to(dev) for n in ("q", "k", "v", "dO"))
    mask = _device_mask(prob, dev)
    mp, per = (None if mask is None else mask.data_ptr()), (1 if c.mask == "image" else 0)
    ws = torch.empty(lib.mpf_attn_workspace_bytes(Lq, Lk, N, A.H), dtype=torch.uint8, device=dev)
    kt, vt = (_nan((N, A.E, Lk), torch.bfloat16, dev) for _ in range(2))
    _lib.check(lib.mpf_attn_transpose2(k.data_ptr(), v.data_ptr(), kt.data_ptr(), vt.data_ptr(), Lk, Lk, N, A.E, st), "transpose2")
    out = _nan((Lq, N, A.E), torch.bfloat16, dev)
    lse = _nan((N, A.H, Lq), torch.float32, dev)
    ws.fill_(0xFF)
    _lib.check(lib.mpf_attn_forward(q.data_ptr(), k.data_ptr(), vt.data_ptr(), mp, per, out.data_ptr(), lse.data_ptr(), Lq, Lk, N, A.H,
                                    A.HD, A.SCALE, ws.data_ptr(), ws.numel(), st), "forward")
    qT, doT = (_nan((N, A.E, LqP), torch.bfloat16, dev) for _ in range(2))
    delta = _nan((N, A.H, Lq), torch.float32, dev)
    _lib.check(lib.mpf_attn_bwd_prep(q.data_ptr(), do.data_ptr(), out.data_ptr(), qT.data_ptr(), doT.data_ptr(), delta.data_ptr(),
                                     Lq, LqP, N, A.H, st), "bwd_prep")
    dq = _nan((Lq, N, A.E), torch.bfloat16, dev)
    dk, dv = (_nan((Lk, N, A.E), torch.bfloat16, dev) for _ in range(2))
    ws.fill_(0xFF)
    _lib.check(lib.mpf_attn_backward(q.data_ptr(), k.data_ptr(), v.data_ptr(), kt.data_ptr(), qT.data_ptr(), do.data_ptr(),
                                     doT.data_ptr(), mp, per, lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dk.data_ptr(),
                                     dv.data_ptr(), Lq, LqP, Lk, N, A.H, A.HD, A.SCALE, ws.data_ptr(), ws.numel(), st), "backward")
    torch.cuda.synchronize(dev)
    return dict(out=out.cpu(), lse=lse.cpu(), dq=dq.cpu(), dk=dk.cpu(), dv=dv.cpu())


@pytest.mark.parametrize("case", A.CASES, ids=A.CASE_IDS)
def test_attention_key_exact(case):
    """selector rows: out == v[key] and dv[key] == dO bit for bit, lse the fp64 score, zero gradients for every key no row opens;
    few-keys, no-mask and fully-masked-row problems: per-element bounds against fp64, zeros / -inf for fully masked rows.
    Everything finite although the workspace held 0xFF bytes and the outputs NaN."""
    prob = A.build(case)
    ratios = A.evaluate(prob, run_native(prob))
    print(f"[attn keys] {case.name} ({case.family}, Lq {case.Lq} Lk {case.Lk} N {case.N}, kpw {case.kpw_eff} wg {case.wg}): "
          + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
