"""The Swin backbone without a GPU: names and shapes of the reference's state dict, the closed-form index, the torch route against
the reference's fp64 results (tests/golden/swin_tiny.npz, tests/golden/make_golden_swin.py), stochastic depth, train(), frozen
stages, the detectron2 registration with stand-ins, and the argument errors of the two native entries."""
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

import _swin_common as S
import _win_attn_cases as W
from conftest import GOLDEN


@pytest.fixture(scope="module")
def swin():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import swin
    return swin


@pytest.mark.parametrize("size", sorted(S.SIZES))
def test_state_dict_keys_and_shapes_equal_the_reference(swin, size):
    want = json.load(open(os.path.join(GOLDEN, "swin_keys.json")))[size]
    got = {k: list(v.shape) for k, v in swin.SwinTransformer(**S.SIZES[size]).state_dict().items()}
    assert sorted(got) == sorted(want)
    assert got == want


def test_ape_adds_the_position_embedding_key(swin):
    m = swin.SwinTransformer(pretrain_img_size=64, ape=True, **S.TINY)
    assert tuple(m.state_dict()["absolute_pos_embed"].shape) == (1, 32, 16, 16)


@pytest.mark.parametrize("ws", [2, 3, 7, 8, 12])
def test_relative_position_index_is_the_closed_form_of_the_kernel(swin, ws):
    idx = swin.relative_position_index(ws)
    assert idx.dtype == torch.int64 and torch.equal(idx, W.index_buffer(ws))
    _, code, _ = W.token_geometry(W.Case(1, ws, ws, 1, ws, 0))
    assert torch.equal(idx, code[:, None] - code[None, :] + (ws - 1) * 2 * ws)
    m = swin.WindowAttention(32, ws, 1)
    assert torch.equal(m.relative_position_index, idx)


def _tiny(swin, **kw):
    m = swin.SwinTransformer(**{**S.TINY, **kw}).double()
    m.load_state_dict(S.det_state(m), strict=True)
    return m


def test_torch_route_reproduces_the_reference_in_fp64(swin):
    z = np.load(os.path.join(GOLDEN, "swin_tiny.npz"))
    m = _tiny(swin).train()
    x = S.det_input().requires_grad_(True)
    outs = m(x)
    assert swin.last_route() == "torch" and sorted(outs) == sorted(S.OUTPUTS)
    S.loss_of(outs).backward()
    params = dict(m.named_parameters())
    got = {k: outs[k].detach() for k in S.OUTPUTS}
    got["grad.input"] = x.grad
    got.update({"grad." + k: params[k].grad for k in S.GRAD_PARAMS})
    assert sorted(got) == sorted(z.files)
    for k in z.files:
        np.testing.assert_allclose(got[k].numpy(), z[k], rtol=1e-10, atol=1e-10, err_msg=k)


def test_use_checkpoint_gives_the_same_results(swin):
    x = S.det_input()
    a, b = _tiny(swin).train(), _tiny(swin, use_checkpoint=True).train()
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    S.loss_of(a(xa)).backward()
    S.loss_of(b(xb)).backward()
    assert torch.equal(xa.grad, xb.grad)


def test_window_attention_torch_equals_the_case_reference(swin):
    """the torch route on the kernel's test problems: the same function as tests/_win_attn_cases.reference"""
    for case in (W.CASES[1], W.CASES[2], W.CASES[7]):
        prob = W.build(case)
        out = swin.window_attention_torch(prob["qkv"].double(), prob["table"].double(), case.ws, case.shift, W.SCALE)
        assert (out - W.reference(prob)["out"]).abs().max() < 1e-12


def test_stochastic_depth(swin):
    d = swin.DropPath(0.25)
    x = torch.randn(64, 5, 3).abs() + 1.0
    assert d.eval()(x) is x
    torch.manual_seed(0)
    y = d.train()(x)
    kept = (y != 0).flatten(1).any(1)
    assert 0 < int(kept.sum()) < 64
    assert torch.equal(y[kept], x[kept] * (torch.ones(()) / 0.75)) and (y[~kept] == 0).all()
    m = swin.SwinTransformer(**{**S.TINY, "drop_path_rate": 0.2})
    rates = [b.drop_path.p if isinstance(b.drop_path, swin.DropPath) else 0.0 for l in m.layers for b in l.blocks]
    assert rates == pytest.approx(torch.linspace(0, 0.2, 8).tolist())


def test_train_returns_self_and_keeps_frozen_stages_in_eval(swin):
    m = swin.SwinTransformer(frozen_stages=2, **S.TINY)
    assert m.train() is m and m.eval() is m and m.train(False) is m
    m.train()
    assert not m.patch_embed.training and not m.pos_drop.training and not m.layers[0].training
    assert m.layers[1].training and m.layers[3].training


@pytest.mark.parametrize("stages", [-1, 0, 1, 2, 3])
def test_frozen_stages_freeze_what_the_reference_freezes(swin, stages):
    m = swin.SwinTransformer(frozen_stages=stages, ape=True, pretrain_img_size=64, **S.TINY)
    frozen = {k for k, p in m.named_parameters() if not p.requires_grad}
    want = set()
    for k, _ in m.named_parameters():
        if stages >= 0 and k.startswith("patch_embed."):
            want.add(k)
        if stages >= 1 and k == "absolute_pos_embed":
            want.add(k)
        if stages >= 2 and any(k.startswith(f"layers.{i}.") for i in range(stages - 1)):
            want.add(k)
    assert frozen == want


def test_register_backbone_with_a_stub_registry(swin):
    from mp_former_amd import d2_plugin

    class Registry(dict):
        def register(self, obj):
            self[obj.__name__] = obj

    class Backbone(torch.nn.Module):
        pass

    reg = Registry()
    cls = d2_plugin.register_backbone(reg, Backbone)
    assert reg["D2SwinTransformerHIP"] is cls and issubclass(cls, Backbone) and issubclass(cls, swin.SwinTransformer)
    sw = types.SimpleNamespace(PRETRAIN_IMG_SIZE=224, PATCH_SIZE=4, EMBED_DIM=32, DEPTHS=[2, 2, 2, 2], NUM_HEADS=[1, 2, 4, 8],
                               WINDOW_SIZE=7, MLP_RATIO=4.0, QKV_BIAS=True, QK_SCALE=None, DROP_RATE=0.0, ATTN_DROP_RATE=0.0,
                               DROP_PATH_RATE=0.3, APE=False, PATCH_NORM=True, USE_CHECKPOINT=False, OUT_FEATURES=["res3", "res5"])
    cfg = types.SimpleNamespace(MODEL=types.SimpleNamespace(SWIN=sw))
    m = cls(cfg, None)
    assert m.size_divisibility == 32
    shapes = m.output_shape()
    assert {k: (v.channels, v.stride) for k, v in shapes.items()} == {"res3": (64, 8), "res5": (256, 32)}
    out = m.eval()(torch.zeros(1, 3, 32, 32))
    assert {k: tuple(v.shape) for k, v in out.items()} == {"res3": (1, 64, 4, 4), "res5": (1, 256, 1, 1)}
    try:
        import detectron2  # noqa: F401
    except ImportError:
        assert d2_plugin.register_backbone() is False


def test_argument_errors_of_the_native_entries(swin):
    """every rejection happens before any HIP call: the pointers are never dereferenced and no GPU is needed"""
    from mp_former_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    good = dict(B=1, Hp=14, Wp=21, heads=3, head_dim=32, ws=7, shift=3)

    def fwd(qkv=one, table=one, out=one, **kw):
        a = {**good, **kw}
        return lib.mpf_win_attn_forward(qkv, table, out, a["B"], a["Hp"], a["Wp"], a["heads"], a["head_dim"], a["ws"], a["shift"], 0.25, None)

    def bwd(bufs=(one,) * 7, nbytes=1 << 30, **kw):
        a = {**good, **kw}
        return lib.mpf_win_attn_backward(*bufs[:6], a["B"], a["Hp"], a["Wp"], a["heads"], a["head_dim"], a["ws"], a["shift"], 0.25, bufs[6],
                                         nbytes, None)

    for call in (fwd, bwd):
        assert call(ws=13, Hp=13, Wp=13) == -2 and b"window size" in lib.mpf_last_error()
        assert call(ws=1, shift=0) == -2
        assert call(head_dim=64) == -2 and b"head_dim" in lib.mpf_last_error()
        assert call(shift=7) == -2 and call(shift=-1) == -2 and b"shift" in lib.mpf_last_error()
        assert call(Hp=15) == -2 and call(Wp=20) == -2 and b"multiples" in lib.mpf_last_error()
        assert call(B=0) == -2 and call(heads=0) == -2
        assert call(B=4096, Hp=252, Wp=252, heads=32) == -4
    assert fwd(qkv=None) == -3 and fwd(table=None) == -3 and fwd(out=None) == -3
    for i in range(7):
        assert bwd(bufs=(one,) * i + (None,) + (one,) * (6 - i)) == -3, i
    assert fwd(qkv=ctypes.c_void_p(24)) == -2 and b"aligned" in lib.mpf_last_error()
    assert bwd(nbytes=16) == -2 and b"workspace" in lib.mpf_last_error()
    need = lib.mpf_win_attn_workspace_bytes(2, 264, 264, 4, 12)
    assert need >= 128 * 4 * 23 * 23 * 4 and need % 256 == 0
    assert lib.mpf_win_attn_workspace_bytes(2, 264, 264, 4, 13) == 0 and lib.mpf_win_attn_workspace_bytes(2, 265, 264, 4, 12) == 0
