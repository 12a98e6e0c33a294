"""The clip decoder's two layer routes (mp_former_amd/video_decoder.py): 'native' — one native call per layer with the learned
query positions as an operand (decoder_layer.decoder_layer_pos) — against 'ops' — ``_layer_by_ops``, one autograd node per op —
on ONE module, switched by ``fused_layers``, on the fixtures of tests/_vdec_common.py under bf16 autocast: which route runs
when, the forward bit for bit, the gradients against the fp32 golden no further off than the op-by-op route's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _vdec_common as V
from conftest import ROOT
from test_video_decoder_gpu import _fixture, _module, _run

pytestmark = pytest.mark.gpu


def _route_run(m, name, z, cfg, tag, fused, grad):
    from mp_former_amd import video_decoder as VD
    m.fused_layers = fused
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            xs, mf, out, masks = _run(m, name, z, cfg, tag, "channels_last", grad)
    finally:
        m.fused_layers = None
    assert VD.last_layer_route() == ("native" if fused else "ops")
    return xs, mf, out, masks


def _grads(m, name, xs, mf, out):
    m.zero_grad(set_to_none=True)
    V.seeded_loss(f"{name}.train", V.outputs_list(out)).backward()
    params = dict(m.named_parameters())
    g = {f"x{i}": x.grad for i, x in enumerate(xs)}
    g["mf"] = mf.grad
    g.update({k: params[k].grad.clone() for k in V.SMALL_GRADS + V.WEIGHT_GRADS})
    return g


def test_default_route_is_native_under_bf16_autocast_and_ops_in_fp32():
    from mp_former_amd import _lib
    from mp_former_amd import video_decoder as VD
    name = "vdec_small"
    z, cfg = _fixture(name)
    m = _module(name, z, cfg)
    assert m.fused_layers is None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _run(m, name, z, cfg, "train", "channels_last", True)
    assert VD.last_layer_route() == "native" and _lib.last_kernel() is not None
    _run(m, name, z, cfg, "train", "channels_last", True)
    assert VD.last_layer_route() == "ops"
    m.fused_layers = True                               # forced where the native layer cannot run: an error, no fallback
    with pytest.raises(RuntimeError, match="fused_layers"):
        _run(m, name, z, cfg, "train", "channels_last", True)


@pytest.mark.parametrize("name", list(V.CONFIGS))
def test_training_routes_agree(name):
    """Forward: class logits and mask logits of every layer and every attention mask bit-equal between the routes.  Gradients
    (x0..x2, mask_features, query_embed, query_feat, level_embed, layer 0's attention weights): each route's relative L2 against
    the fp32 golden; the native route's must be <= 1.3 x the op-by-op route's per tensor (30 %: the convention of DESIGN section 2
    for a bf16 figure).  The route-to-route difference is printed (DESIGN section 9.8 records it)."""
    z, cfg = _fixture(name)
    m = _module(name, z, cfg)
    runs = {}
    for fused in (False, True):
        xs, mf, out, masks = _route_run(m, name, z, cfg, "train", fused, True)
        runs[fused] = (V.outputs_list(out), masks, _grads(m, name, xs, mf, out))
    (outs_o, masks_o, g_o), (outs_n, masks_n, g_n) = runs[False], runs[True]
    assert len(outs_o) == len(outs_n) == cfg["dec_layers"] + 1 and len(masks_o) == len(masks_n) == cfg["dec_layers"] + 1
    for l, ((c_o, m_o), (c_n, m_n)) in enumerate(zip(outs_o, outs_n)):
        assert torch.equal(c_o, c_n), f"class logits {l}"
        assert torch.equal(m_o, m_n), f"mask logits {l}"
    for l, (a, b) in enumerate(zip(masks_o, masks_n)):
        assert torch.equal(a, b), f"attention mask {l}"
    bad = []
    for k in g_o:
        want = z[f"train.grad.{k}"]
        e_o = float(np.linalg.norm(V.sample(g_o[k]) - want) / np.linalg.norm(want))
        e_n = float(np.linalg.norm(V.sample(g_n[k]) - want) / np.linalg.norm(want))
        between = float((g_n[k].double() - g_o[k].double()).norm() / g_o[k].double().norm())
        print(f"[vdec routes] {name} grad {k}: vs fp32 golden ops {e_o:.4f} native {e_n:.4f}; native vs ops {between:.4f}")
        if not e_n <= 1.3 * e_o:
            bad.append((k, e_o, e_n))
    assert not bad, bad


def test_eval_routes_bit_equal():
    """vdec_small in eval mode (3 frames of one clip, no_grad): every output and attention mask bit-equal between the routes"""
    name = "vdec_small"
    z, cfg = _fixture(name)
    m = _module(name, z, cfg)
    res = {}
    with torch.no_grad():
        for fused in (False, True):
            _, _, out, masks = _route_run(m, name, z, cfg, "eval", fused, False)
            res[fused] = (V.outputs_list(out), masks)
    for (c_o, m_o), (c_n, m_n) in zip(res[False][0], res[True][0]):
        assert torch.equal(c_o, c_n) and torch.equal(m_o, m_n)
    assert all(torch.equal(a, b) for a, b in zip(res[False][1], res[True][1]))


_CHILD = """
import sys, torch
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import test_video_decoder_gpu as T
from mp_former_amd import video_decoder as VD
z, cfg = T._fixture("vdec_small")
m = T._module("vdec_small", z, cfg)
with torch.autocast("cuda", dtype=torch.bfloat16), torch.no_grad():
    T._run(m, "vdec_small", z, cfg, "eval", "channels_last", False)
print("route", VD.last_layer_route())
"""


def test_env_switch_selects_the_op_by_op_route():
    """MPF_FUSED_DECODER=0 in a fresh process: ``_layer_by_ops`` under bf16 autocast"""
    env = dict(os.environ, MPF_FUSED_DECODER="0")
    code = _CHILD.format(tests=os.path.join(ROOT, "tests"), root=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "route ops" in out.stdout, out.stdout
