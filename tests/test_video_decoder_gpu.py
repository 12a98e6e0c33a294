"""The clip decoder (mp_former_amd/video_decoder.py, csrc/video_decoder.hip) on the GPU: the clip-inputs kernel against its torch
statement, the all-masked-row rule over the clip on both mask routes, the whole module against the reference's own results
(tests/golden/vdec_*.npz, made by tests/golden/make_golden_vdec.py), the hand-over to the clip criterion and
``d2_plugin.install_native_video_decoder``."""
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import _vdec_common as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


# ---- 1. clip inputs ---------------------------------------------------------------------------------------------------------------
def _padded_frames(BT, C, H, W, pad, fill, gen):
    """x [BT, C, H, W] as channel-last planes inside a buffer with ``pad`` floats between frames -> (x, buffer)"""
    S = H * W
    buf = torch.full((BT, S * C + pad), fill, dtype=torch.float32)
    buf[:, :S * C] = torch.randn(BT, S * C, generator=gen)
    buf = buf.to(DEV)
    x = buf[:, :S * C].view(BT, H, W, C).permute(0, 3, 1, 2)
    assert x.stride() == (S * C + pad, 1, W * C, C)
    return x, buf


def _clip_statement(x, level, pos_yx, pos_z, B, T):
    """the statement of include/mpformer_hip.h, fp32, in its order: x + level first, the two tables summed first, then one add"""
    BT, C, H, W = x.shape
    S = H * W
    src = x.reshape(B, T, C, S) + level[None, None, :, None]
    src = src.permute(1, 3, 0, 2).reshape(T * S, B, C)                          # [(t * S + s), b, c]
    pos = (pos_yx[None, :, :] + pos_z[:, None, :]).reshape(T * S, 1, C)
    return src, src + pos


@pytest.mark.parametrize("grid", [(3, 5), (8, 12)])
def test_clip_inputs_forward_and_backward_equal_the_torch_statement(grid):
    from mp_former_amd import _lib
    from mp_former_amd.video_decoder import PositionEmbeddingSine3D, _ClipInputs
    B, T, C = 2, 3, 256
    H, W = grid
    S, pad = H * W, 64
    gen = torch.Generator().manual_seed(H * 100 + W)
    x, buf = _padded_frames(B * T, C, H, W, pad, 7.5, gen)
    level = torch.randn(C, generator=gen).to(DEV)
    pos_yx, pos_z = PositionEmbeddingSine3D(C // 2, normalize=True).tables(T, H, W, DEV)
    want_src, want_kin = _clip_statement(x, level, pos_yx, pos_z, B, T)
    for dt in (torch.float32, torch.bfloat16):
        src, kin = _ClipInputs.apply(x, level, pos_yx, pos_z, T, dt)
        assert _lib.last_kernel() == "clip_inputs_fwd_kernel"
        assert src.shape == kin.shape == (T * S, B, C) and src.dtype == kin.dtype == dt and src.is_contiguous() and kin.is_contiguous()
        assert torch.equal(src, want_src.to(dt)) and torch.equal(kin, want_kin.to(dt))
    assert torch.all(buf[:, S * C:] == 7.5)
    # backward: dx = g_src + g_kin in fp32, each of the two NULL in turn, written with x's strides; the padding stays as it was
    for gdt in (torch.float32, torch.bfloat16):
        g_src = torch.randn(T * S, B, C, generator=gen).to(DEV).to(gdt)
        g_kin = torch.randn(T * S, B, C, generator=gen).to(DEV).to(gdt)
        for a, b in ((g_src, g_kin), (g_src, None), (None, g_kin)):
            dbuf = torch.full((B * T, S * C + pad), -3.25, dtype=torch.float32, device=DEV)
            _lib.call("mpf_clip_inputs_backward", DEV, _lib.ptr(a), _lib.ptr(b), _lib.DTYPE[gdt], dbuf.data_ptr(), S * C + pad, C,
                      S, T, B, C, _lib.stream_ptr(DEV))
            total = sum(g.float() for g in (a, b) if g is not None)                                     # [(t * S + s), b, c]
            want = total.view(T, S, B, C).permute(2, 0, 1, 3).reshape(B * T, S * C)
            assert torch.equal(dbuf[:, :S * C], want)
            assert torch.all(dbuf[:, S * C:] == -3.25)
    # through autograd: the level-embedding gradient is the host-side sum, an unused output arrives as no gradient at all
    xg = x.detach().requires_grad_(True)
    lv = level.clone().requires_grad_(True)
    src, kin = _ClipInputs.apply(xg, lv, pos_yx, pos_z, T, torch.float32)
    g = torch.randn(T * S, B, C, generator=gen).to(DEV)
    dx, dl = torch.autograd.grad([kin], [xg, lv], [g])
    want = g.view(T, S, B, C).permute(2, 0, 3, 1).reshape(B * T, C, H, W)
    assert torch.equal(dx, want)
    torch.testing.assert_close(dl, g.sum((0, 1)), rtol=1e-5, atol=1e-4)


# ---- 3. the row rule over the clip --------------------------------------------------------------------------------------------------
def test_all_masked_row_rule_spans_the_clip_on_both_routes():
    """query 0 is open in frame 1 only: its frame 0 stays masked; query 1 is masked in every frame: it attends everywhere; query 2
    is open everywhere.  The resize is the identity here (level grid = feature grid), so both routes see the same logits."""
    from mp_former_amd import _lib
    from mp_former_amd.transformer_decoder import mask_head_bits, pool_features
    from mp_former_amd.video_decoder import clip_attn_mask_torch
    B, T, Q, C, h, w = 2, 2, 3, 256, 4, 8
    HW = h * w
    gen = torch.Generator().manual_seed(5)
    pattern = torch.where(torch.rand(B, h, w, generator=gen) < 0.5, -1.0, 1.0)
    pattern[:, 0, 0], pattern[:, 0, 1] = 1.0, -1.0                              # both signs present in every clip
    mf = torch.zeros(B, T, C, h, w)
    mf[:, 0, 0], mf[:, 1, 0] = -1.0, 1.0                                        # channel 0: the frame's sign
    mf[:, 1, 1] = pattern                                                       # channel 1: a pattern, in frame 1 only
    mf[:, :, 2] = 1.0                                                           # channel 2: one everywhere
    me = torch.zeros(Q, B, C)
    me[0, :, 0], me[0, :, 1] = 1.0, 2.0                                         # frame 0: -1; frame 1: 1 + 2 * pattern
    me[1, :, 2] = -1.0                                                          # -1 everywhere
    me[2, :, 2] = 1.0                                                           # +1 everywhere
    mf, me = mf.to(DEV).to(torch.bfloat16), me.to(DEV).to(torch.bfloat16)
    want = torch.zeros(B, Q, T, HW, dtype=torch.bool)
    want[:, 0, 0] = True
    want[:, 0, 1] = (pattern < 0).flatten(1)
    want = want.flatten(2).to(DEV)
    pooled = pool_features(mf.flatten(0, 1), (h, w)).view(B, T * HW, C)
    for _ in range(2):                                                          # second call: the flags were left clean
        got = mask_head_bits(me, pooled, None)
        assert got.shape == (B, Q, T * HW) and torch.equal(got, want)
        flags = _lib.scratch("next_mask_flags", DEV, _lib.stream_ptr(DEV), 4 * B * Q, zeroed=True)
        assert not flags.any()
    for operands in ((me, mf), (me.float(), mf.float())):
        assert torch.equal(clip_attn_mask_torch(*operands, (h, w)), want)
    # the per-plane rule of the image kernel would have opened frame 0 of query 0: this is what must not happen
    assert want[:, 0, :HW].all() and not want[:, 1].any() and not want[:, 2].any()


# ---- 4. attention masks on random data ------------------------------------------------------------------------------------------------
def _clip_reference(me, mf, size):
    """:449-458 + :409 in float64 on the given operands -> (bool [B, Q, T * HW], resized logits, resized |.| scale)"""
    B, T = mf.shape[:2]
    Q = me.shape[0]
    m = torch.einsum("qbc,btchw->bqthw", me.double(), mf.double())
    r = F.interpolate(m.flatten(0, 1), size=size, mode="bilinear", align_corners=False).view(B, Q, -1)
    am = r.sigmoid() < 0.5
    am[torch.where(am.sum(-1) == am.shape[-1])] = False
    s = torch.einsum("qbc,btchw->bqthw", me.double() ** 2, mf.double() ** 2).sqrt()
    s = F.interpolate(s.flatten(0, 1), size=size, mode="bilinear", align_corners=False).view(B, Q, -1)
    return am, r, s


@pytest.mark.parametrize("B,T,Q,hw,size", [(2, 2, 50, (16, 24), (8, 12)), (1, 3, 37, (24, 40), (12, 20))])
def test_clip_attention_masks_on_random_operands(B, T, Q, hw, size):
    """The constants and the procedure of tests/test_mask_head_gpu.py, for a clip: positions with |logit| <= 2^-7 * scale are left
    out, rows the rule could flip because of such a position too, and the differing share stays below 5e-3.  ``scale`` is the
    root of the sum of the squared terms of the logit, resized like the logit — the logit's own standard deviation for operands
    of random sign, so that the left-out share is P(|z| <= 2^-7) of a unit Gaussian times the factor by which the resize
    averages the logit down (about 2), under the asserted 2 %.  The fused head rounds the resized features to bf16: 256 terms, each
    off by at most 2^-9 of itself with random sign, move the logit by about 2^-9 / sqrt(3) * scale, so 2^-7 * scale is seven
    standard deviations of that error."""
    from mp_former_amd.transformer_decoder import mask_head_bits, pool_features
    from mp_former_amd.video_decoder import clip_attn_mask_torch
    gen = torch.Generator().manual_seed(Q)
    me = (torch.randn(Q, B, 256, generator=gen) * 0.5).to(torch.bfloat16).to(DEV)
    mf = torch.randn(B, T, 256, *hw, generator=gen).to(torch.bfloat16).to(DEV)
    me[1] = -me[1].abs()
    mf[:, :, :, :2] = mf[:, :, :, :2].abs()                                    # (a band where query 1 is masked for sure)
    HW = size[0] * size[1]
    assert (T * HW) % 16 == 0
    want, logits, scale = _clip_reference(me, mf, size)
    near = logits.abs() <= 2.0 ** -7 * scale
    assert float(near.double().mean()) <= 0.02
    rows_fragile = ((~want) & ~near).sum(-1) == 0
    pooled = pool_features(mf.flatten(0, 1), size).view(B, T * HW, 256)
    for route, got in (("fused", mask_head_bits(me, pooled, None)), ("torch", clip_attn_mask_torch(me, mf, size))):
        assert got.dtype == torch.bool and got.shape == want.shape
        diff = got != want
        bad = diff & ~near & ~rows_fragile[..., None]
        assert int(bad.sum()) == 0, f"{route}: {int(bad.sum())} mask bits differ away from zero logits (of {diff.numel()})"
        assert float(diff.float().mean()) < 5e-3, route
    assert 0.05 < float(want.float().mean()) < 0.95


# ---- 5. the whole decoder, fp32, against the reference's results ----------------------------------------------------------------------
def _fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, V.CONFIGS[name]


def _module(name, z, cfg):
    from mp_former_amd.video_decoder import VideoMultiScaleMaskedTransformerDecoder
    m = VideoMultiScaleMaskedTransformerDecoder(**V.module_kwargs(cfg))
    shapes = json.loads(str(z["param_names"]))
    m.load_state_dict(V.DP.det_state_dict(shapes, name + "."), strict=True)
    return m.to(DEV)


def _leaf(v, layout, grad):
    v = v.to(DEV)
    if layout == "channels_last":
        v = v.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return v.requires_grad_(grad)


def _run(m, name, z, cfg, tag, layout, grad):
    B, T = (cfg["B"], cfg["num_frames"]) if tag == "train" else (1, cfg["eval_frames"])
    xs, mf = V.inputs(name, cfg, int(z["seed"]), B, T)
    xs, mf = [_leaf(x, layout, grad) for x in xs], _leaf(mf, layout, grad)
    m.train(tag == "train")
    m.mask_log = []
    try:
        out = m(xs, mf)
        masks = m.mask_log
    finally:
        m.mask_log = None
    return xs, mf, out, masks


def _check_forward(z, cfg, tag, out, masks, B, T):
    Q = cfg["Q"]
    assert len(masks) == cfg["dec_layers"] + 1
    for l, am in enumerate(masks):
        hl, wl = cfg["levels"][l % 3]
        n = B * Q * T * hl * wl
        raw = torch.from_numpy(np.unpackbits(z[f"{tag}.attn{l}"])[:n].reshape(B, Q, T * hl * wl).astype(bool))
        assert torch.equal(am.cpu(), V.clip_row_rule(raw)), f"attention mask {l}"
    outs = V.outputs_list(out)
    assert out["pred_masks"].shape == (B, Q, T) + tuple(cfg["mf"]) and len(outs) == cfg["dec_layers"] + 1
    for l, (c, mk) in enumerate(outs):
        np.testing.assert_allclose(c.detach().float().cpu().numpy(), z[f"{tag}.cls"][l], rtol=5e-3, atol=2e-3, err_msg=f"class {l}")
        np.testing.assert_allclose(V.sample(mk), z[f"{tag}.masks{l}"], rtol=5e-3, atol=5e-3, err_msg=f"masks {l}")
    return outs


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("name", list(V.CONFIGS))
def test_decoder_matches_reference_golden_fp32(name, layout):
    """training mode: attention masks equal (the fixture's seed keeps every thresholded logit away from zero), logits and
    gradients within the per-tensor tolerances of test_head_gpu.test_head_matches_reference_golden_fp32.  channels_last feeds
    the pixel decoder's layout: the clip-inputs kernel runs; nchw takes the torch statement of the same.  vdec_odd: T * HW = 30 on
    level 0."""
    z, cfg = _fixture(name)
    m = _module(name, z, cfg)
    xs, mf, out, masks = _run(m, name, z, cfg, "train", layout, True)
    outs = _check_forward(z, cfg, "train", out, masks, cfg["B"], cfg["num_frames"])
    V.seeded_loss(f"{name}.train", outs).backward()
    for k, v in [(f"x{i}", x) for i, x in enumerate(xs)] + [("mf", mf)]:
        n = float(z[f"train.gradnorm.{k}"])
        np.testing.assert_allclose(v.grad.double().norm().item(), n, rtol=5e-3, err_msg=k)
        got, want = V.sample(v.grad), z[f"train.grad.{k}"]
        assert np.linalg.norm(got - want) <= 3e-3 * np.linalg.norm(want), k
    params = dict(m.named_parameters())
    for k in V.SMALL_GRADS + V.WEIGHT_GRADS:
        want = z[f"train.grad.{k}"]
        np.testing.assert_allclose(V.sample(params[k].grad), want, rtol=1e-2, atol=1e-4 + 5e-3 * np.abs(want).max(), err_msg=k)
        np.testing.assert_allclose(params[k].grad.double().norm().item(), float(z[f"train.gradnorm.{k}"]), rtol=5e-3, err_msg=k)


@pytest.mark.parametrize("amp", [False, True])
def test_level_inputs_channel_last_runs_the_kernel_and_equals_the_torch_route(amp):
    """the module's two ways to a level's (src, kin): channel-last maps take the clip-inputs kernel, NCHW maps the torch ops; same
    operation order, so the same bits, in fp32 and rounded to bf16"""
    from mp_former_amd import _lib
    z, cfg = _fixture("vdec_odd")
    m = _module("vdec_odd", z, cfg)
    B, T = cfg["B"], cfg["num_frames"]
    xs, _ = V.inputs("vdec_odd", cfg, 0, B, T)
    adt = torch.bfloat16 if amp else None
    for i, x in enumerate(xs):
        with torch.no_grad():
            a = m._level_inputs({}, i, _leaf(x, "channels_last", False), B, T, amp, adt)
            assert _lib.last_kernel() == "clip_inputs_fwd_kernel"
            b = m._level_inputs({}, i, _leaf(x, "nchw", False), B, T, amp, adt)
        for got, want in zip(a, b):
            assert got.dtype == want.dtype == (torch.bfloat16 if amp else torch.float32) and torch.equal(got, want)


def test_decoder_eval_mode_three_frames_fp32():
    """eval: bs = 1 and every frame handed over is one clip (:371-374), here T = 3 with num_frames = 2"""
    z, cfg = _fixture("vdec_small")
    m = _module("vdec_small", z, cfg)
    with torch.no_grad():
        _, _, out, masks = _run(m, "vdec_small", z, cfg, "eval", "channels_last", False)
    _check_forward(z, cfg, "eval", out, masks, 1, cfg["eval_frames"])


# ---- 6. bf16 autocast against the fp32 golden -----------------------------------------------------------------------------------------
def _amp_figures(got, want_rows):
    """(l2, med, over) of DESIGN section 2: relative L2 of the whole tensor, median over the rows of the row's relative L2, share of
    rows beyond 0.25"""
    d = (got - want_rows).reshape(want_rows.shape[0], -1)
    w = want_rows.reshape(want_rows.shape[0], -1)
    rows = np.linalg.norm(d, axis=1) / np.maximum(np.linalg.norm(w, axis=1), 1e-30)
    return float(np.linalg.norm(d) / np.linalg.norm(w)), float(np.median(rows)), float((rows > 0.25).mean())


# Worst value measured on the MI355X over the layers of the two fixtures + 30 %, the convention of DESIGN section 2 (a measured
# share of 0 gets that table's 0.01); the figures are in section 9.8.  Measured: class logits 0.0180 / 0.0129 / 0 (vdec_small,
# layer 4); gradients that pass through the layers 0.1553 (vdec_small, x2), the gradient of mask_features 0.0115 (vdec_odd).  The
# gradients of sum(seed * output) with seeds of random sign cancel heavily, rounding noise does not: the reference's own loop in
# plain torch under bf16 autocast sits 0.07 - 0.16 from the same fp32 results on the same GPU (0.016 for mask_features).
AMP_CLASS_BARS = (0.0234, 0.0168, 0.01)
AMP_MASK_L2_BAR = 0.0187
AMP_GRAD_BAR = 0.202
AMP_MF_GRAD_BAR = 0.015


@pytest.mark.parametrize("name", list(V.CONFIGS))
def test_decoder_bf16_autocast_close_to_fp32_golden(name):
    """the op-by-op route under bf16 autocast (native attention, small GEMMs, residual LayerNorm, fused mask head where
    T * HW % 16 == 0): class logits of every layer by (l2, med, over) over the (clip, query) rows, gradients by relative L2"""
    from mp_former_amd import _lib
    z, cfg = _fixture(name)
    m = _module(name, z, cfg)
    _lib.profile_enable(True)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            xs, mf, out, masks = _run(m, name, z, cfg, "train", "channels_last", True)
        assert _lib.profile_get("attn_fwd")[0] >= 2 * cfg["dec_layers"], _lib.last_kernel()
        assert _lib.profile_get("mask_head_bits")[0] >= 1, "the fused mask head did not run"
    finally:
        _lib.profile_enable(False)
    outs = V.outputs_list(out)
    worst = [0.0, 0.0, 0.0]
    for l, (c, _) in enumerate(outs):
        want = z["train.cls"][l]
        fig = _amp_figures(c.detach().float().cpu().numpy().reshape(-1, want.shape[-1]), want.reshape(-1, want.shape[-1]))
        print(f"{name} layer {l} class l2/med/over {fig[0]:.4f} {fig[1]:.4f} {fig[2]:.4f}")
        worst = [max(a, b) for a, b in zip(worst, fig)]
    worst_m = 0.0
    for l, (_, mk) in enumerate(outs):                  # (the fixture holds a strided sample of the mask logits: whole-sample L2)
        got, want = V.sample(mk), z[f"train.masks{l}"]
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        print(f"{name} layer {l} masks l2 {rel:.4f}")
        worst_m = max(worst_m, rel)
    assert worst_m <= AMP_MASK_L2_BAR, worst_m
    V.seeded_loss(f"{name}.train", outs).backward()
    params = dict(m.named_parameters())
    grads = {f"x{i}": x.grad for i, x in enumerate(xs)}
    grads["mf"] = mf.grad
    grads.update({k: params[k].grad for k in V.SMALL_GRADS + V.WEIGHT_GRADS})
    worst_g = 0.0
    for k, g in grads.items():
        got, want = V.sample(g), z[f"train.grad.{k}"]
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        print(f"{name} grad {k} l2 {rel:.4f}")
        if k == "mf":
            mf_rel = rel
        else:
            worst_g = max(worst_g, rel)
    print(f"{name} worst class l2/med/over {worst[0]:.4f} {worst[1]:.4f} {worst[2]:.4f} worst grad l2 {worst_g:.4f}")
    assert all(a <= b for a, b in zip(worst, AMP_CLASS_BARS)), worst
    assert worst_g <= AMP_GRAD_BAR, worst_g
    assert mf_rel <= AMP_MF_GRAD_BAR, mf_rel


# ---- 7. hand-over to the clip criterion -----------------------------------------------------------------------------------------------
def test_training_outputs_go_through_the_clip_criterion_in_place():
    from mp_former_amd.point_sample import MapSet
    from mp_former_amd.video_losses import VideoHungarianMatcher, VideoSetCriterion, clip_planes
    name = "vdec_small"
    z, cfg = _fixture(name)
    m = _module(name, z, cfg)
    B, T, Q, K = cfg["B"], cfg["num_frames"], cfg["Q"], cfg["K"]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        xs, mf, out, _ = _run(m, name, z, cfg, "train", "channels_last", False)
    outs = V.outputs_list(out)
    # one parent: every layer's masks are a dim-1 slice of the same [B, L * Q, T, h, w] memory, and clip_planes is a view of it
    planes = [clip_planes(mk) for _, mk in outs]
    assert all(p.data_ptr() == mk.data_ptr() for p, (_, mk) in zip(planes, outs))
    ms = MapSet(planes)
    assert len(ms.bases) == 1 and ms.bases[0].shape[1] == len(outs) * Q * T
    assert sorted(int(q) for q in ms.q0) == [l * Q * T for l in range(len(outs))]
    H, Wd = 4 * cfg["mf"][0], 4 * cfg["mf"][1]
    gen = torch.Generator().manual_seed(11)
    targets = []
    for b in range(B):
        masks = torch.zeros(3, T, H, Wd, dtype=torch.bool)
        for g in range(3):
            y0, x0 = int(torch.randint(0, H // 2, (1,), generator=gen)), int(torch.randint(0, Wd // 2, (1,), generator=gen))
            masks[g, :, y0:y0 + H // 3, x0:x0 + Wd // 3] = True
        targets.append({"labels": torch.randint(0, K, (3,), generator=gen).to(DEV), "ids": torch.arange(3).repeat(T, 1).t().to(DEV),
                        "masks": masks.to(DEV)})
    base = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0}
    wd = dict(base)
    for i in range(len(outs) - 1):
        wd.update({k + f"_{i}": v for k, v in base.items()})
    matcher = VideoHungarianMatcher(cost_class=2.0, cost_mask=5.0, cost_dice=5.0, num_points=200)
    crit = VideoSetCriterion(K, matcher=matcher, weight_dict=wd, eos_coef=0.1, losses=["labels", "masks"], num_points=200,
                             oversample_ratio=3.0, importance_sample_ratio=0.75).to(DEV)
    torch.manual_seed(3)
    losses = crit(out, targets)
    assert sorted(losses) == sorted(wd)
    total = sum(losses[k] * wd[k] for k in wd)
    assert torch.isfinite(total)
    total.backward()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    assert float(m.query_embed.weight.grad.abs().max()) > 0


# ---- 8. install_native_video_decoder --------------------------------------------------------------------------------------------------
class _Layer(nn.Module):
    def __init__(self, **mods):
        super().__init__()
        self.normalize_before = False
        for k, v in mods.items():
            setattr(self, k, v)


class _ReferenceFields(nn.Module):
    """what install_native_video_decoder reads of the reference module: its fields and its state dict (no forward)"""

    def __init__(self, cfg):
        super().__init__()
        C, H = cfg["hidden"], cfg["heads"]
        self.mask_classification, self.num_frames = True, cfg["num_frames"]
        self.num_heads, self.num_layers, self.num_queries = H, cfg["dec_layers"], cfg["Q"]
        self.transformer_self_attention_layers = nn.ModuleList(
            _Layer(self_attn=nn.MultiheadAttention(C, H), norm=nn.LayerNorm(C)) for _ in range(cfg["dec_layers"]))
        self.transformer_cross_attention_layers = nn.ModuleList(
            _Layer(multihead_attn=nn.MultiheadAttention(C, H), norm=nn.LayerNorm(C)) for _ in range(cfg["dec_layers"]))
        self.transformer_ffn_layers = nn.ModuleList(
            _Layer(linear1=nn.Linear(C, cfg["ffn"]), linear2=nn.Linear(cfg["ffn"], C), norm=nn.LayerNorm(C)) for _ in range(cfg["dec_layers"]))
        self.decoder_norm = nn.LayerNorm(C)
        self.query_feat, self.query_embed, self.level_embed = nn.Embedding(cfg["Q"], C), nn.Embedding(cfg["Q"], C), nn.Embedding(3, C)
        self.input_proj = nn.ModuleList(nn.Sequential() for _ in range(3))
        self.class_embed = nn.Linear(C, cfg["K"] + 1)
        self.mask_embed = _Layer(layers=nn.ModuleList(nn.Linear(C, C) for _ in range(3)))


def test_install_native_video_decoder_on_reference_fields():
    from mp_former_amd import d2_plugin
    from mp_former_amd.video_decoder import VideoMultiScaleMaskedTransformerDecoder
    name = "vdec_small"
    z, cfg = _fixture(name)
    old = _ReferenceFields(cfg)
    shapes = json.loads(str(z["param_names"]))
    assert {k: list(v.shape) for k, v in old.state_dict().items()} == shapes
    old.load_state_dict(V.DP.det_state_dict(shapes, name + "."), strict=True)
    old.to(DEV).eval()
    model = NS(sem_seg_head=NS(predictor=old))
    new = d2_plugin.install_native_video_decoder(model)
    assert model.sem_seg_head.predictor is new and isinstance(new, VideoMultiScaleMaskedTransformerDecoder) and not new.training
    assert new.num_frames == cfg["num_frames"] and new.num_layers == cfg["dec_layers"] and new.num_heads == cfg["heads"]
    assert new.transformer_ffn_layers[0].linear1.out_features == cfg["ffn"] and next(new.parameters()).device == DEV
    for k, v in old.state_dict().items():
        assert torch.equal(new.state_dict()[k], v), k
    with torch.no_grad():
        _, _, out, masks = _run(new, name, z, cfg, "eval", "channels_last", False)
    _check_forward(z, cfg, "eval", out, masks, 1, cfg["eval_frames"])
