"""Masked-attention transformer decoder with mask-piloted (MP) queries — host-side mirror of
``MultiScaleMaskedTransformerDecoderMaskDN`` (dn_mode="points"), reference:
mask2former/modeling/transformer_decoder/mask2former_transformer_decoder.py
  :19-206   SelfAttentionLayer / CrossAttentionLayer / FFNLayer / MLP
  :558-727  constructor, from_config          :729-735  prepare_for_normal
  :968-1060 prepare_for_dn_v5 (MP queries)    :1584-1622 gen_mask_dn
  :1706-1857 forward                           :1859-1877 forward_prediction_heads

Same parameter names (checkpoints load unchanged), same forward signature and output dict.
Differences that do not change results:
  * the boolean attention mask is kept as ONE [N, Qtot, HW] tensor shared by the 8 heads (the
    reference materialises the 8x repeat, :1873); with HEAD_DN False the rows are identical;
  * the "all-masked row -> unmask" rule (:1780) and the MP-row overwrite (:1814-1816) are applied
    by the attention-mask builder instead of by in-place edits of the repeated tensor;
  * ground-truth masks are OR-reduced to the 3 level sizes once per forward (A.5: area <= 1e-8 is
    "no GT pixel in the block") instead of 10 area-interpolations;
  * hard-coded .cuda() / 8 heads of the reference become the module's device / num_heads.
Only dn_mode "points" is implemented (other modes and HEAD_DN raise), with or without point noise on the MP rows:
NOISE_SCALE 0 (the shipped run script) builds the rows once per forward; NOISE_SCALE > 0 (the DN_query configs) makes each
mask's rows with one native launch (``mp_noise_rows``, csrc/mp_noise.hip), the flips drawn by a counter-based generator keyed by
the device generator's seed and offset.  The torch ops of the reference remain as ``noisy_rows`` for the tests, which feed them
recorded draws through ``_rng.install_replay``.
"""
import math
import ctypes
import os
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _lib, _rng, mask_fused
from ._h2d import upload
from ._targets import stacked_masks
from .attention import attention_core
from .resln import res_ln
from .small_linear import small_linear, tall_linear, tall_usable as _tall_ok, usable as _small_ok
from .decoder_layer import decoder_layer, split_cols
from .pixel_decoder import PositionEmbeddingSine, _ConvNorm, _c2_xavier_fill




class _CastParams(torch.autograd.Function):
    """bf16 working copies of a list of fp32 parameters in ONE multi-tensor launch (and one for the
    gradients on the way back) instead of one cast kernel per parameter per use, which is what
    autocast does (~280 cast launches forward and ~630 backward per decoder step).  Same numerics as
    autocast: weights rounded to bf16 for the GEMMs, weight gradients produced in bf16 and accumulated
    into the fp32 .grad.

    ``chunks[i]`` > 1 returns parameter i as that many separate row blocks (the q / k / v parts of a
    packed in-projection): the consumer never slices, so the backward has no zero-fill + copy + add
    per slice — the block gradients are copied straight into one fp32 gradient."""

    @staticmethod
    def forward(ctx, dtype, chunks, *params):
        # ONE buffer for all copies (256-byte slots; layout cached per list of shapes) and one view per parameter: ~230
        # allocations per direction were 0.5 ms of launch-thread time each way, at the two places of the step where the GPU
        # has caught up with the host (end of the pixel decoder forward / end of the decoder backward)
        dev = params[0].device
        dt = dtype if dtype is not None else params[0].dtype
        offs, tot, strides = _flat_layout(tuple(p.shape for p in params))
        if dtype is None and any(p.dtype != dt for p in params):
            raise RuntimeError("_CastParams without a target dtype needs parameters of one dtype")
        flat = torch.empty(tot, dtype=dt, device=dev)
        dsts, outs = [], []
        for p, c, o, st in zip(params, chunks, offs, strides):
            full = flat.as_strided(p.shape, st, o)
            dsts.append(full)
            # row blocks of ONE buffer: the blocks of a packed in-projection stay side by side in memory (the native
            # decoder layer then runs q | k | v as one GEMM)
            outs += [full] if c == 1 else list(full.chunk(c, 0))
        torch._foreach_copy_(dsts, list(params))
        ctx.chunks = chunks
        ctx.shapes = tuple(p.shape for p in params)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        res, dsts, srcs = [], [], []
        dev = next((g for g in grads if g is not None), None)
        if dev is None:
            return (None, None) + (None,) * len(ctx.shapes)
        offs, tot, strides = _flat_layout(ctx.shapes)
        flat = torch.empty(tot, dtype=torch.float32, device=dev.device)
        k = 0
        for shape, c, o, st in zip(ctx.shapes, ctx.chunks, offs, strides):
            gs = grads[k:k + c]
            k += c
            if c == 1:
                if gs[0] is None:
                    res.append(None)
                    continue
                full = flat.as_strided(shape, st, o)
                dsts.append(full)
                srcs.append(gs[0])
                res.append(full)
                continue
            if all(g is None for g in gs):
                res.append(None)
                continue
            full = flat.as_strided(shape, st, o)
            for part, g in zip(full.chunk(c, 0), gs):
                if g is None:
                    part.zero_()
                else:
                    dsts.append(part)
                    srcs.append(g)
            res.append(full)
        if dsts:
            torch._foreach_copy_(dsts, srcs)
        return (None, None, *res)


_flat_layouts = {}


def _flat_layout(shapes):
    """(element offsets in 64-element slots, total, contiguous strides) of tensors of the given shapes inside one flat buffer"""
    hit = _flat_layouts.get(shapes)
    if hit is None:
        offs, strides, tot = [], [], 0
        for s_ in shapes:
            offs.append(tot)
            tot += (s_.numel() + 63) & ~63
            st, acc = [], 1
            for d in reversed(s_):
                st.append(acc)
                acc *= d
            strides.append(tuple(reversed(st)))
        if len(_flat_layouts) > 16:
            _flat_layouts.clear()
        hit = _flat_layouts[shapes] = (tuple(offs), tot, tuple(strides))
    return hit


class _GatherRows(torch.autograd.Function):
    """Row-wise concatenations of groups of tensors in ONE multi-tensor launch: ``sizes[g]`` consecutive inputs form
    output g.  The gradient of an input is a row-block VIEW of its output's gradient (no launch).  Used to put the key
    (value) projection weights of the decoder layers that share a feature level side by side."""

    @staticmethod
    def forward(ctx, sizes, *ts):
        outs, dsts, k = [], [], 0
        for n in sizes:
            grp = ts[k:k + n]
            k += n
            full = torch.empty((sum(t.shape[0] for t in grp),) + tuple(grp[0].shape[1:]), dtype=grp[0].dtype, device=grp[0].device)
            r = 0
            for t in grp:
                dsts.append(full[r:r + t.shape[0]])
                r += t.shape[0]
            outs.append(full)
        torch._foreach_copy_(dsts, [t.detach() for t in ts])
        ctx.sizes, ctx.rows = sizes, [t.shape[0] for t in ts]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gs):
        res, k = [], 0
        for n, g in zip(ctx.sizes, gs):
            r = 0
            for rows in ctx.rows[k:k + n]:
                res.append(None if g is None else g[r:r + rows])
                r += rows
            k += n
        return (None, *res)


class _DecoderInputs(torch.autograd.Function):
    """(src, kin) [S, N, C] of one feature level from its map x [N, C, H, W] (a channel-last view), the level
    embedding row and the [S, C] sine position embedding — one native pass each way (csrc/decoder.hip;
    mask2former_transformer_decoder.py:1756-1764)."""

    @staticmethod
    def forward(ctx, x, level_row, pos_t, out_dtype):
        N, C, H, W = x.shape
        S = H * W
        src = torch.empty((S, N, C), dtype=out_dtype, device=x.device)
        kin = torch.empty((S, N, C), dtype=out_dtype, device=x.device)
        dt = _lib.MPF_BF16 if out_dtype == torch.bfloat16 else _lib.MPF_F32
        _lib.call("mpf_decoder_inputs_forward", x.device, x.data_ptr(), x.stride(0), x.stride(3), level_row.data_ptr(), pos_t.data_ptr(),
                  src.data_ptr(), kin.data_ptr(), dt, S, N, C, _lib.stream_ptr(x.device))
        ctx.dims = (N, C, H, W)
        return src, kin

    @staticmethod
    def backward(ctx, g_src, g_kin):
        N, C, H, W = ctx.dims
        S = H * W
        g = g_src if g_src is not None else g_kin
        if g_src is not None and g_kin is not None and g_src.dtype != g_kin.dtype:
            g_src, g_kin = g_src.float(), g_kin.float()
            g = g_src
        if g.dtype not in (torch.float32, torch.bfloat16):
            g_src = g_src.float() if g_src is not None else None
            g_kin = g_kin.float() if g_kin is not None else None
            g = g_src if g_src is not None else g_kin
        g_src = g_src.contiguous() if g_src is not None else None
        g_kin = g_kin.contiguous() if g_kin is not None else None
        mem = torch.empty((N, S, C), dtype=torch.float32, device=g.device)       # channel-last, like the input view
        dt = _lib.MPF_BF16 if g.dtype == torch.bfloat16 else _lib.MPF_F32
        _lib.call("mpf_decoder_inputs_backward", g.device, _lib.ptr(g_src), _lib.ptr(g_kin), dt, mem.data_ptr(),
                  S * C, C, S, N, C, _lib.stream_ptr(g.device))
        dx = mem.permute(0, 2, 1).view(N, C, H, W)
        d_level = mem.sum((0, 1)) if ctx.needs_input_grad[1] else None
        return dx, d_level, None, None


def native_attn_mask(masks, size, mp_rows=None):
    """[N,Qtot,h,w] mask logits (f32/bf16) -> bool [N,Qtot,hl*wl] attention mask of the next layer:
    bilinear resize + (< 0) + MP-row overwrite + all-masked-row rule in one native kernel
    (csrc/decoder.hip; decoder :1869-1875, :1814-1816, :1780)."""
    if not masks.is_cuda:
        raise RuntimeError("mp_former_amd decoder runs on the GPU only (no CPU fallback)")
    N, Q, h, w = masks.shape
    hl, wl = size
    if masks.stride(3) != 1 or masks.stride(2) != w:
        masks = masks.contiguous()
    if masks.dtype not in (torch.float32, torch.bfloat16):
        masks = masks.float()
    pad = 0 if mp_rows is None else mp_rows.shape[1]
    if pad:
        mp_rows = mp_rows.contiguous()
    out = torch.empty((N, Q, hl * wl), dtype=torch.bool, device=masks.device)
    _lib.call("mpf_attn_mask", masks.device, masks.data_ptr(), _lib.DTYPE[masks.dtype], masks.stride(0), masks.stride(1), h, w,
              mp_rows.data_ptr() if pad else None, pad, out.data_ptr(), N, Q, hl, wl, _lib.stream_ptr(masks.device))
    return out


def pool_features(mask_features, size):
    """F.interpolate(mask_features [N,256,h,w], size, mode="bilinear", align_corners=False) as a pixel-major bf16
    matrix [N, hl*wl, 256] — the B operand of the fused mask head (csrc/mask_head.hip).  Once per step and level."""
    N, C, h, w = mask_features.shape
    hl, wl = size
    dt = _lib.DTYPE[mask_features.dtype]
    out = torch.empty((N, hl * wl, C), dtype=torch.bfloat16, device=mask_features.device)
    stream = _lib.stream_ptr(mask_features.device)
    if _is_planes(mask_features) and not mask_features.is_contiguous():
        # channel-last features (the pixel decoder's layout): no transpose needed
        _lib.call("mpf_pool_features_cl", mask_features.device, mask_features.data_ptr(), mask_features.stride(0), dt, out.data_ptr(),
                  N, C, h, w, hl, wl, stream)
        return out
    mf = mask_features if mask_features.is_contiguous() else mask_features.contiguous()
    _lib.call("mpf_pool_features", mf.device, mf.data_ptr(), dt, out.data_ptr(), N, C, h, w, hl, wl, stream)
    return out


def _is_planes(x):
    """[N, C, H, W] whose images are dense [H*W, C] planes (channels_last), 16-byte aligned."""
    return (x.dim() == 4 and x.stride(1) == 1 and x.stride(3) == x.shape[1] and x.stride(2) == x.shape[3] * x.shape[1]
            and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0)


def mask_product(me, mask_features):
    """outputs_mask = einsum("bqc,bchw->bqhw", mask_embed, mask_features) (decoder :1869).  bf16 operands with channel-last
    features (the AMP path) run on the native MFMA product (csrc/mask_fused.hip, forward and both gradients); anything else
    is the library einsum."""
    if me.is_cuda and me.dtype == mask_features.dtype and mask_fused.supported(me, mask_features):
        amp = torch.is_autocast_enabled()
        if not amp or me.dtype == torch.get_autocast_dtype("cuda"):      # operands already in the dtype autocast would pick
            with torch.autocast(device_type="cuda", enabled=False):
                return mask_fused.full_product(me, mask_features)
    return torch.einsum("bqc,bchw->bqhw", me, mask_features)


class MpfNextMask(ctypes.Structure):
    """include/mpformer_hip.h MpfNextMask"""
    _fields_ = [(n, ctypes.c_void_p) for n in ("x", "ln_gamma", "ln_beta", "w0", "b0", "w1", "b1", "w2", "b2", "pooled", "mp_rows",
                                                "out", "flags", "scratch")] + \
               [("scratch_bytes", ctypes.c_size_t), ("N", ctypes.c_int), ("Q", ctypes.c_int), ("HW", ctypes.c_int),
                ("pad", ctypes.c_int), ("eps", ctypes.c_float)]


def next_attn_mask_native(x, norm, mlp, pooled, mp_rows=None):
    """bool [N, Q, HW] attention mask of the next layer from the residual stream x fp32 [Q, N, 256]: decoder_norm, the
    three mask_embed layers (``mlp`` = [(w, b)] x 3, bf16) and the fused mask head as ONE native call
    (``mpf_next_attn_mask``; same five launches as res_ln + 3 x linear + mask_head_bits, bit-identical)."""
    Q, N, C = x.shape
    HW = pooled.shape[1]
    dev = x.device
    pad = 0 if mp_rows is None else mp_rows.shape[1]
    if pad:
        mp_rows = mp_rows.contiguous()
    stream = _lib.stream_ptr(dev)
    flags = _lib.scratch("next_mask_flags", dev, stream, 4 * N * Q, zeroed=True)       # zero on entry, zeroed again by the kernel
    sc = _lib.scratch("next_mask", dev, stream, _lib.lib().mpf_next_attn_mask_scratch_bytes(N, Q))
    out = torch.empty((N, Q, HW), dtype=torch.bool, device=dev)
    m = MpfNextMask()
    m.x, m.ln_gamma, m.ln_beta, m.eps = x.data_ptr(), norm.weight.data_ptr(), norm.bias.data_ptr(), float(norm.eps)
    (w0, b0), (w1, b1), (w2, b2) = mlp
    m.w0, m.b0, m.w1, m.b1, m.w2, m.b2 = w0.data_ptr(), b0.data_ptr(), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr()
    m.pooled, m.mp_rows, m.out, m.flags = pooled.data_ptr(), (mp_rows.data_ptr() if pad else None), out.data_ptr(), flags.data_ptr()
    m.scratch, m.scratch_bytes = sc.data_ptr(), sc.numel()
    m.N, m.Q, m.HW, m.pad = N, Q, HW, pad
    _lib.call("mpf_next_attn_mask", dev, ctypes.byref(m), stream)
    return out


def mask_head_bits(mask_embed, pooled, mp_rows=None):
    """mask_embed bf16 [Qtot, N, 256] (sequence-first, as the MLP leaves it) x pooled [N, HW, 256] -> bool [N, Qtot, HW]
    attention mask of the next layer: sign of the product (sigmoid < 0.5), MP rows, all-masked-row rule
    (decoder :1869-1875, :1814-1816, :1780) without ever forming the [N, Qtot, H/4, W/4] map."""
    Q, N, C = mask_embed.shape
    HW = pooled.shape[1]
    assert mask_embed.dtype == torch.bfloat16 and pooled.dtype == torch.bfloat16 and mask_embed.stride(2) == 1
    pad = 0 if mp_rows is None else mp_rows.shape[1]
    if pad:
        mp_rows = mp_rows.contiguous()
    dev = mask_embed.device
    stream = _lib.stream_ptr(dev)
    flags = _lib.scratch("next_mask_flags", dev, stream, 4 * N * Q, zeroed=True)       # zero on entry, zeroed again by the kernel
    out = torch.empty((N, Q, HW), dtype=torch.bool, device=dev)
    _lib.call("mpf_mask_head_bits", dev, mask_embed.data_ptr(), mask_embed.stride(1), mask_embed.stride(0), pooled.data_ptr(),
              mp_rows.data_ptr() if pad else None, pad, out.data_ptr(), flags.data_ptr(), N, Q, HW, stream)
    return out


def linear(x, w, b=None, relu=False):
    """relu?(F.linear(x, w, b)).  bf16 activations with a few hundred rows (the query side of the decoder
    under autocast) run on the small-row MFMA GEMM with the ReLU / its backward gate / the bias gradient
    fused (small_linear.py); everything else is the library GEMM."""
    if _small_ok(x, w, b):
        return small_linear(x, w, b, relu)
    if not relu and _tall_ok(x, w, b):
        return tall_linear(x, w, b)         # library forward / dX, native split-over-rows weight gradient
    y = F.linear(x, w, b)
    return F.relu(y) if relu else y


def _class_linear(x, w, b):
    """class_embed over the batched residual streams (mask2former_transformer_decoder.py:1862): K + 1 = 81 outputs is not a
    multiple of the native GEMM's 4-column / 32-deep granules, so weight and bias are zero-padded to 96 rows — forward, input
    gradient (contraction over the 96 padded outputs, whose gradient is zero) and weight gradient then run on the native tall
    kernels like every other Linear of the heads; the pad rows are sliced off again (autograd pads / slices the gradients)."""
    n, K = w.shape
    rows = x.numel() // max(K, 1)
    if not (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and b is not None and b.dtype == torch.bfloat16
            and n % 32 and K % 32 == 0 and rows > 1024):
        return F.linear(x, w, b)
    pad = (-n) % 32
    # (contiguous: the criterion's class-loss kernels address the logits as dense [rows, K + 1])
    return tall_linear(x, F.pad(w, (0, 0, 0, pad)), F.pad(b, (0, pad)))[..., :n].contiguous()


def masked_mha_w(q_in, k_in, v_in, w, b, wo, bo, nheads, mask: Optional[Tensor]):
    """Multi-head attention with in-projection (w, b) and out-projection (wo, bo), seq-first.
    q_in [Lq,N,E]; k_in, v_in [Lk,N,E]; mask bool, True = masked: [N,Lq,Lk] (shared by heads) or
    [Lq,Lk]; returns [Lq,N,E].  ``w`` / ``b`` are either the packed [3E,E] / [3E] parameters or
    3-tuples of their q / k / v row blocks (see _CastParams).  Self-attention (q_in is k_in is v_in)
    with packed weights runs ONE in-projection GEMM.  The projections are library GEMMs;
    softmax(QK^T/sqrt(hd))V runs on the native bf16 MFMA kernels (csrc/attn.hip), fp32 softmax."""
    E = q_in.shape[-1]
    if not isinstance(w, (tuple, list)) and q_in is k_in and k_in is v_in:
        q, k, v = F.linear(q_in, w, b).split(E, dim=-1)
    else:
        if not isinstance(w, (tuple, list)):
            w, b = (w[:E], w[E:2 * E], w[2 * E:]), (b[:E], b[E:2 * E], b[2 * E:])
        q = linear(q_in, w[0], b[0])
        k = linear(k_in, w[1], b[1])
        v = linear(v_in, w[2], b[2])
    o = attention_core(q, k, v, mask, nheads)
    return linear(o, wo, bo)


def masked_mha(q_in, k_in, v_in, mha: nn.MultiheadAttention, mask: Optional[Tensor]):
    return masked_mha_w(q_in, k_in, v_in, mha.in_proj_weight, mha.in_proj_bias, mha.out_proj.weight,
                        mha.out_proj.bias, mha.num_heads, mask)


class SelfAttentionLayer(nn.Module):
    def __init__(self, d_model, nhead, dropout=0.0, activation="relu", normalize_before=False):
        super().__init__()
        assert not normalize_before and dropout == 0.0, "post-norm, dropout 0 (PRE_NORM False) only"
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.norm = nn.LayerNorm(d_model)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, tgt, tgt_mask=None, tgt_key_padding_mask=None, query_pos=None):
        assert tgt_key_padding_mask is None and query_pos is None
        return self.norm(tgt + masked_mha(tgt, tgt, tgt, self.self_attn, tgt_mask))


class CrossAttentionLayer(nn.Module):
    def __init__(self, d_model, nhead, dropout=0.0, activation="relu", normalize_before=False):
        super().__init__()
        assert not normalize_before and dropout == 0.0
        self.multihead_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.norm = nn.LayerNorm(d_model)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, tgt, memory, memory_mask=None, memory_key_padding_mask=None, pos=None, query_pos=None,
                memory_plus_pos=None):
        assert memory_key_padding_mask is None and query_pos is None
        k_in = memory_plus_pos if memory_plus_pos is not None else (memory if pos is None else memory + pos)
        return self.norm(tgt + masked_mha(tgt, k_in, memory, self.multihead_attn, memory_mask))


class FFNLayer(nn.Module):
    def __init__(self, d_model, dim_feedforward=2048, dropout=0.0, activation="relu", normalize_before=False):
        super().__init__()
        assert not normalize_before and dropout == 0.0
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm = nn.LayerNorm(d_model)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, tgt):
        return self.norm(tgt + self.linear2(F.relu(self.linear1(tgt))))


class MLP(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = F.relu(layer(x)) if i < self.num_layers - 1 else layer(x)
        return x


def gt_block_or(masks: Tensor, size):
    """A.5: 'masked' rows of the MP queries = no ground-truth pixel inside the (H/h)x(W/w) block
    (== F.interpolate(mode='area') <= 1e-8 of :986-987 when H % h == 0).  masks [T,H,W] bool/float
    -> [T, h*w] bool, True = do not attend."""
    T, H, W = masks.shape
    h, w = size
    if H % h or W % w:
        return F.interpolate(masks.float().unsqueeze(1), size=size, mode="area").flatten(1) <= 1e-8
    m = masks if masks.dtype == torch.bool else masks > 0
    if not m.is_cuda:
        raise RuntimeError("mp_former_amd decoder runs on the GPU only (no CPU fallback)")
    m = m.contiguous()
    out = torch.empty((T, h * w), dtype=torch.bool, device=m.device)
    _lib.call("mpf_mask_block_empty", m.device, m.data_ptr(), out.data_ptr(), T, H, W, h, w, _lib.stream_ptr(m.device))
    return out


def mp_open_counts(base: Tensor) -> Tensor:
    """``areas`` of :995 / :1610: base [R, HW] bool (True = do not attend) -> the number of open positions per row, int32 [R]."""
    if not base.is_cuda:
        raise RuntimeError("mp_former_amd decoder runs on the GPU only (no CPU fallback)")
    base = base.contiguous()
    R, HW = base.shape
    counts = torch.empty(R, dtype=torch.int32, device=base.device)
    _lib.call("mpf_mp_open_counts", base.device, base.data_ptr(), R, HW, counts.data_ptr(), _lib.stream_ptr(base.device))
    return counts


def mp_noise_rows(base: Tensor, src_of: Tensor, N: int, pad: int, noise_scale: float, seed: int, draw: int,
                  counts: Optional[Tensor] = None) -> Tensor:
    """One attention mask's worth of mask-piloted rows with point noise (:985-998, :1599-1620), one native launch.
    base [R, HW] bool (the GT rows of the level, True = do not attend), src_of [N * pad] int32 (for each output row the row of
    ``base`` it shows, -1 = empty slot -> all True) -> [N, pad, HW] bool.  Each position of row r flips with probability
    counts[r] * noise_scale / HW; the flips are the function of (seed, draw, r, position) that include/mpformer_hip.h defines.
    ``counts``: mp_open_counts(base) if the caller already has it (it does not change within a forward)."""
    if not base.is_cuda:
        raise RuntimeError("mp_former_amd decoder runs on the GPU only (no CPU fallback)")
    base = base.contiguous()
    R, HW = base.shape
    if counts is None:
        counts = mp_open_counts(base)
    assert base.dtype == torch.bool and counts.dtype == torch.int32 and counts.numel() == R and counts.is_contiguous()
    assert src_of.dtype == torch.int32 and src_of.numel() == N * pad and src_of.is_contiguous()
    assert src_of.device == base.device and counts.device == base.device
    out = torch.empty((N, pad, HW), dtype=torch.bool, device=base.device)
    mask64 = (1 << 64) - 1
    _lib.call("mpf_mp_noise_rows", base.device, base.data_ptr(), counts.data_ptr(), src_of.data_ptr(), R, HW, N, pad, float(noise_scale),
              int(seed) & mask64, int(draw) & mask64, out.data_ptr(), _lib.stream_ptr(base.device))
    return out


def _next_noise_draw(device):
    """(seed, draw) of the next noised mask, from the CUDA generator of ``device``: its seed, and its Philox offset as the draw
    number, advanced by 4 (the generator's own granularity) per mask.  ``torch.manual_seed`` and a saved / restored generator
    state therefore reproduce the masks.  Host-side state only: no device synchronisation."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[idx]
    draw = gen.get_offset()
    gen.set_offset(draw + 4)
    return gen.initial_seed(), draw


class MultiScaleMaskedTransformerDecoderMaskDN(nn.Module):
    _version = 2

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                              error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version < 2:   # decoder :562-583
            for k in list(state_dict.keys()):
                if "static_query" in k:
                    state_dict[k.replace("static_query", "query_feat")] = state_dict.pop(k)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                      error_msgs)

    def __init__(self, in_channels, mask_classification=True, *, num_classes: int, hidden_dim: int,
                 num_queries: int, nheads: int, dim_feedforward: int, dec_layers: int, pre_norm: bool,
                 mask_dim: int, enforce_input_project: bool, dn_mode="base", head_dn=False, all_lys=False,
                 dn_ratio=0.5, dn_label_noise_ratio=-1.0):
        super().__init__()
        assert mask_classification, "Only support mask classification model"
        if dn_mode != "points":
            raise NotImplementedError("only dn_mode='points' (the shipped MP-Former configuration) is implemented")
        if head_dn:
            raise NotImplementedError("HEAD_DN True is not part of the shipped configuration")
        self.mask_classification = mask_classification
        self.head_dn, self.dn_ratio = head_dn, dn_ratio
        self.pe_layer = PositionEmbeddingSine(hidden_dim // 2, normalize=True)
        self._pos_t = {}            # [S, C] transposes of the cached position embeddings, per (H, W, device)
        self.dn_label_noise_ratio = dn_label_noise_ratio
        self.num_heads, self.num_classes, self.num_layers = nheads, num_classes, dec_layers
        self.dn_mode = dn_mode
        self.transformer_self_attention_layers = nn.ModuleList()
        self.transformer_cross_attention_layers = nn.ModuleList()
        self.transformer_ffn_layers = nn.ModuleList()
        for _ in range(self.num_layers):
            self.transformer_self_attention_layers.append(SelfAttentionLayer(hidden_dim, nheads, 0.0, normalize_before=pre_norm))
            self.transformer_cross_attention_layers.append(CrossAttentionLayer(hidden_dim, nheads, 0.0, normalize_before=pre_norm))
            self.transformer_ffn_layers.append(FFNLayer(hidden_dim, dim_feedforward, 0.0, normalize_before=pre_norm))
        self.decoder_norm = nn.LayerNorm(hidden_dim)
        self.num_queries = num_queries
        self.query_feat = nn.Embedding(num_queries, hidden_dim)
        self.num_feature_levels = 3
        self.level_embed = nn.Embedding(self.num_feature_levels, hidden_dim)
        self.input_proj = nn.ModuleList()
        for _ in range(self.num_feature_levels):
            if in_channels != hidden_dim or enforce_input_project:
                self.input_proj.append(_ConvNorm(in_channels, hidden_dim, kernel_size=1))
                _c2_xavier_fill(self.input_proj[-1])
            else:
                self.input_proj.append(nn.Sequential())
        self.class_embed = nn.Linear(hidden_dim, num_classes + 1)
        self.mask_embed = MLP(hidden_dim, hidden_dim, mask_dim, 3)
        self.label_enc = nn.Embedding(num_classes, hidden_dim)
        self.all_lys = all_lys
        # True: in training mode "pred_masks" are mask_fused.FactoredMasks (for mp_former_amd's SetCriterion, which samples
        # them from the factors); False (the reference interface): materialised [N, Q, H/4, W/4] tensors
        self.factored_masks = False

    @classmethod
    def from_config(cls, cfg, in_channels, mask_classification):
        """decoder :697-727 (detectron2 CfgNode)."""
        mf = cfg.MODEL.MASK_FORMER
        assert mf.DEC_LAYERS >= 1
        return dict(in_channels=in_channels, mask_classification=mask_classification,
                    num_classes=cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES, hidden_dim=mf.HIDDEN_DIM,
                    num_queries=mf.NUM_OBJECT_QUERIES, nheads=mf.NHEADS, dim_feedforward=mf.DIM_FEEDFORWARD,
                    dec_layers=mf.DEC_LAYERS - 1, pre_norm=mf.PRE_NORM, enforce_input_project=mf.ENFORCE_INPUT_PROJ,
                    mask_dim=cfg.MODEL.SEM_SEG_HEAD.MASK_DIM, dn_mode=mf.DN_MODE, head_dn=mf.HEAD_DN,
                    all_lys=mf.ALL_LY_DN, dn_ratio=mf.DN_RATIO, dn_label_noise_ratio=mf.LB_NOISE_RATIO)

    # ---------------------------------------------------------------------------------------------
    def _mp_setup(self, dn_args, bs, size_list, device):
        """prepare_for_dn_v5 (:968-1060) minus the prediction-head call.  Returns None when there is
        no ground truth in the batch (-> prepare_for_normal)."""
        targets, scalar, noise_scale = dn_args["tgt"], dn_args["scalar"], dn_args["noise_scale"]
        num = [len(t["boxes"]) for t in targets]
        max_num = max(num)
        if scalar >= 100:
            scalar = scalar // max_num if max_num else 0
        if max_num == 0 or scalar == 0:
            return None
        pad = scalar * max_num
        labels = torch.cat([t["labels"] for t in targets]).repeat(scalar, 1).view(-1)
        if self.dn_label_noise_ratio > 0:
            prob = _rng.rand("label_prob", tuple(labels.shape), device)
            chosen = prob < self.dn_label_noise_ratio
            if _rng.replaying():
                # tests replay the reference's draws, which has one new label per CHOSEN position
                # (:1003-1007: nonzero -> randint_like -> scatter_, a device->host sync)
                new_label = _rng.randint("label_new", (int(chosen.sum()),), self.num_classes, device)
                labels = labels.clone()
                labels[chosen] = new_label.to(labels.dtype)
            else:
                # same distribution without the sync: draw a candidate for every position, keep the chosen
                cand = torch.randint(0, self.num_classes, tuple(labels.shape), device=device, dtype=labels.dtype)
                labels = torch.where(chosen, cand, labels)
        feats = self.label_enc(labels)
        bid = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(num)]).repeat(scalar, 1).view(-1)
        slot = torch.cat([torch.arange(n) for n in num])
        slot = torch.cat([slot + max_num * i for i in range(scalar)]).long()
        bid, slot = upload(bid, device), upload(slot, device)
        padding = torch.zeros(bs, pad, feats.shape[-1], device=device, dtype=feats.dtype)
        padding[(bid, slot)] = feats
        # GT rows per level, computed once per forward (the reference re-derives them every layer)
        rows, base = [], []
        gts = [t["masks"] for t in targets if len(t["masks"]) > 0]
        same = all(g.shape[1:] == gts[0].shape[1:] and g.dtype == gts[0].dtype for g in gts)
        all_masks = stacked_masks(gts) if same else None      # (shared with the matcher's copy: _targets.py)
        for size in size_list:
            gt = gt_block_or(all_masks, size) if same else torch.cat([gt_block_or(g, size) for g in gts])
            base.append(gt.repeat(scalar, 1))
            if noise_scale == 0:
                pm = torch.ones(bs, pad, size[0] * size[1], dtype=torch.bool, device=device)
                pm[(bid, slot)] = base[-1]
                rows.append(pm)

        def noisy_rows(level):
            """point noise (:991-998, :1606-1613): a fresh draw per call flips every position of a row with probability
            (open area of the row) * noise_scale / (h w)"""
            b = base[level]
            ratio = (~b).sum(1) * (noise_scale / b.shape[1])
            pm = torch.ones(bs, pad, b.shape[1], dtype=torch.bool, device=device)
            pm[(bid, slot)] = torch.logical_xor(b, _rng.rand("mp_noise", tuple(b.shape), device) < ratio[:, None])
            return pm

        if noise_scale != 0 and _rng.replaying():
            rows = noisy_rows          # the tests' reference: the reference's ops, fed with the reference's recorded draws
        elif noise_scale != 0:
            # production: one native launch per mask (mp_noise.hip).  What does not change within the forward is made once:
            # the open counts of every level, and the inverse of (bid, slot) — for each output row the base row it shows
            counts = [mp_open_counts(b) for b in base]
            total = sum(num)
            src_of = np.full((bs, pad), -1, dtype=np.int32)
            first = 0
            for b, n in enumerate(num):
                for s in range(scalar):
                    src_of[b, s * max_num:s * max_num + n] = np.arange(s * total + first, s * total + first + n, dtype=np.int32)
                first += n
            src_of = upload(src_of.reshape(-1), device)

            def rows(level):
                seed, draw = _next_noise_draw(device)
                return mp_noise_rows(base[level], src_of, bs, pad, noise_scale, seed, draw, counts[level])
        tgt_size = pad + self.num_queries
        tgt_mask = torch.zeros(tgt_size, tgt_size, dtype=torch.bool, device=device)
        tgt_mask[pad:, :pad] = True
        for i in range(scalar):
            tgt_mask[max_num * i:max_num * (i + 1), max_num * (i + 1):pad] = True
            tgt_mask[max_num * i:max_num * (i + 1), :max_num * i] = True
        return dict(padding=padding, rows=rows, tgt_mask=tgt_mask, dn_args={"max_num": max_num, "pad_size": pad})

    # ---------------------------------------------------------------------------------------------
    def _weights(self):
        """name -> tensor for every GEMM weight / bias of the decoder.  Under autocast these are bf16
        working copies made by ONE grouped cast (_CastParams); the packed in-projections come back as
        (q, k, v) row-block tuples.  LayerNorm / embedding
        parameters stay fp32 modules (autocast runs them in fp32 anyway)."""
        # (walking the module tree costs ~1 ms of launch-thread time per call: the (name, owner module, key) triples are kept and
        # the parameters read from their owners each time, so a replaced parameter is still picked up)
        cache = self.__dict__.get("_gemm_param_slots")
        if cache is not None:
            # the cache is valid only while the module tree is the one it was built from: every owner is still the child its
            # parent holds under the same name (a swapped / wrapped submodule fails this), with the same number of parameters,
            # none of them removed (~0.2 k dict lookups, tens of microseconds)
            where, links, counts = cache
            if not (all(p._modules.get(k) is c for p, k, c in links) and all(len(m._parameters) == n for m, n in counts)
                    and all(m._parameters.get(k) is not None for _, m, k in where)):
                cache = None
        if cache is None:
            where, links, counts = [], [], []
            for mname, m in self.named_modules():
                counts.append((m, len(m._parameters)))
                for cname, child in m._modules.items():
                    if child is not None:
                        links.append((m, cname, child))
                for k in m._parameters:
                    n = (mname + "." if mname else "") + k
                    if m._parameters[k] is not None and not (".norm." in n or n.startswith("decoder_norm")
                                                             or n.startswith(("query_feat", "query_embed", "level_embed", "label_enc"))):
                        where.append((n, m, k))
            self.__dict__["_gemm_param_slots"] = (where, links, counts)
        named = [(n, m._parameters[k]) for n, m, k in where]
        if torch.is_autocast_enabled() and named and named[0][1].is_cuda:
            chunks = [3 if "in_proj" in n else 1 for n, _ in named]
            cast = _CastParams.apply(torch.get_autocast_dtype("cuda"), chunks, *[p for _, p in named])
            out, k = {}, 0
            for (n, _), c in zip(named, chunks):
                out[n] = cast[k] if c == 1 else tuple(cast[k:k + c])
                k += c
            return out
        return dict(named)

    def _kv_batched(self, W, kin, src):
        """Key / value projections of ALL decoder layers before the layer loop (they depend on the encoder memory only,
        :1784-1789 with level = i % num_feature_levels): the layers that attend to one level share their input, so their
        projections are ONE GEMM with the weights side by side ([S, N, 3 * 256] for 9 layers / 3 levels) instead of one
        per layer — 6 GEMMs instead of 18 forward, and likewise for the input and weight gradients.  Layer i reads its 256
        columns in place (strided K / V in the attention kernels) and its backward writes its columns of the packed
        gradient.  -> {layer: ((k_c, handle), (v_c, handle))}"""
        nl, nlev = self.num_layers, self.num_feature_levels
        groups = [(l, [i for i in range(nl) if i % nlev == l]) for l in range(nlev)]
        groups = [(l, g) for l, g in groups if g]              # (fewer layers than levels: some levels are never attended to)
        ng = len(groups)
        ws, sizes = [], []
        for which in (1, 2):                                   # k rows, then v rows of the packed in-projections
            for key in ("in_proj_weight", "in_proj_bias"):
                for _, g in groups:
                    ws += [W[f"transformer_cross_attention_layers.{i}.multihead_attn.{key}"][which] for i in g]
                    sizes.append(len(g))
        cat = _GatherRows.apply(sizes, *ws)                    # [wk_g..., bk_g..., wv_g..., bv_g...]
        out = {}
        for gi, (l, g) in enumerate(groups):
            wk, bk, wv, bv = cat[gi], cat[ng + gi], cat[2 * ng + gi], cat[3 * ng + gi]
            ks = split_cols(linear(kin[l], wk, bk), len(g))
            vs = split_cols(linear(src[l], wv, bv), len(g))
            for j, i in enumerate(g):
                out[i] = (ks[j], vs[j])
        return out

    def _heads(self, W, output, mask_features, attn_mask_target_size, mp_rows=None):
        """forward_prediction_heads (:1859-1877).  Returns (outputs_class, outputs_mask,
        attn_mask[N,Qtot,HW] bool) where the attention mask already has the MP rows written (:1814-1816)
        and all-masked rows cleared (:1780).  ``output`` is the fp32 residual stream [Qtot, N, C]; the
        heads run sequence-first and only the (small) results are viewed batch-first."""
        amp = W["class_embed.weight"].dtype == torch.bfloat16
        d32, d16 = res_ln(self.decoder_norm, output, None, want32=not amp, want16=amp)
        x = d16 if amp else d32
        outputs_class = F.linear(x, W["class_embed.weight"], W["class_embed.bias"]).transpose(0, 1)
        e = F.relu(F.linear(x, W["mask_embed.layers.0.weight"], W["mask_embed.layers.0.bias"]))
        e = F.relu(F.linear(e, W["mask_embed.layers.1.weight"], W["mask_embed.layers.1.bias"]))
        mask_embed = F.linear(e, W["mask_embed.layers.2.weight"], W["mask_embed.layers.2.bias"]).transpose(0, 1)
        outputs_mask = mask_product(mask_embed, mask_features)
        am = native_attn_mask(outputs_mask.detach(), attn_mask_target_size, mp_rows)
        return outputs_class, outputs_mask, am

    def forward_prediction_heads(self, output, mask_features, attn_mask_target_size, mp_rows=None):
        W = self._weights()
        return self._heads(W, output, mask_features.to(W["class_embed.weight"].dtype), attn_mask_target_size, mp_rows)

    def _next_attn_mask(self, W, output, mask_features, attn_mask_target_size, mp_rows=None, pooled=None):
        """The attention mask the NEXT layer needs (:1869-1875), from this layer's mask prediction,
        outside autograd (the reference detaches it, :1875).  The differentiable predictions of all
        layers are produced together by ``_heads_batched`` after the last layer."""
        with torch.no_grad():
            amp = W["class_embed.weight"].dtype == torch.bfloat16
            if (pooled is not None and amp and output.dtype == torch.float32 and output.is_contiguous() and output.shape[-1] == 256
                    and output.shape[0] * output.shape[1] <= 1024):
                n_ = self.decoder_norm
                mlp = [(W[f"mask_embed.layers.{k}.weight"], W[f"mask_embed.layers.{k}.bias"]) for k in range(3)]
                if (n_.elementwise_affine and n_.bias is not None
                        # (raw pointers below: everything the native call reads is checked here — ADVICE r4)
                        and n_.weight.dtype == n_.bias.dtype == torch.float32 and n_.weight.is_contiguous() and n_.bias.is_contiguous()
                        and n_.weight.device == n_.bias.device == output.device and n_.weight.numel() == 256
                        and pooled.dtype == torch.bfloat16 and pooled.is_contiguous() and pooled.shape[-1] == 256
                        and pooled.device == output.device
                        and all(w_.dtype == torch.bfloat16 and w_.shape == (256, 256) and w_.is_contiguous() and b_.is_contiguous()
                                for w_, b_ in mlp)):
                    return next_attn_mask_native(output, n_, mlp, pooled, mp_rows)
            d32, d16 = res_ln(self.decoder_norm, output.detach(), None, want32=not amp, want16=amp)
            x = d16 if amp else d32
            e = linear(x, W["mask_embed.layers.0.weight"].detach(), W["mask_embed.layers.0.bias"].detach(), relu=True)
            e = linear(e, W["mask_embed.layers.1.weight"].detach(), W["mask_embed.layers.1.bias"].detach(), relu=True)
            me = linear(e, W["mask_embed.layers.2.weight"].detach(), W["mask_embed.layers.2.bias"].detach())     # [Qtot, N, C]
            if pooled is not None:
                # fused mask head (csrc/mask_head.hip): product with the features already resized to this level
                return mask_head_bits(me, pooled, mp_rows)
            m = mask_product(me.transpose(0, 1), mask_features.detach())
            return native_attn_mask(m, attn_mask_target_size, mp_rows)

    def _heads_batched(self, W, outputs, mask_features):
        """forward_prediction_heads (:1859-1870) for the residual streams of ALL layers in one go: the
        heads share their weights, so one LayerNorm / four GEMMs / one batched mask product over the
        concatenated queries replace ten of each — and in the backward ten weight-gradient
        accumulations per parameter and nine adds of a mask_features-sized gradient.  The mask
        predictions of layer l are rows [l*Qtot, (l+1)*Qtot) of one [N, L*Qtot, H, W] tensor (the
        criterion addresses them through that parent, point_sample.MapSet).
        Returns (list of outputs_class [N,Qtot,K+1], list of outputs_mask [N,Qtot,H,W])."""
        L = len(outputs)
        Qt, N, C = outputs[0].shape
        amp = W["class_embed.weight"].dtype == torch.bfloat16
        X = torch.stack(outputs, 0).view(L * Qt, N, C)
        d32, d16 = res_ln(self.decoder_norm, X, None, want32=not amp, want16=amp)
        x = d16 if amp else d32
        cls = _class_linear(x, W["class_embed.weight"], W["class_embed.bias"])              # [L*Qt, N, K+1]
        # (2 000+ rows: `linear` takes the library forward / dX and the native split-over-rows weight + bias gradient — the
        # library's dW for a [256, 2 280] x [2 280, 256] product is 4 workgroups walking the whole contraction)
        lin = linear if os.environ.get("MPF_HEADS_TALL", "1") == "1" else F.linear
        e = F.relu(lin(x, W["mask_embed.layers.0.weight"], W["mask_embed.layers.0.bias"]))
        e = F.relu(lin(e, W["mask_embed.layers.1.weight"], W["mask_embed.layers.1.bias"]))
        me = lin(e, W["mask_embed.layers.2.weight"], W["mask_embed.layers.2.bias"]).transpose(0, 1)   # [N, L*Qt, C]
        cls = cls.view(L, Qt, N, -1)
        if self.factored_masks and self.training and mask_fused.supported(me, mask_features):
            # training: the criterion samples the predictions from their factors (matching cost, loss planes of the pairs);
            # the [N, L*Qt, H, W] maps are never formed (mask_fused.FactoredMasks)
            pm = mask_fused.FactoredMasks(me, mask_features)
        else:
            pm = mask_product(me, mask_features)                                             # [N, L*Qt, H, W]
        return [cls[l].transpose(0, 1) for l in range(L)], [pm[:, l * Qt:(l + 1) * Qt] for l in range(L)]

    def _layer_by_ops(self, W, i, level, output, xb, kin, src, attn_mask, tgt_mask, post_norm):
        """One decoder layer, one autograd node per op (fp32 / non-AMP runs, and the reference the fused
        layer is tested against)."""
        H = self.num_heads
        # cross-attention first (:1784-1789), post-norm
        pre = f"transformer_cross_attention_layers.{i}.multihead_attn."
        t2 = masked_mha_w(xb, kin[level], src[level], W[pre + "in_proj_weight"], W[pre + "in_proj_bias"],
                          W[pre + "out_proj.weight"], W[pre + "out_proj.bias"], H, attn_mask)
        output, xb = post_norm(self.transformer_cross_attention_layers[i].norm, output, t2)
        # self-attention (:1791-1795)
        pre = f"transformer_self_attention_layers.{i}.self_attn."
        t2 = masked_mha_w(xb, xb, xb, W[pre + "in_proj_weight"], W[pre + "in_proj_bias"],
                          W[pre + "out_proj.weight"], W[pre + "out_proj.bias"], H, tgt_mask)
        output, xb = post_norm(self.transformer_self_attention_layers[i].norm, output, t2)
        # FFN (:1798-1800)
        pre = f"transformer_ffn_layers.{i}."
        t2 = linear(linear(xb, W[pre + "linear1.weight"], W[pre + "linear1.bias"], relu=True),
                    W[pre + "linear2.weight"], W[pre + "linear2.bias"])
        return post_norm(self.transformer_ffn_layers[i].norm, output, t2)

    def forward(self, x, mask_features, mask=None, dn_args=None):
        assert len(x) == self.num_feature_levels
        del mask
        W = self._weights()
        amp = torch.is_autocast_enabled() and x[0].is_cuda
        adt = torch.get_autocast_dtype("cuda") if amp else None
        src, kin, size_list = [], [], []
        for i in range(self.num_feature_levels):
            size_list.append(tuple(x[i].shape[-2:]))
            xi = x[i]
            if len(self.input_proj[i]._modules) or isinstance(self.input_proj[i], nn.Conv2d):   # 1x1 conv when channels differ
                xi = F.conv2d(xi, W[f"input_proj.{i}.weight"], W[f"input_proj.{i}.bias"])
            Hi, Wi = size_list[-1]
            if (xi.is_cuda and xi.dtype == torch.float32 and xi.shape[1] % 8 == 0 and xi.stride(1) == 1 and xi.stride(2) == Wi * xi.stride(3)
                    and xi.stride(3) % 4 == 0 and xi.stride(0) % 4 == 0 and xi.data_ptr() % 16 == 0
                    and (not amp or adt == torch.bfloat16)):
                # the pixel decoder hands over channel-last views of the encoder memory: one native pass
                key = (Hi, Wi, xi.device)
                pos_t = self._pos_t.get(key)
                if pos_t is None:
                    pos_t = self.pe_layer(xi)[0].flatten(1).t().contiguous()          # [S, C]
                    self._pos_t[key] = pos_t
                s, k_in = _DecoderInputs.apply(xi, self.level_embed.weight[i], pos_t, adt if amp else torch.float32)
            else:
                p = self.pe_layer(xi).flatten(2).permute(2, 0, 1)
                s = (xi.flatten(2) + self.level_embed.weight[i][None, :, None]).permute(2, 0, 1)
                k_in = s + p                 # key input, shared by the 3 layers that use this level
                if amp:                      # one cast per level instead of one per use (9 uses each); the cast also
                    # makes the [S, N, C] operands of the key / value projections row-contiguous
                    s = s.to(adt, memory_format=torch.contiguous_format)
                    k_in = k_in.to(adt, memory_format=torch.contiguous_format)
            src.append(s)
            kin.append(k_in)
        if amp:                          # one cast for the 10 prediction heads
            mask_features = mask_features.to(adt)
        bs = src[0].shape[1]
        device = src[0].device
        mp = self._mp_setup(dn_args, bs, size_list, device) if dn_args is not None else None
        query = self.query_feat.weight.unsqueeze(1).repeat(1, bs, 1)
        if mp is not None:
            output = torch.cat([mp["padding"].transpose(0, 1).to(query.dtype), query], dim=0)
            tgt_mask = mp["tgt_mask"]
        else:
            output, tgt_mask = query, None

        def rows(level, i=None):
            if mp is None:
                return None
            if i is not None and not (self.all_lys or i < 3):
                return None
            r = mp["rows"]
            return r(level) if callable(r) else r[level]           # (callable: point noise, a fresh draw per layer)

        H = self.num_heads
        output = output.float().contiguous()            # fp32 residual stream [Qtot, N, C]
        xb = output.to(adt) if amp else output           # operand copy for the GEMMs (bf16 under AMP)
        # fused mask head (AMP, 256 channels): the features resized ONCE per step to each level grid; the per-layer mask
        # is then a [Qtot x 256] x [256 x HW_l] MFMA product whose sign goes straight to the byte mask
        pooled = [None] * self.num_feature_levels
        if (amp and adt == torch.bfloat16 and mask_features.shape[1] == 256
                and all((hh * ww) % 16 == 0 for hh, ww in size_list)):
            with torch.no_grad():
                done = {}
                for lv, sz in enumerate(size_list):
                    if sz not in done:
                        done[sz] = pool_features(mask_features.detach(), sz)
                    pooled[lv] = done[sz]
        attn_mask = self._next_attn_mask(W, output, mask_features, size_list[0], rows(0), pooled[0])
        streams = [output]

        def post_norm(norm, x32, t2):
            y32, y16 = res_ln(norm, x32, t2, want32=True, want16=amp)
            return y32, (y16 if amp else y32)

        # bf16 autocast, 256 channels x 8 heads: the whole layer is one native call (decoder_layer.py)
        fused = (amp and adt == torch.bfloat16 and output.shape[-1] == 256 and H == 8
                 and isinstance(W["transformer_cross_attention_layers.0.multihead_attn.in_proj_weight"], tuple)
                 and os.environ.get("MPF_FUSED_DECODER", "1") == "1")
        kv = self._kv_batched(W, kin, src) if fused and os.environ.get("MPF_KV_BATCH", "1") == "1" else None
        for i in range(self.num_layers):
            level = i % self.num_feature_levels
            if fused:
                ca = f"transformer_cross_attention_layers.{i}.multihead_attn."
                sa = f"transformer_self_attention_layers.{i}.self_attn."
                ff = f"transformer_ffn_layers.{i}."
                cw, cb = W[ca + "in_proj_weight"], W[ca + "in_proj_bias"]
                sw, sb = W[sa + "in_proj_weight"], W[sa + "in_proj_bias"]
                if kv is not None:
                    (k_c, pk), (v_c, pv) = kv[i]
                    kv_pack = (pk, pv) if pk is not None and pv is not None else None
                else:
                    k_c, v_c, kv_pack = linear(kin[level], cw[1], cb[1]), linear(src[level], cw[2], cb[2]), None
                n1, n2, n3 = (self.transformer_cross_attention_layers[i].norm, self.transformer_self_attention_layers[i].norm,
                              self.transformer_ffn_layers[i].norm)
                output, xb, out_heads = decoder_layer(
                    output, xb, k_c, v_c, attn_mask, tgt_mask, H, n1.eps,
                    (cw[0], cb[0], W[ca + "out_proj.weight"], W[ca + "out_proj.bias"], n1.weight, n1.bias,
                     sw[0], sb[0], sw[1], sb[1], sw[2], sb[2], W[sa + "out_proj.weight"], W[sa + "out_proj.bias"], n2.weight, n2.bias,
                     W[ff + "linear1.weight"], W[ff + "linear1.bias"], W[ff + "linear2.weight"], W[ff + "linear2.bias"],
                     n3.weight, n3.bias), kv_pack)
            else:
                output, xb = self._layer_by_ops(W, i, level, output, xb, kin, src, attn_mask, tgt_mask, post_norm)
                out_heads = output
            nxt = (i + 1) % self.num_feature_levels
            # (the fused layer's second alias of its output, decoder_layer.DecoderLayerFn)
            streams.append(out_heads)
            if i + 1 < self.num_layers:
                attn_mask = self._next_attn_mask(W, output, mask_features, size_list[nxt], rows(nxt, i), pooled[nxt])
            elif mp is not None and callable(mp["rows"]) and (self.all_lys or i < 3):
                # the reference makes the mask after the last layer too (unused): dec_layers + 1 noised masks per forward.  Under
                # replay this keeps the FIFO aligned; the native route follows the same schedule, so the generator offset a
                # forward consumes is the reference's count of draws (one launch at this level's size)
                rows(nxt, i)
        predictions_class, predictions_mask = self._heads_batched(W, streams, mask_features)

        nq = self.num_queries
        if tgt_mask is not None:
            dn_c = [c[:, :-nq] for c in predictions_class]
            dn_m = [m[:, :-nq] for m in predictions_mask]
            predictions_class = [c[:, -nq:] for c in predictions_class]
            predictions_mask = [m[:, -nq:] for m in predictions_mask]
            dn_out = {"pred_logits": dn_c[-1], "pred_masks": dn_m[-1], "aux_outputs": self._set_aux_loss(dn_c, dn_m),
                      "dn_args": mp["dn_args"]}
        else:
            dn_out = None
            # keeps label_enc in the autograd graph so DDP sees every parameter used (:1846)
            predictions_class[-1] = predictions_class[-1] + self.label_enc.weight[0, 0] * 0.0
        return {"pred_logits": predictions_class[-1], "pred_masks": predictions_mask[-1],
                "aux_outputs": self._set_aux_loss(predictions_class, predictions_mask), "dn_out": dn_out}

    @staticmethod
    def _set_aux_loss(outputs_class, outputs_seg_masks):
        return [{"pred_logits": a, "pred_masks": b} for a, b in zip(outputs_class[:-1], outputs_seg_masks[:-1])]
