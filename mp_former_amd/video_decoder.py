"""Masked-attention transformer decoder of a clip — host-side mirror of ``VideoMultiScaleMaskedTransformerDecoder``, reference:
mask2former_video/modeling/transformer_decoder/video_mask2former_transformer_decoder.py
  :18-179   SelfAttentionLayer / CrossAttentionLayer / FFNLayer (with query positions, :45-47, :104-106)
  :213-339  state-dict upgrade, constructor     :341-368  from_config
  :370-442  forward                             :444-461  forward_prediction_heads
and position_encoding.py:29-57 (``PositionEmbeddingSine3D``).

Same parameter names (checkpoints load unchanged), same forward signature and output dict (``pred_masks`` [B, Q, T, h, w]).  The
module is built from the image decoder's parts (transformer_decoder.py), which it imports and shares.  What a clip changes:

  * the memory of a level is [(T * HW), B, C], frame-major (:390-393), and its key input adds the 3D sine embedding, which is the
    sum of a per-pixel table ``pos_yx`` [HW, C] and a per-frame table ``pos_z`` [T, C] (position_encoding.py:56): one native pass
    per level makes both operands from the channel-last feature maps and the two tables (csrc/video_decoder.hip); the
    [T * HW, C] table of a whole video is never formed;
  * the learned query positions ``query_embed`` are added to the query of the cross-attention and to the query and key of the
    self-attention (:415, :421), in fp32 before the operand is rounded — the reference's rounding point under autocast;
  * the "all-masked row -> unmask" rule spans the clip (:409 on [B * h, Q, T * HW]): the fused mask head gives exactly that when
    the features resized per frame are handed to it as [B, T * HW, 256]; where it cannot run (fp32 operands, T * HW not a
    multiple of 16, other widths) the mask is made by torch ops with the rule over the whole clip.  ``mpf_attn_mask`` applies
    the rule per [h, w] plane and is not used here;
  * the mask predictions of all layers are ONE parent [B, L * Q, T, h, w]; layer l is the slice [:, l * Q:(l + 1) * Q], which
    ``video_losses.clip_planes`` / ``MapSet`` address in place.

A layer takes one of two routes (``last_layer_route()`` names the one taken): 'native' — the whole layer is ONE autograd node
whose forward / backward are single native calls (decoder_layer.decoder_layer_pos: the image decoder's one-call layer with a
query-position operand) — under bf16 autocast with 256 channels and 8 heads unless MPF_FUSED_DECODER=0; 'ops' — ``_layer_by_ops``,
one autograd node per op on the same attention / small-GEMM / residual-LayerNorm kernels — everywhere else (fp32, other widths).
The module attribute ``fused_layers`` (None = that rule, True / False = forced) switches routes in one process.  GPU only.
"""
import math
import os

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, mask_fused
from .attention import attention_core
from .decoder_layer import decoder_layer_pos
from .pixel_decoder import _ConvNorm, _c2_xavier_fill
from .resln import res_ln
from .transformer_decoder import (MLP, CrossAttentionLayer, FFNLayer, MultiScaleMaskedTransformerDecoderMaskDN as _ImageDecoder,
                                  SelfAttentionLayer, linear, pool_features)


_last_layer_route = None


def last_layer_route():
    """'native' (one call per layer, decoder_layer_pos) | 'ops' (_layer_by_ops): the route of the most recent decoder layer
    (None before the first)"""
    return _last_layer_route


class PositionEmbeddingSine3D(nn.Module):
    """position_encoding.py:12-57 with mask=None.  ``tables(T, H, W, device)`` -> (pos_yx [H * W, C], pos_z [T, C]), the two
    summands of :56 (C = 2 * num_pos_feats), cached; ``forward(x [B, T, C, H, W])`` -> the reference's [B, T, C, H, W] value."""

    def __init__(self, num_pos_feats=64, temperature=10000, normalize=False, scale=None):
        super().__init__()
        if scale is not None and normalize is False:
            raise ValueError("normalize should be True if scale is passed")
        self.num_pos_feats, self.temperature, self.normalize = num_pos_feats, temperature, normalize
        self.scale = 2 * math.pi if scale is None else scale
        self._tables = {}

    def _embed(self, n, device):
        """:35-42: positions 1 .. n (the cumulative sum of an all-ones mask), normalised to (0, scale]"""
        e = torch.arange(1, n + 1, dtype=torch.float32, device=device)
        if self.normalize:
            e = e / (e[-1:] + 1e-6) * self.scale
        return e

    def _sincos(self, embed, feats):
        dim_t = torch.arange(feats, dtype=torch.float32, device=embed.device)
        dim_t = self.temperature ** (2 * torch.div(dim_t, 2, rounding_mode="floor") / feats)
        p = embed[:, None] / dim_t
        return torch.stack((p[:, 0::2].sin(), p[:, 1::2].cos()), dim=2).flatten(1)

    def tables(self, T, H, W, device):
        key = (T, H, W, device)
        hit = self._tables.get(key)
        if hit is None:
            npf = self.num_pos_feats
            pos_y = self._sincos(self._embed(H, device), npf)[:, None, :].expand(H, W, npf)
            pos_x = self._sincos(self._embed(W, device), npf)[None, :, :].expand(H, W, npf)
            pos_yx = torch.cat((pos_y, pos_x), dim=2).reshape(H * W, 2 * npf).contiguous()
            pos_z = self._sincos(self._embed(T, device), 2 * npf).contiguous()
            if len(self._tables) > 16:
                self._tables.clear()
            hit = self._tables[key] = (pos_yx, pos_z)
        return hit

    def full(self, T, H, W, device):
        """[T, C, H, W], the sum as :56 forms it"""
        pos_yx, pos_z = self.tables(T, H, W, device)
        return (pos_yx[None] + pos_z[:, None]).view(T, H, W, -1).permute(0, 3, 1, 2)

    def forward(self, x, mask=None):
        assert x.dim() == 5 and mask is None, "b, t, c, h, w without a padding mask"
        B, T, _, H, W = x.shape
        return self.full(T, H, W, x.device)[None].expand(B, -1, -1, -1, -1)


class _ClipInputs(torch.autograd.Function):
    """(src, kin) [(T * S), B, C] of one feature level from its maps x [B * T, C, H, W] (a channel-last view), the level
    embedding row and the two position tables — one native pass each way (csrc/video_decoder.hip; :385-393, :105)."""

    @staticmethod
    def forward(ctx, x, level_row, pos_yx, pos_z, T, out_dtype):
        BT, C, H, W = x.shape
        S, B = H * W, BT // T
        src = torch.empty((T * S, B, C), dtype=out_dtype, device=x.device)
        kin = torch.empty((T * S, B, C), dtype=out_dtype, device=x.device)
        _lib.call("mpf_clip_inputs_forward", x.device, x.data_ptr(), x.stride(0), x.stride(3), level_row.data_ptr(), pos_yx.data_ptr(),
                  pos_z.data_ptr(), src.data_ptr(), kin.data_ptr(), _lib.DTYPE[out_dtype], S, T, B, C, _lib.stream_ptr(x.device))
        ctx.dims = (BT, C, H, W, T)
        ctx.set_materialize_grads(False)          # an unused output arrives as None (a NULL operand of the kernel), not as zeros
        return src, kin

    @staticmethod
    def backward(ctx, g_src, g_kin):
        BT, C, H, W, T = ctx.dims
        S, B = H * W, BT // T
        gs = [g for g in (g_src, g_kin) if g is not None]
        if not gs:
            return None, None, None, None, None, None
        if any(g.dtype != gs[0].dtype for g in gs) or gs[0].dtype not in (torch.float32, torch.bfloat16):
            g_src = g_src.float() if g_src is not None else None
            g_kin = g_kin.float() if g_kin is not None else None
        g_src = g_src.contiguous() if g_src is not None else None
        g_kin = g_kin.contiguous() if g_kin is not None else None
        g = g_src if g_src is not None else g_kin
        mem = torch.empty((BT, S, C), dtype=torch.float32, device=g.device)       # channel-last, like the input view
        _lib.call("mpf_clip_inputs_backward", g.device, _lib.ptr(g_src), _lib.ptr(g_kin), _lib.DTYPE[g.dtype], mem.data_ptr(),
                  S * C, C, S, T, B, C, _lib.stream_ptr(g.device))
        dx = mem.permute(0, 2, 1).view(BT, C, H, W)
        d_level = mem.sum((0, 1)) if ctx.needs_input_grad[1] else None
        return dx, d_level, None, None, None, None


def clip_attn_mask_torch(mask_embed, mask_features, size):
    """The attention mask of :449-458 with the row rule of :409, by torch ops: mask_embed [Q, B, C] x mask_features
    [B, T, C, h, w] -> bool [B, Q, T * hl * wl] (one copy for all heads), True = do not attend; a query masked at every position
    of the CLIP attends everywhere.  The route where the fused mask head cannot run."""
    Q, B, _ = mask_embed.shape
    T = mask_features.shape[1]
    m = torch.einsum("qbc,btchw->bqthw", mask_embed, mask_features)
    r = F.interpolate(m.flatten(0, 1).float(), size=tuple(size), mode="bilinear", align_corners=False)
    am = (r < 0).view(B, Q, T * size[0] * size[1])                              # sigmoid(v) < 0.5  <=>  v < 0
    return am & ~am.all(-1, keepdim=True)


class VideoMultiScaleMaskedTransformerDecoder(nn.Module):
    _version = 2

    # shared with the image decoder: the grouped bf16 working copies of the GEMM weights, the key / value projections of all
    # layers per level, the detached mask of the next layer on the fused mask head, the batched prediction heads
    _weights = _ImageDecoder._weights
    _kv_batched = _ImageDecoder._kv_batched
    _next_attn_mask = _ImageDecoder._next_attn_mask
    _heads_batched = _ImageDecoder._heads_batched
    _set_aux_loss = staticmethod(_ImageDecoder._set_aux_loss)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version < 2:   # :213-234
            for k in list(state_dict.keys()):
                if "static_query" in k:
                    state_dict[k.replace("static_query", "query_feat")] = state_dict.pop(k)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def __init__(self, in_channels, mask_classification=True, *, num_classes: int, hidden_dim: int, num_queries: int, nheads: int,
                 dim_feedforward: int, dec_layers: int, pre_norm: bool, mask_dim: int, enforce_input_project: bool, num_frames):
        super().__init__()
        assert mask_classification, "Only support mask classification model"
        self.mask_classification = mask_classification
        self.num_frames = num_frames
        self.pe_layer = PositionEmbeddingSine3D(hidden_dim // 2, normalize=True)
        self.num_heads, self.num_layers = nheads, dec_layers
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
        self.query_embed = nn.Embedding(num_queries, hidden_dim)
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
        # True: in training mode "pred_masks" are mask_fused.FactoredClipMasks (for mp_former_amd's VideoSetCriterion, which takes
        # the matching cost and the matched tubes' planes from the factors); the [B, L * Q, T, h, w] maps are then never formed
        self.factored_masks = False
        self.mask_log = None             # tests: a list here receives the attention mask made after every layer, the last included
        self.fused_layers = None         # None: the rule of ``_one_call_layers``; True / False: that route (tests, the bench tool)

    @classmethod
    def from_config(cls, cfg, in_channels, mask_classification):
        """:341-368 (detectron2 CfgNode)."""
        mf = cfg.MODEL.MASK_FORMER
        assert mf.DEC_LAYERS >= 1
        return dict(in_channels=in_channels, mask_classification=mask_classification, num_classes=cfg.MODEL.SEM_SEG_HEAD.NUM_CLASSES,
                    hidden_dim=mf.HIDDEN_DIM, num_queries=mf.NUM_OBJECT_QUERIES, nheads=mf.NHEADS, dim_feedforward=mf.DIM_FEEDFORWARD,
                    dec_layers=mf.DEC_LAYERS - 1, pre_norm=mf.PRE_NORM, enforce_input_project=mf.ENFORCE_INPUT_PROJ,
                    mask_dim=cfg.MODEL.SEM_SEG_HEAD.MASK_DIM, num_frames=cfg.INPUT.SAMPLING_FRAME_NUM)

    # ---------------------------------------------------------------------------------------------
    def _level_inputs(self, W, i, xi, bs, t, amp, adt):
        """(src, kin) [(T * HW), B, C] of level i (:385-393; kin = src + pos, the key input of :105)"""
        if len(self.input_proj[i]._modules) or isinstance(self.input_proj[i], nn.Conv2d):   # 1x1 conv when channels differ
            xi = F.conv2d(xi, W[f"input_proj.{i}.weight"], W[f"input_proj.{i}.bias"])
        BT, C, Hi, Wi = xi.shape
        if (xi.dtype == torch.float32 and C % 8 == 0 and xi.stride(1) == 1 and xi.stride(2) == Wi * xi.stride(3)
                and xi.stride(3) % 4 == 0 and xi.stride(0) % 4 == 0 and xi.data_ptr() % 16 == 0 and (not amp or adt == torch.bfloat16)):
            # the pixel decoder hands over channel-last views of the encoder memory: one native pass
            pos_yx, pos_z = self.pe_layer.tables(t, Hi, Wi, xi.device)
            return _ClipInputs.apply(xi, self.level_embed.weight[i], pos_yx, pos_z, t, adt if amp else torch.float32)
        pos = self.pe_layer.full(t, Hi, Wi, xi.device).flatten(2).permute(0, 2, 1).reshape(t * Hi * Wi, 1, C)
        s = xi.flatten(2) + self.level_embed.weight[i][None, :, None]
        s = s.view(bs, t, C, Hi * Wi).permute(1, 3, 0, 2).flatten(0, 1)
        k_in = s + pos
        if amp:      # one cast per level instead of one per use; it also makes the operands row-contiguous
            s, k_in = s.to(adt, memory_format=torch.contiguous_format), k_in.to(adt, memory_format=torch.contiguous_format)
        return s, k_in

    def _clip_attn_mask(self, W, output, mf5, size, pooled):
        """The attention mask the next layer needs (:449-459, detached) with the row rule of :409 over the clip: bool
        [B, Q, T * HW].  ``pooled`` [B, T * HW, 256] bf16: the fused mask head; None: torch ops."""
        if pooled is not None:
            return self._next_attn_mask(W, output, None, size, None, pooled)
        with torch.no_grad():
            amp = W["class_embed.weight"].dtype == torch.bfloat16
            d32, d16 = res_ln(self.decoder_norm, output.detach(), None, want32=not amp, want16=amp)
            e = d16 if amp else d32
            for k in range(3):
                e = linear(e, W[f"mask_embed.layers.{k}.weight"].detach(), W[f"mask_embed.layers.{k}.bias"].detach(), relu=k < 2)
            return clip_attn_mask_torch(e, mf5.detach(), size)

    @staticmethod
    def _in_proj(W, pre):
        """the q / k / v row blocks of a packed in-projection: already split under autocast (_CastParams), sliced otherwise"""
        w, b = W[pre + "in_proj_weight"], W[pre + "in_proj_bias"]
        if isinstance(w, (tuple, list)):
            return w, b
        E = w.shape[1]
        return (w[:E], w[E:2 * E], w[2 * E:]), (b[:E], b[E:2 * E], b[2 * E:])

    def _layer_by_ops(self, W, i, output, xb, qpos, k_c, v_c, attn_mask, post_norm, cast):
        """One decoder layer with query positions, one autograd node per op.  ``output`` is the fp32 residual stream, ``xb`` its
        operand copy, ``cast(fp32 sum)`` the operand of a projection that takes ``x + query_pos`` (:45, :104)."""
        H = self.num_heads
        # cross-attention first (:411-416), post-norm
        pre = f"transformer_cross_attention_layers.{i}.multihead_attn."
        w, b = self._in_proj(W, pre)
        q = linear(cast(output + qpos), w[0], b[0])
        t2 = linear(attention_core(q, k_c, v_c, attn_mask, H), W[pre + "out_proj.weight"], W[pre + "out_proj.bias"])
        output, xb = post_norm(self.transformer_cross_attention_layers[i].norm, output, t2)
        # self-attention (:418-422): queries and keys from x + query_pos, values from x
        pre = f"transformer_self_attention_layers.{i}.self_attn."
        w, b = self._in_proj(W, pre)
        xq = cast(output + qpos)
        o = attention_core(linear(xq, w[0], b[0]), linear(xq, w[1], b[1]), linear(xb, w[2], b[2]), None, H)
        t2 = linear(o, W[pre + "out_proj.weight"], W[pre + "out_proj.bias"])
        output, xb = post_norm(self.transformer_self_attention_layers[i].norm, output, t2)
        # FFN (:425-427)
        pre = f"transformer_ffn_layers.{i}."
        t2 = linear(linear(xb, W[pre + "linear1.weight"], W[pre + "linear1.bias"], relu=True),
                    W[pre + "linear2.weight"], W[pre + "linear2.bias"])
        return post_norm(self.transformer_ffn_layers[i].norm, output, t2)

    def _one_call_layers(self, W, amp, adt, channels):
        """Does a layer run as ONE native call (decoder_layer_pos)?  By default under the image decoder's conditions: bf16
        autocast (the weights then arrive as bf16 row blocks), 256 channels, 8 heads, post-norm, MPF_FUSED_DECODER not 0.
        ``fused_layers`` = True / False forces a route; True where the native layer cannot run is an error, not a fallback."""
        # (post-norm holds by construction: the attention / FFN modules refuse normalize_before)
        can = (amp and adt == torch.bfloat16 and channels == 256 and self.num_heads == 8
               and isinstance(W["transformer_cross_attention_layers.0.multihead_attn.in_proj_weight"], tuple))
        want = getattr(self, "fused_layers", None)
        if want is None:
            return can and os.environ.get("MPF_FUSED_DECODER", "1") != "0"
        if want and not can:
            raise RuntimeError("fused_layers=True: the one-call decoder layer needs bf16 autocast, 256 channels, 8 heads, post-norm")
        return bool(want)

    def _layer_native(self, W, i, output, qpos, k_c, v_c, kv_pack, attn_mask):
        """One decoder layer with query positions as one autograd node whose forward / backward are single native calls
        (decoder_layer.decoder_layer_pos): the kernels and rounding points of ``_layer_by_ops``, issued from C++.
        -> (x3 fp32, xb3 bf16, x3 again for the prediction heads)"""
        ca = f"transformer_cross_attention_layers.{i}.multihead_attn."
        sa = f"transformer_self_attention_layers.{i}.self_attn."
        ff = f"transformer_ffn_layers.{i}."
        cw, cb = W[ca + "in_proj_weight"], W[ca + "in_proj_bias"]
        sw, sb = W[sa + "in_proj_weight"], W[sa + "in_proj_bias"]
        n1, n2, n3 = (self.transformer_cross_attention_layers[i].norm, self.transformer_self_attention_layers[i].norm,
                      self.transformer_ffn_layers[i].norm)
        return decoder_layer_pos(
            output, qpos, k_c, v_c, attn_mask, None, self.num_heads, n1.eps,
            (cw[0], cb[0], W[ca + "out_proj.weight"], W[ca + "out_proj.bias"], n1.weight, n1.bias,
             sw[0], sb[0], sw[1], sb[1], sw[2], sb[2], W[sa + "out_proj.weight"], W[sa + "out_proj.bias"], n2.weight, n2.bias,
             W[ff + "linear1.weight"], W[ff + "linear1.bias"], W[ff + "linear2.weight"], W[ff + "linear2.bias"],
             n3.weight, n3.bias), kv_pack)

    def forward(self, x, mask_features, mask=None):
        global _last_layer_route
        assert len(x) == self.num_feature_levels
        del mask                                           # :382-383
        if not mask_features.is_cuda or not all(xi.is_cuda for xi in x):
            raise RuntimeError("mp_former_amd decoder runs on the GPU only (no CPU fallback)")
        bt, c_m, h_m, w_m = mask_features.shape
        bs = bt // self.num_frames if self.training else 1                         # :371-374
        t = bt // bs
        W = self._weights()
        amp = torch.is_autocast_enabled()
        adt = torch.get_autocast_dtype("cuda") if amp else None
        nlev = self.num_feature_levels
        src, kin, size_list = [], [], []
        for i in range(nlev):
            size_list.append(tuple(x[i].shape[-2:]))
            s, k_in = self._level_inputs(W, i, x[i], bs, t, amp, adt)
            src.append(s)
            kin.append(k_in)
        if amp:                          # one cast for the prediction heads of all layers
            mask_features = mask_features.to(adt)
        mf5 = mask_features.view(bs, t, c_m, h_m, w_m)
        # einsum("bqc,btchw->bqthw") as the image product on [B, C, T * h, w]: a view when the frames of a clip are dense
        # channel-last planes (the native MFMA product then takes it under autocast), one copy otherwise
        mf4 = mf5.permute(0, 2, 1, 3, 4).reshape(bs, c_m, t * h_m, w_m)

        # fused mask head (bf16 autocast, 256 channels): the features resized ONCE per level on the B * T frames and seen as
        # [B, T * HW, 256], so that the all-masked-row rule spans the clip; a level whose T * HW is not a multiple of 16 takes
        # the torch route
        pooled = [None] * nlev
        if amp and adt == torch.bfloat16 and c_m == 256:
            with torch.no_grad():
                done = {}
                for lv, sz in enumerate(size_list):
                    if (t * sz[0] * sz[1]) % 16 == 0:
                        if sz not in done:
                            done[sz] = pool_features(mask_features.detach(), sz).view(bs, t * sz[0] * sz[1], c_m)
                        pooled[lv] = done[sz]

        qpos = self.query_embed.weight.float().unsqueeze(1)                       # [Q, 1, C], the same for every clip (:396)
        output = self.query_feat.weight.unsqueeze(1).repeat(1, bs, 1).float().contiguous()     # fp32 residual stream [Q, B, C]
        xb = output.to(adt) if amp else output
        cast = (lambda v: v.to(adt)) if amp else (lambda v: v)

        bf16 = amp and adt == torch.bfloat16

        def post_norm(norm, x32, t2):
            y32, y16 = res_ln(norm, x32, t2, want32=True, want16=bf16)
            return y32, (y16 if bf16 else cast(y32))

        log = self.mask_log
        attn_mask = self._clip_attn_mask(W, output, mf5, size_list[0], pooled[0])
        if log is not None:
            log.append(attn_mask)
        streams = [output]
        # the key / value projections of the layers that share a level as one GEMM each (autocast: the weights arrive as row blocks)
        batched = amp and isinstance(W["transformer_cross_attention_layers.0.multihead_attn.in_proj_weight"], tuple)
        kv = self._kv_batched(W, kin, src) if batched else None
        fused = self._one_call_layers(W, amp, adt, output.shape[-1])
        qpos2 = self.query_embed.weight.float() if fused else None      # [Q, C], passed to every layer: autograd sums the d_qpos
        _last_layer_route = "native" if fused else "ops"
        for i in range(self.num_layers):
            level = i % nlev
            if kv is not None:
                (k_c, pk), (v_c, pv) = kv[i]
            else:
                w, b = self._in_proj(W, f"transformer_cross_attention_layers.{i}.multihead_attn.")
                k_c, v_c, pk, pv = linear(kin[level], w[1], b[1]), linear(src[level], w[2], b[2]), None, None
            if fused:
                kv_pack = (pk, pv) if pk is not None and pv is not None else None
                # (the third result: a second alias of the stream for the prediction heads, decoder_layer._LayerNode)
                output, xb, out_heads = self._layer_native(W, i, output, qpos2, k_c, v_c, kv_pack, attn_mask)
            else:
                output, xb = self._layer_by_ops(W, i, output, xb, qpos, k_c, v_c, attn_mask, post_norm, cast)
                out_heads = output
            streams.append(out_heads)
            nxt = (i + 1) % nlev
            if i + 1 < self.num_layers or log is not None:       # (the reference makes the mask after the last layer too, unused)
                attn_mask = self._clip_attn_mask(W, output, mf5, size_list[nxt], pooled[nxt])
                if log is not None:
                    log.append(attn_mask)
        predictions_class, planes = self._heads_batched(W, streams, mf4)
        # the batched heads return dim-1 slices of ONE parent [B, L * Q, T * h, w]; seen per frame they are slices of
        # [B, L * Q, T, h, w], which clip_planes / MapSet address through that parent
        if isinstance(planes[0], mask_fused.FactoredMasks):      # factored_masks, training, operands the native product takes
            predictions_mask = [mask_fused.FactoredClipMasks(m.me, m.mf, t, m.q0, m.q1) for m in planes]
        else:
            predictions_mask = [m.view(bs, m.shape[1], t, h_m, w_m) for m in planes]
        return {"pred_logits": predictions_class[-1], "pred_masks": predictions_mask[-1],
                "aux_outputs": self._set_aux_loss(predictions_class, predictions_mask)}
