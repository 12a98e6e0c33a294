"""Swin Transformer backbone with native shifted-window attention (csrc/win_attn.hip).

Mirrors the submodule, parameter and buffer names of the reference's backbone (mask2former/modeling/backbone/swin.py), so a
converted checkpoint loads with ``strict=True``.  LayerNorm, the Linear layers, GELU, patch embedding and patch merging are
torch ops; the attention core of a block — roll, window partition, scaled product, relative position bias, shift mask, softmax,
product with v, window reverse, roll back — is ONE native call per direction on the qkv Linear's output:

  window_attention(qkv, table, ws, shift, scale)   autograd Function over mpf_win_attn_forward / mpf_win_attn_backward
  window_attention_torch(...)                      the same function as the reference's op sequence: any device, any dtype

A block takes the native route when qkv is bf16 on the GPU (the qkv Linear under bf16 autocast), the head dim is 32, the window
is at most 12 wide and MPF_SWIN_NATIVE is not 0; otherwise the torch-op route.  `last_route()` names the route of the most recent
block; `_lib.last_kernel()` names the kernel.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils import checkpoint

from . import _lib

HEAD_DIM = 32
MAX_WINDOW = 12
_last_route = None


def last_route():
    """'native' | 'torch': the route of the most recent block's attention (None before the first)"""
    return _last_route


def relative_position_index(ws):
    """[ws^2, ws^2] int64, closed form of swin.py:111-120: (ri - rj + ws - 1) (2 ws - 1) + (ci - cj + ws - 1) for query i, key j —
    the index csrc/win_attn.hip computes from the two tokens' in-window coordinates"""
    t = torch.arange(ws * ws)
    r, c = t // ws, t % ws
    return (r[:, None] - r[None, :] + ws - 1) * (2 * ws - 1) + (c[:, None] - c[None, :] + ws - 1)


def shift_regions(Hp, Wp, ws, shift, device=None):
    """[Hp, Wp] region number of every ROLLED position (swin.py:413-431): 3 rh + rc, rh = 0 | 1 | 2 for r < Hp - ws | < Hp - shift | else"""
    r, c = torch.arange(Hp, device=device), torch.arange(Wp, device=device)
    rh = (r >= Hp - ws).long() + (r >= Hp - shift).long()
    rc = (c >= Wp - ws).long() + (c >= Wp - shift).long()
    return 3 * rh[:, None] + rc[None, :]


def _partition(x, ws):
    """[B, Hp, Wp, ...] -> [B, nW, ws^2, ...]"""
    B, Hp, Wp = x.shape[:3]
    rest = x.shape[3:]
    x = x.reshape(B, Hp // ws, ws, Wp // ws, ws, *rest)
    return x.permute(0, 1, 3, 2, 4, *range(5, 5 + len(rest))).reshape(B, (Hp // ws) * (Wp // ws), ws * ws, *rest)


def window_attention_torch(qkv, table, ws, shift, scale, index=None):
    """The reference's op sequence on qkv [B, Hp, Wp, 3 C] of the padded, un-rolled map -> [B, Hp, Wp, C] (un-rolled)."""
    B, Hp, Wp, C3 = qkv.shape
    C = C3 // 3
    heads = table.shape[1]
    N = ws * ws
    x = torch.roll(qkv, shifts=(-shift, -shift), dims=(1, 2)) if shift > 0 else qkv
    x = _partition(x, ws).reshape(B, -1, N, 3, heads, C // heads).permute(3, 0, 1, 4, 2, 5)       # [3, B, nW, heads, N, hd]
    q, k, v = x[0], x[1], x[2]
    attn = (q * scale) @ k.transpose(-2, -1)
    if index is None:
        index = relative_position_index(ws).to(table.device)
    bias = table[index.reshape(-1)].view(N, N, heads).permute(2, 0, 1)
    attn = attn + bias
    if shift > 0:
        reg = _partition(shift_regions(Hp, Wp, ws, shift, qkv.device)[None], ws)[0]                # [nW, N]
        mask = (reg[:, None, :] != reg[:, :, None]).float() * -100.0
        attn = attn + mask[None, :, None]
    attn = torch.softmax(attn, dim=-1)
    out = (attn.to(v.dtype) @ v).transpose(2, 3).reshape(B, Hp // ws, Wp // ws, ws, ws, C)
    out = out.permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    return torch.roll(out, shifts=(shift, shift), dims=(1, 2)) if shift > 0 else out


def _geometry(qkv, table, ws):
    B, Hp, Wp, C3 = qkv.shape
    heads = table.shape[1]
    if C3 != 3 * heads * HEAD_DIM:
        raise ValueError(f"window_attention: qkv has {C3} channels, the table {heads} heads of dim {HEAD_DIM}")
    if table.shape[0] != (2 * ws - 1) ** 2:
        raise ValueError(f"window_attention: the table has {table.shape[0]} rows, window {ws} needs {(2 * ws - 1) ** 2}")
    return B, Hp, Wp, heads


class _WindowAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, table, ws, shift, scale):
        if not (qkv.is_cuda and qkv.dtype == torch.bfloat16):
            raise RuntimeError("window_attention: the native route takes bf16 CUDA tensors (window_attention_torch is the other route)")
        qkv = qkv.contiguous()
        table = table.detach().float().contiguous()
        B, Hp, Wp, heads = _geometry(qkv, table, ws)
        out = torch.empty(B, Hp, Wp, heads * HEAD_DIM, dtype=torch.bfloat16, device=qkv.device)
        _lib.call("mpf_win_attn_forward", qkv.device, qkv.data_ptr(), table.data_ptr(), out.data_ptr(), B, Hp, Wp, heads, HEAD_DIM,
                  ws, shift, scale, _lib.stream_ptr(qkv.device))
        ctx.save_for_backward(qkv, table, out)
        ctx.args = (ws, shift, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, table, out = ctx.saved_tensors
        ws, shift, scale = ctx.args
        B, Hp, Wp, heads = _geometry(qkv, table, ws)
        dout = dout.contiguous()
        dqkv = torch.empty_like(qkv)
        dtable = torch.empty_like(table)
        stream = _lib.stream_ptr(qkv.device)
        nbytes = _lib.lib().mpf_win_attn_workspace_bytes(B, Hp, Wp, heads, ws)
        work = _lib.scratch("win_attn_bwd", qkv.device, stream, nbytes)
        _lib.call("mpf_win_attn_backward", qkv.device, qkv.data_ptr(), table.data_ptr(), out.data_ptr(), dout.data_ptr(), dqkv.data_ptr(),
                  dtable.data_ptr(), B, Hp, Wp, heads, HEAD_DIM, ws, shift, scale, work.data_ptr(), work.numel(), stream)
        return dqkv, dtable, None, None, None


def window_attention(qkv, table, ws, shift, scale):
    """softmax(scale q k^T + bias + shift mask) v per (image, window, head) on qkv [B, Hp, Wp, 3 C] bf16 (padded, un-rolled) ->
    [B, Hp, Wp, C] bf16; table fp32 [(2 ws - 1)^2, heads].  Unsupported sizes raise (the library's argument error)."""
    return _WindowAttention.apply(qkv, table, int(ws), int(shift), float(scale))


def native_route(qkv, heads, ws):
    """whether a block's attention on this qkv takes the native kernels"""
    return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.shape[-1] == 3 * heads * HEAD_DIM and 2 <= ws <= MAX_WINDOW
            and os.environ.get("MPF_SWIN_NATIVE", "1") != "0")


class DropPath(nn.Module):
    """Per-sample stochastic depth: a sample is kept with probability 1 - p and scaled by 1 / (1 - p); identity in eval."""

    def __init__(self, p=0.0):
        super().__init__()
        self.p = float(p)

    def forward(self, x):
        if not self.training or self.p == 0.0:
            return x
        keep = 1.0 - self.p
        shape = (x.shape[0],) + (1,) * (x.dim() - 1)
        gate = (torch.rand(shape, device=x.device, dtype=torch.float32) < keep).to(x.dtype)
        return x * (gate / keep)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features, drop=0.0):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden_features, in_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class WindowAttention(nn.Module):
    """qkv Linear -> attention core (either route) -> proj Linear, on the padded un-rolled map [B, Hp, Wp, C] (the reference's
    module takes partitioned windows; the Linear layers are per token, so the parameters mean the same)."""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0.0, proj_drop=0.0):
        super().__init__()
        if attn_drop:
            raise NotImplementedError("attention dropout is not supported (every reference config has ATTN_DROP_RATE 0)")
        self.dim, self.window_size, self.num_heads = dim, window_size, num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size - 1) ** 2, num_heads))
        self.register_buffer("relative_position_index", relative_position_index(window_size))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)

    def forward(self, x, shift):
        global _last_route
        qkv = self.qkv(x)
        if native_route(qkv, self.num_heads, self.window_size):
            _last_route = "native"
            out = window_attention(qkv, self.relative_position_bias_table, self.window_size, shift, self.scale)
        else:
            _last_route = "torch"
            out = window_attention_torch(qkv, self.relative_position_bias_table, self.window_size, shift, self.scale,
                                         self.relative_position_index)
        return self.proj_drop(self.proj(out))


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size=7, shift_size=0, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0,
                 attn_drop=0.0, drop_path=0.0, norm_layer=nn.LayerNorm):
        super().__init__()
        assert 0 <= shift_size < window_size, "shift_size must be in 0 .. window_size - 1"
        self.dim, self.num_heads, self.window_size, self.shift_size = dim, num_heads, window_size, shift_size
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size, num_heads, qkv_bias, qk_scale, attn_drop, drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio), drop)

    def forward(self, x, H, W):
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        ws = self.window_size
        y = self.norm1(x).view(B, H, W, C)
        pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
        if pad_r or pad_b:
            y = F.pad(y, (0, 0, 0, pad_r, 0, pad_b))                # zeros after the norm: a padded token's q, k, v are the bias
        y = self.attn(y, self.shift_size)
        if pad_r or pad_b:
            y = y[:, :H, :W, :]
        x = x + self.drop_path(y.reshape(B, H * W, C))
        return x + self.drop_path(self.mlp(self.norm2(x)))


class PatchMerging(nn.Module):
    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x, H, W):
        B, L, C = x.shape
        assert L == H * W, "input feature has wrong size"
        x = x.view(B, H, W, C)
        if H % 2 or W % 2:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
        return self.reduction(self.norm(x.reshape(B, -1, 4 * C)))


class BasicLayer(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size=7, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop=0.0, attn_drop=0.0,
                 drop_path=0.0, norm_layer=nn.LayerNorm, downsample=None, use_checkpoint=False):
        super().__init__()
        self.window_size, self.depth, self.use_checkpoint = window_size, depth, use_checkpoint
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim, num_heads, window_size, 0 if i % 2 == 0 else window_size // 2, mlp_ratio, qkv_bias, qk_scale,
                                 drop, attn_drop, drop_path[i] if isinstance(drop_path, (list, tuple)) else drop_path, norm_layer)
            for i in range(depth)])
        self.downsample = downsample(dim=dim, norm_layer=norm_layer) if downsample is not None else None

    def forward(self, x, H, W):
        for blk in self.blocks:
            x = checkpoint.checkpoint(blk, x, H, W, use_reentrant=False) if self.use_checkpoint else blk(x, H, W)
        if self.downsample is not None:
            return x, H, W, self.downsample(x, H, W), (H + 1) // 2, (W + 1) // 2
        return x, H, W, x, H, W


class PatchEmbed(nn.Module):
    def __init__(self, patch_size=4, in_chans=3, embed_dim=96, norm_layer=None):
        super().__init__()
        self.patch_size = (patch_size, patch_size) if isinstance(patch_size, int) else tuple(patch_size)
        self.in_chans, self.embed_dim = in_chans, embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = norm_layer(embed_dim) if norm_layer is not None else None

    def forward(self, x):
        H, W = x.shape[-2:]
        ph, pw = self.patch_size
        if H % ph or W % pw:
            x = F.pad(x, (0, (pw - W % pw) % pw, 0, (ph - H % ph) % ph))
        x = self.proj(x)
        if self.norm is not None:
            Wh, Ww = x.shape[-2:]
            x = self.norm(x.flatten(2).transpose(1, 2)).transpose(1, 2).reshape(-1, self.embed_dim, Wh, Ww)
        return x


class SwinTransformer(nn.Module):
    """Constructor arguments as the reference's SwinTransformer (swin.py:526-547); returns {"res2": .., "res5": ..} NCHW."""

    def __init__(self, pretrain_img_size=224, patch_size=4, in_chans=3, embed_dim=96, depths=(2, 2, 6, 2), num_heads=(3, 6, 12, 24),
                 window_size=7, mlp_ratio=4.0, qkv_bias=True, qk_scale=None, drop_rate=0.0, attn_drop_rate=0.0, drop_path_rate=0.2,
                 norm_layer=nn.LayerNorm, ape=False, patch_norm=True, out_indices=(0, 1, 2, 3), frozen_stages=-1, use_checkpoint=False):
        super().__init__()
        depths, num_heads = list(depths), list(num_heads)
        self.pretrain_img_size, self.num_layers, self.embed_dim = pretrain_img_size, len(depths), embed_dim
        self.ape, self.patch_norm, self.out_indices, self.frozen_stages = ape, patch_norm, tuple(out_indices), frozen_stages
        self.patch_embed = PatchEmbed(patch_size, in_chans, embed_dim, norm_layer if patch_norm else None)
        if ape:
            size = (pretrain_img_size,) * 2 if isinstance(pretrain_img_size, int) else tuple(pretrain_img_size)
            ph, pw = self.patch_embed.patch_size
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, embed_dim, size[0] // ph, size[1] // pw))
            nn.init.trunc_normal_(self.absolute_pos_embed, std=0.02)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]
        self.layers = nn.ModuleList()
        for i in range(self.num_layers):
            self.layers.append(BasicLayer(int(embed_dim * 2 ** i), depths[i], num_heads[i], window_size, mlp_ratio, qkv_bias, qk_scale,
                                          drop_rate, attn_drop_rate, dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer,
                                          PatchMerging if i < self.num_layers - 1 else None, use_checkpoint))
        self.num_features = [int(embed_dim * 2 ** i) for i in range(self.num_layers)]
        for i in self.out_indices:
            self.add_module(f"norm{i}", norm_layer(self.num_features[i]))
        self._freeze_stages()

    def _freeze_stages(self):
        """what swin.py:618-633 freezes: patch_embed from 0, the position embedding from 1, pos_drop and layers 0 .. n - 2 from 2"""
        if self.frozen_stages >= 0:
            self.patch_embed.eval()
            for p in self.patch_embed.parameters():
                p.requires_grad = False
        if self.frozen_stages >= 1 and self.ape:
            self.absolute_pos_embed.requires_grad = False
        if self.frozen_stages >= 2:
            self.pos_drop.eval()
            for i in range(self.frozen_stages - 1):
                self.layers[i].eval()
                for p in self.layers[i].parameters():
                    p.requires_grad = False

    def forward(self, x):
        x = self.patch_embed(x)
        Wh, Ww = x.shape[-2:]
        if self.ape:
            x = x + F.interpolate(self.absolute_pos_embed, size=(Wh, Ww), mode="bicubic")
        x = self.pos_drop(x.flatten(2).transpose(1, 2))
        outs = {}
        for i, layer in enumerate(self.layers):
            x_out, H, W, x, Wh, Ww = layer(x, Wh, Ww)
            if i in self.out_indices:
                x_out = getattr(self, f"norm{i}")(x_out)
                outs[f"res{i + 2}"] = x_out.view(-1, H, W, self.num_features[i]).permute(0, 3, 1, 2).contiguous()
        return outs

    def train(self, mode=True):
        """training mode with the frozen stages kept in eval; returns self (the reference's override returns None)"""
        super().train(mode)
        self._freeze_stages()
        return self
