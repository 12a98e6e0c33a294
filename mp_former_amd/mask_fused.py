"""The mask predictions as their FACTORS (csrc/mask_fused.hip behind the C ABI).

    outputs_mask = einsum("bqc,bchw->bqhw", mask_embed, mask_features)      (mask2former_transformer_decoder.py:1865-1870)

is consumed on the training path only through point samples (matcher.py:120-132, criterion.py:141-191), so the decoder hands
the criterion a ``FactoredMasks`` (mask_embed rows + channel-last mask_features) instead of ten [N, Qtot, H/4, W/4] maps:
  * ``match_cost_fused``: the matcher's mask + dice cost straight from the factors (gather + interpolate the features at the
    points, MFMA product with the embeddings, cost sums in registers);
  * ``pair_planes``: the logits planes of the matched / mask-piloted (prediction, target) pairs only, as one MFMA launch over
    embedding rows gathered by the device assignment's indices, differentiable w.r.t. both factors (native backward);
  * ``full_product``: the same kernel over all rows — what a caller of the reference interface gets as ``pred_masks``.
Clips (``FactoredClipMasks``, ``match_cost_fused_clip``): the mask features of a clip are one tall image [B, 256, T * h, w], so
``pair_planes`` writes a tube's T frame planes back to back; the matching cost has its own entry, which pads every frame with
zeros on its own and sums over the T * P samples of one shared point set.
bf16, 256 channels, GPU only (no CPU or eager fallback: unsupported shapes are rejected by ``supported`` before use).
"""
import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from ._h2d import upload


def _is_planes(x):
    """[N, C, H, W] whose images are dense [H*W, C] planes (channels_last), 16-byte aligned."""
    return (x.dim() == 4 and x.stride(1) == 1 and x.stride(3) == x.shape[1] and x.stride(2) == x.shape[3] * x.shape[1]
            and x.stride(0) % 8 == 0 and x.data_ptr() % 16 == 0)


def supported(me, mf):
    """me [N, R, 256] bf16 with contiguous rows, mf [N, 256, H, W] bf16 channel-last planes, H * W a multiple of 128.
    The forward alone takes any H * W % 4 == 0 (include/mpformer_hip.h); 128 is the backward's tile (d F works on 128-pixel
    column tiles, d E on 64-pixel steps of 16-byte aligned gradient rows), and a product accepted here must be differentiable."""
    return (me.is_cuda and mf.is_cuda and me.dtype == torch.bfloat16 and mf.dtype == torch.bfloat16 and me.dim() == 3
            and mf.dim() == 4 and me.shape[2] == 256 and mf.shape[1] == 256 and me.shape[0] == mf.shape[0] and me.stride(2) == 1
            and me.stride(0) % 8 == 0 and me.stride(1) % 8 == 0 and me.data_ptr() % 16 == 0 and _is_planes(mf)
            and (mf.shape[2] * mf.shape[3]) % 128 == 0)


class PairPlanes(Function):
    """planes[slot] = me_row(slot) . mf[image(slot)]  ->  [total_slots, H*W] bf16.
    ``row_off`` int64 (device): element offset from ``me.data_ptr()`` of the embedding row of every PAIR;
    ``pair_of_slot`` int32 (device, or None for the identity): pair of every slot; the slots of image b are
    ``slot_first[b] .. + slot_count[b]`` (int32, device).  Backward: d me (the paired rows; zero elsewhere) and d mf
    (channel-last planes), both native (mpf_pair_planes_backward)."""

    @staticmethod
    def forward(ctx, me, mf, row_off, pair_of_slot, slot_first, slot_count, total_slots, max_count):
        N, C, H, W = mf.shape
        HW = H * W
        dev = me.device
        out = torch.empty((total_slots, HW), dtype=torch.bfloat16, device=dev)
        if total_slots and max_count:
            _lib.call("mpf_pair_planes_forward", dev, me.data_ptr(), row_off.data_ptr(), _lib.ptr(pair_of_slot),
                      slot_first.data_ptr(), slot_count.data_ptr(), mf.data_ptr(), mf.stride(0),
                      out.data_ptr(), N, HW, C, _lib.stream_ptr(dev))
        ctx.save_for_backward(me, mf, row_off, pair_of_slot if pair_of_slot is not None else row_off, slot_first, slot_count)
        ctx.identity = pair_of_slot is None
        ctx.sizes = (total_slots, max_count)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        me, mf, row_off, pair_of_slot, slot_first, slot_count = ctx.saved_tensors
        if ctx.identity:
            pair_of_slot = None
        total_slots, max_count = ctx.sizes
        N, C, H, W = mf.shape
        HW = H * W
        dev = me.device
        want_me, want_mf = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d_me = torch.empty_strided(me.shape, me.stride(), dtype=me.dtype, device=dev).zero_() if want_me else None
        d_mf = torch.empty((N, HW, C), dtype=mf.dtype, device=dev) if want_mf else None
        if not (total_slots and max_count):
            if d_mf is not None:
                d_mf.zero_()
        else:
            g = g.contiguous()
            lib = _lib.lib()
            ws = torch.empty(lib.mpf_pair_planes_backward_workspace_bytes(N, HW, total_slots, max_count), dtype=torch.uint8, device=dev)
            _lib.call("mpf_pair_planes_backward", dev,
                      g.data_ptr(), me.data_ptr(), row_off.data_ptr(), _lib.ptr(pair_of_slot),
                      slot_first.data_ptr(), slot_count.data_ptr(), mf.data_ptr(), mf.stride(0),
                      _lib.ptr(d_mf), HW * C, _lib.ptr(d_me),
                      _lib.MPF_BF16, N, HW, C, total_slots, max_count, ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
        g_mf = d_mf.view(N, H, W, C).permute(0, 3, 1, 2) if d_mf is not None else None
        return d_me, g_mf, None, None, None, None, None, None


_identity_cache = {}


def _identity_layout(me, dev):
    """row offsets / slot ranges of the full product: slot b * R + r = row r of image b"""
    N, R, _ = me.shape
    key = (N, R, me.stride(0), me.stride(1), dev)
    lay = _identity_cache.get(key)
    if lay is None:
        b, r = np.meshgrid(np.arange(N, dtype=np.int64), np.arange(R, dtype=np.int64), indexing="ij")
        row_off = upload((b * me.stride(0) + r * me.stride(1)).reshape(-1), dev)
        i32 = upload(np.concatenate([np.arange(N) * R, np.full(N, R)]).astype(np.int32), dev)
        lay = (row_off, i32[:N], i32[N:])
        if len(_identity_cache) > 64:
            _identity_cache.clear()
        _identity_cache[key] = lay
    return lay


def full_product(me, mf):
    """einsum("bqc,bchw->bqhw", me, mf) -> [N, R, H, W] bf16 (differentiable), for ``supported`` operands."""
    N, R, _ = me.shape
    H, W = mf.shape[2:]
    row_off, first, count = _identity_layout(me, me.device)
    return PairPlanes.apply(me, mf, row_off, None, first, count, N * R, R).view(N, R, H, W)


class FactoredMasks:
    """Rows [q0, q1) of every image of ``einsum("bqc,bchw->bqhw", me, mf)``, unevaluated.  Behaves like the [N, q1 - q0, H, W]
    tensor where the decoder / criterion touch it (shape, dim-1 slicing, detach); anything else goes through
    ``materialize()`` (also reached by float() / cpu() / __torch_function__-free helpers used in the tests)."""

    def __init__(self, me, mf, q0=0, q1=None):
        self.me, self.mf = me, mf
        self.q0 = int(q0)
        self.q1 = int(me.shape[1] if q1 is None else q1)

    @property
    def shape(self):
        return torch.Size((self.me.shape[0], self.q1 - self.q0, self.mf.shape[2], self.mf.shape[3]))

    dtype = property(lambda self: self.me.dtype)
    device = property(lambda self: self.me.device)
    is_cuda = property(lambda self: self.me.is_cuda)
    requires_grad = property(lambda self: self.me.requires_grad or self.mf.requires_grad)

    def dim(self):
        return 4

    def size(self, d=None):
        return self.shape if d is None else self.shape[d]

    def same_factors(self, other):
        return isinstance(other, FactoredMasks) and other.me is self.me and other.mf is self.mf

    def __getitem__(self, idx):
        if isinstance(idx, tuple) and len(idx) == 2 and idx[0] == slice(None) and isinstance(idx[1], slice):
            a, b, step = idx[1].indices(self.q1 - self.q0)
            if step == 1:
                return FactoredMasks(self.me, self.mf, self.q0 + a, self.q0 + max(a, b))
        return self.materialize()[idx]

    def detach(self):
        return FactoredMasks(self.me.detach(), self.mf.detach(), self.q0, self.q1)

    def materialize(self):
        return full_product(self.me[:, self.q0:self.q1], self.mf)

    def float(self):
        return self.materialize().float()

    def cpu(self):
        return self.materialize().cpu()

    def row_offsets(self, b, q):
        """numpy int64: element offsets (from me.data_ptr()) of the embedding rows of (image b, row q of this view)."""
        return b * self.me.stride(0) + (self.q0 + q) * self.me.stride(1)


class FactoredClipMasks(FactoredMasks):
    """Rows [q0, q1) of every clip of ``einsum("bqc,btchw->bqthw", me, mf5)``, unevaluated: ``mf4`` is the clip's mask features
    as ONE tall image [B, 256, T * h, w] (frame f = rows f * h .. (f + 1) * h), the form the clip decoder's product runs on.
    Behaves like the [B, q1 - q0, T, h, w] tensor where the clip criterion touches it (shape, dim-1 slicing, detach);
    anything else goes through ``materialize()``."""

    def __init__(self, me, mf4, T, q0=0, q1=None):
        super().__init__(me, mf4, q0, q1)
        self.T = int(T)
        if mf4.shape[2] % self.T:
            raise RuntimeError(f"a tall image of {mf4.shape[2]} rows does not hold {self.T} frames")

    @property
    def shape(self):
        return torch.Size((self.me.shape[0], self.q1 - self.q0, self.T, self.mf.shape[2] // self.T, self.mf.shape[3]))

    def dim(self):
        return 5

    def same_factors(self, other):
        return isinstance(other, FactoredClipMasks) and other.me is self.me and other.mf is self.mf and other.T == self.T

    def __getitem__(self, idx):
        if isinstance(idx, tuple) and len(idx) == 2 and idx[0] == slice(None) and isinstance(idx[1], slice):
            a, b, step = idx[1].indices(self.q1 - self.q0)
            if step == 1:
                return FactoredClipMasks(self.me, self.mf, self.T, self.q0 + a, self.q0 + max(a, b))
        return self.materialize()[idx]

    def detach(self):
        return FactoredClipMasks(self.me.detach(), self.mf.detach(), self.T, self.q0, self.q1)

    def materialize(self):
        me = self.me[:, self.q0:self.q1]
        # (operands the native product does not take — a criterion handed factors it cannot use — go through the library)
        prod = full_product(me, self.mf) if supported(me, self.mf) else torch.einsum("bqc,bchw->bqhw", me, self.mf)
        return prod.view(self.shape)


def _match_cost(entry, scratch_owner, ws_bytes, views, coords, tsamp, rows, t_first, t_count, group_view, group_index, Q, Tmax, w_mask, w_dice,
                hw, strides, frames):
    """What the two matching-cost entries share: the groups' row offsets, the packed int32 upload, the cost buffer and the call.
    ``strides``: of the features, as the entry takes them; ``frames``: () or (T,); the workspace of ``ws_bytes`` is the scratch
    buffer of ``scratch_owner``, or a fresh tensor when that is None."""
    me, mf = views[0].me, views[0].mf
    dev = me.device
    G, P = coords.shape[0], coords.shape[1]
    first = np.array([views[v].row_offsets(int(b), 0) for v, b in zip(group_view, group_index)], dtype=np.int64)
    first_d = upload(first, dev)
    i32 = upload(np.concatenate([group_index, t_first, t_count]).astype(np.int32), dev)
    cost = torch.zeros((G, Q, Tmax), dtype=torch.float32, device=dev)
    st = _lib.stream_ptr(dev)
    ws = _lib.scratch(scratch_owner, dev, st, ws_bytes) if scratch_owner else torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.call(entry, dev, me.data_ptr(), first_d.data_ptr(), me.stride(1), mf.data_ptr(), *strides, i32[:G].data_ptr(), *hw, mf.shape[1],
              coords.data_ptr(), tsamp.data_ptr(), rows, i32[G:2 * G].data_ptr(), i32[2 * G:].data_ptr(), cost.data_ptr(), G, Q, Tmax, P, *frames,
              float(w_mask), float(w_dice), ws.data_ptr(), ws.numel(), st)
    return cost


def match_cost_fused_clip(views, coords, tsamp, t_first, t_count, group_view, group_clip, Q, Tmax, w_mask, w_dice):
    """Mask + dice matching cost of tubes (mask2former_video/modeling/matcher.py:113-148) of G groups from the factors -> fp32
    [G, Q, Tmax].  views: FactoredClipMasks of one (me, mf4); group g = rows of views[group_view[g]] in clip group_clip[g];
    coords [G, P, 2]: ONE point set for all frames of the group; tsamp [rows, T * P] frame-major."""
    mf, T = views[0].mf, views[0].T
    G, P = coords.shape[0], coords.shape[1]
    h, W = mf.shape[2] // T, mf.shape[3]
    # rows of T * P floats, however the sampler shaped them ([rows * T, P] per plane is the same memory)
    if not tsamp.is_contiguous() or tsamp.numel() % (T * P):
        raise RuntimeError(f"target samples of {tuple(tsamp.shape)} are not rows of {T} x {P}")
    rows = tsamp.numel() // (T * P)
    if int(np.max(np.asarray(t_first) + np.asarray(t_count))) > rows:
        raise RuntimeError("a group's target rows lie outside the target samples")
    ws_bytes = _lib.lib().mpf_match_cost_fused_clip_workspace_bytes(G, Q, Tmax, P, T, rows)
    return _match_cost("mpf_match_cost_fused_clip", "match_cost_fused_clip", ws_bytes, views, coords, tsamp, rows, t_first, t_count, group_view,
                       group_clip, Q, Tmax, w_mask, w_dice, (h, W), (mf.stride(0), h * W * mf.shape[1]), (T,))


def match_cost_fused(views, coords, tsamp, t_first, t_count, group_view, group_image, Q, Tmax, w_mask, w_dice):
    """Mask + dice matching cost (matcher.py:105-147) of G groups from the factors -> fp32 [G, Q, Tmax].
    views: FactoredMasks of one (me, mf); group g = rows of views[group_view[g]] in image group_image[g] (numpy int arrays);
    coords [G, P, 2]; tsamp [rows, P]; t_first / t_count numpy int [G]."""
    mf, rows = views[0].mf, tsamp.shape[0]
    ws_bytes = _lib.lib().mpf_match_cost_fused_workspace_bytes(coords.shape[0], Q, Tmax, coords.shape[1], rows)
    return _match_cost("mpf_match_cost_fused", None, ws_bytes, views, coords, tsamp, rows, t_first, t_count, group_view, group_image, Q, Tmax,
                       w_mask, w_dice, tuple(mf.shape[2:]), (mf.stride(0),), ())
