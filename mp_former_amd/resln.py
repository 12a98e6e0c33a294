"""Post-norm residual block ``LayerNorm(x + t)`` of the decoder layers as one native pass
(csrc/elementwise.hip, mpf_res_ln256_*): the fp32 residual stream ``x`` plus the (bf16 under AMP)
branch output ``t``, normalised, written as the next fp32 residual and/or as the bf16 operand of the
next GEMMs — instead of add + LayerNorm + cast kernels forward and five kernels backward.
Reference: mask2former_transformer_decoder.py:42-52, :100-112, :165-169 (forward_post), :1861
(decoder_norm).  256 channels, CUDA; other cases use the torch ops."""
import torch
import torch.nn.functional as F
from torch.autograd import Function

from . import _lib

_BRANCH_DTYPES = (torch.float32, torch.bfloat16)     # what the kernel reads as the branch output t


def _forward_args(x, t, gamma, beta, eps, s_out, y32, y16, padd=None, y_plus=None):
    """-> (mean, rstd, the arguments of mpf_res_ln256_forward / _forward_b up to y_plus)"""
    rows = x.numel() // 256
    mean, rstd = (torch.empty(rows, dtype=torch.float32, device=x.device) for _ in range(2))
    return mean, rstd, (x.data_ptr(), _lib.ptr(t), _lib.DTYPE[t.dtype] if t is not None else 0, gamma.data_ptr(), beta.data_ptr(),
                        _lib.ptr(s_out), _lib.ptr(y32), _lib.ptr(y16), mean.data_ptr(), rstd.data_ptr(), rows, float(eps),
                        _lib.ptr(padd), padd.shape[0] if padd is not None else 0, _lib.ptr(y_plus))


def _backward_ws(s, mean, rstd, gamma, gy32, gy16, gy_plus, ds32, ds16, dgb, ds_amax=None):
    """dgb [2, 256] = (dgamma, dbeta) through per-workgroup partials, fixed order (no atomics, no zero-fill); ds_amax: as ln256_backward"""
    rows = s.numel() // 256
    stream = _lib.stream_ptr(s.device)
    ws = _lib.scratch("ln_bwd", s.device, stream, _lib.lib().mpf_res_ln256_backward_workspace_bytes(rows))
    args = (s.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), _lib.ptr(gy32), _lib.ptr(gy16), _lib.ptr(gy_plus),
            _lib.ptr(ds32), _lib.ptr(ds16), dgb[0].data_ptr(), dgb[1].data_ptr(), rows, ws.data_ptr(), ws.numel())
    if ds_amax is not None:
        _lib.call("mpf_res_ln256_backward_ws_amax", s.device, *args, ds_amax.data_ptr(), stream)
    else:
        _lib.call("mpf_res_ln256_backward_ws", s.device, *args, stream)


def ln_partial_stride(rows):
    """bytes from one LayerNorm's slot of per-workgroup partials to the next (256-aligned) where several share a buffer"""
    return (int(_lib.lib().mpf_res_ln256_backward_workspace_bytes(rows)) + 255) & ~255


class _ResLN(Function):
    @staticmethod
    def forward(ctx, x, t, gamma, beta, eps, want32, want16):
        s = torch.empty_like(x) if t is not None else x
        y32 = torch.empty_like(x) if want32 else None
        y16 = torch.empty_like(x, dtype=torch.bfloat16) if want16 else None
        mean, rstd, args = _forward_args(x, t, gamma, beta, eps, s if t is not None else None, y32, y16)
        _lib.call("mpf_res_ln256_forward", x.device, *args, _lib.stream_ptr(x.device))
        ctx.save_for_backward(s, mean, rstd, gamma)
        ctx.t_dtype = t.dtype if t is not None else None
        ctx.rows = x.numel() // 256
        return y32, y16

    @staticmethod
    def backward(ctx, g32, g16):
        s, mean, rstd, gamma = ctx.saved_tensors
        need_x, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and ctx.t_dtype is not None
        t16 = need_t and ctx.t_dtype == torch.bfloat16
        want32 = need_x or (need_t and not t16) or not t16
        ds32 = torch.empty_like(s) if want32 else None
        ds16 = torch.empty_like(s, dtype=torch.bfloat16) if t16 else None
        dgb = torch.empty((2, 256), dtype=torch.float32, device=s.device)
        g32, g16 = (g.contiguous() if g is not None else None for g in (g32, g16))
        # parameter gradients without float atomics (bit-reproducible): per-workgroup partials summed in a fixed order — by the
        # workgroup that arrives last for a few hundred rows (one launch; "ln_det": a ticket word, zero between calls —
        # zero-initialised, reset by every launch — then the partials), by a parallel second launch beyond
        if ctx.rows <= 1024:
            stream = _lib.stream_ptr(s.device)
            ws = _lib.scratch("ln_det", s.device, stream, _lib.lib().mpf_res_ln256_backward_det_workspace_bytes(ctx.rows), zeroed=True)
            _lib.call("mpf_res_ln256_backward_det", s.device, s.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), _lib.ptr(g32),
                      _lib.ptr(g16), None, _lib.ptr(ds32), _lib.ptr(ds16), dgb.data_ptr(), ctx.rows, ws.data_ptr(), ws.numel(), stream)
        else:
            _backward_ws(s, mean, rstd, gamma, g32, g16, None, ds32, ds16, dgb)
        dt = (ds16 if t16 else ds32) if need_t else None
        return (ds32 if need_x else None), dt, dgb[0], dgb[1], None, None, None


def res_ln(norm, x, t=None, want32=True, want16=False):
    """(y32, y16) = LayerNorm(x + t) with the parameters of ``norm`` (an nn.LayerNorm).  x: fp32
    residual stream; t: branch output (fp32 / bf16) or None.  y32 (fp32) / y16 (bf16) are None unless
    requested."""
    C = x.shape[-1]
    ok = (x.is_cuda and C == 256 and x.dtype == torch.float32 and x.is_contiguous() and norm.elementwise_affine
          and norm.bias is not None and (t is None or (t.shape == x.shape and t.dtype in _BRANCH_DTYPES and t.is_contiguous())))
    if ok:
        return _ResLN.apply(x, t, norm.weight, norm.bias, norm.eps, want32, want16)
    s = x if t is None else x + t
    y = F.layer_norm(s.float(), (C,), norm.weight, norm.bias, norm.eps)
    return (y if want32 else None), (y.to(torch.bfloat16) if want16 else None)


def ln256_forward(x, gamma, beta, eps, padd=None, y_bound=None, padd_amax=None, yplus_bound=None):
    """Raw forward for hand-scheduled callers (encoder_fused): x fp32 [rows, 256] -> (y, mean, rstd[, y + padd[row % len]]).
    y_bound / yplus_bound: zeroed amax slots that receive an upper bound of |y| / |y + padd| (padd_amax: the slot of padd)."""
    y = torch.empty_like(x)
    yp = torch.empty_like(x) if padd is not None else None
    mean, rstd, args = _forward_args(x, None, gamma, beta, eps, None, y, None, padd, yp)
    if y_bound is not None:
        _lib.call("mpf_res_ln256_forward_b", x.device, *args, y_bound.data_ptr(), _lib.ptr(padd_amax),
                  _lib.ptr(yplus_bound) if yp is not None else None, _lib.stream_ptr(x.device))
    else:
        _lib.call("mpf_res_ln256_forward", x.device, *args, _lib.stream_ptr(x.device))
    return y, mean, rstd, yp


def ln256_backward(s, mean, rstd, gamma, gy, gy_plus=None, ds_amax=None):
    """Raw backward: -> (ds fp32, dgamma, dbeta) with g = gy (+ gy_plus); ds_amax: a zeroed amax slot that receives max |ds|."""
    ds = torch.empty_like(s)
    dgb = torch.empty((2, 256), dtype=torch.float32, device=s.device)
    _backward_ws(s, mean, rstd, gamma, gy, None, gy_plus, ds, None, dgb, ds_amax)
    return ds, dgb[0], dgb[1]


class LnGradGroup:
    """Parameter gradients of SEVERAL 256-channel LayerNorm backwards over the same number of rows with ONE reduce launch: every
    backward leaves its per-workgroup partial sums in its own slot (`backward`), `finish()` sums all slots in a fixed order ->
    [n, 2, 256] (dgamma, dbeta) per LayerNorm, in the order of the `backward` calls."""

    def __init__(self, n, rows, device):
        self.n, self.rows, self.used = n, rows, 0
        self.stride = ln_partial_stride(rows)
        self.parts = torch.empty(n * self.stride, dtype=torch.uint8, device=device)

    def backward(self, s, mean, rstd, gamma, gy, gy_plus=None, ds_amax=None):
        """-> ds fp32 (the parameter gradients come from finish())"""
        assert self.used < self.n and s.shape[0] == self.rows
        ds = torch.empty_like(s)
        _lib.call("mpf_res_ln256_backward_partial_amax", s.device,
                  s.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), gy.data_ptr(), None, _lib.ptr(gy_plus), ds.data_ptr(),
                  None, self.rows, self.parts.data_ptr() + self.used * self.stride, self.stride, _lib.ptr(ds_amax),
                  _lib.stream_ptr(s.device))
        self.used += 1
        return ds

    def finish(self):
        out = torch.empty((self.used, 2, 256), dtype=torch.float32, device=self.parts.device)
        _lib.call("mpf_ln_partial_reduce", out.device, self.parts.data_ptr(), self.stride, self.rows, self.used, out.data_ptr(),
                  _lib.stream_ptr(out.device))
        return out
