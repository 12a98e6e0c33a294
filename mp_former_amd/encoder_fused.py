"""The six MSDeformAttn encoder layers of the pixel decoder as ONE autograd node.

Same math as ``MSDeformAttnTransformerEncoderLayer`` x num_layers (reference
mask2former/modeling/pixel_decoder/msdeformattn.py:92-161 with ops/modules/ms_deform_attn.py:82-125
inside, dropout inactive, no padding mask, valid_ratios == 1), scheduled by hand:

* every Linear (forward and input gradient) runs on the split-bf16 fp32 GEMM (csrc/gemm3.hip) with
  its neighbours folded into the epilogue: bias / ReLU / the residual add / the ReLU-backward gate /
  gradient accumulation; ``sampling_offsets`` and ``attention_weights`` are one 288-wide GEMM;
* weight gradients use the split-K "NT" form of the same GEMM, which also returns the column sums of
  the gradient operand (the bias gradients) from its staging loop;
* the positional term is ``pos + level_embed[level]``: its gradient only reaches ``level_embed``, so
  it is obtained from per-level column sums of the 288-wide gradient instead of accumulating a
  [N, S, 256] tensor over the layers.

Used by ``MSDeformAttnTransformerEncoderOnly`` when the inputs are fp32 CUDA tensors and dropout is
inactive; ``MPF_FUSED_ENCODER=0`` selects the layer-by-layer modules (same results to fp32 round-off;
tests/test_encoder_fused_gpu.py).
"""
import ctypes
import math
import os
from collections import namedtuple
from itertools import accumulate, chain, islice

import numpy as np
import torch
from torch.autograd import Function

from . import _lib
from .gemm3 import (amax, amax_slots, gemm3_h2, gemm3_h2_bits, gemm3_nt, gemm3_nt_grouped, nt_reduce_levels, split_weights_grouped_h2,
                    workgroup_slots)
from .msda import host_workspace, ms_deform_attn_backward_raw, ms_deform_attn_forward_raw
from .resln import LnGradGroup, ln256_forward, ln_partial_stride

_EPS = 1e-5

# Range audit of the fp16 x 2 operands (tools/soak.py --range-audit): None, or {operand name: int64 [41] device
# histogram}: bin b counts the rows whose largest magnitude r (relative to what the operand's amax SLOT holds: the scale's
# reference — the true maximum or the upper bound of amax.h) lies in (2^-(b+1), 2^-b], bin 40 everything at or below 2^-40
# incl. all-zero rows.  (floor(-log2 r), not -floor(log2 r), which put every row one bin too high.)
RANGE_AUDIT = None

# Run-time range guard: the fp16 x 2 guarantee is relative to each operand's largest magnitude, so what it
# promises for a ROW depends on how far that row lies below it.  Every RANGE_GUARD_EVERY-th call of the encoder (the third,
# then every 64th: MPF_H2_RANGE_GUARD_EVERY, 0 = off) runs the python-sequenced route and passes every GEMM operand, forward and
# backward, through mpf_h2_range_stats (one read of the operand, two device counters per operand, no synchronisation): rows
# with a non-zero element, and those whose largest magnitude lies below 2^-18 of the slot (where the second piece stops being a
# normal fp16 number).  The counters are copied to pinned memory at the next guarded call and read at the one after (no wait);
# a share above RANGE_GUARD_SHARE warns once per process.  range_guard_report(sync=True) reads them now (tools/soak.py, tests).
RANGE_GUARD_EVERY = int(os.environ.get("MPF_H2_RANGE_GUARD_EVERY", "64"))
RANGE_GUARD_LOG2 = 18
RANGE_GUARD_SHARE = 1e-3
_GUARD_SLOTS = 64
_guard = {"calls": 0, "active": False, "names": {}, "counters": None, "pending": None, "host": None, "warned": False}


def _guard_begin():
    """-> True when this encoder call is a guarded one (counts the call)."""
    n = _guard["calls"]
    _guard["calls"] = n + 1
    if RANGE_GUARD_EVERY <= 0 or RANGE_AUDIT is not None:
        return False
    if not (n == 2 or (n > 2 and (n - 2) % RANGE_GUARD_EVERY == 0) or RANGE_GUARD_EVERY == 1):
        return False
    if _guard["pending"] is not None and _guard["pending"][1].query():          # the copy requested at the last guarded call has landed
        _guard["host"] = _guard["pending"][0].clone()
        _guard["pending"] = None
        _guard_check(_guard["host"])
    if _guard["counters"] is not None and _guard["pending"] is None:
        pinned = torch.empty((_GUARD_SLOTS, 2), dtype=torch.int64).pin_memory()
        pinned.copy_(_guard["counters"], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        _guard["pending"] = (pinned, ev)
    return True


def _guard_shares(host):
    out = {}
    for name, i in _guard["names"].items():
        nz, below = int(host[i, 0]), int(host[i, 1])
        out[name] = {"rows": nz, "below": below, "share": below / nz if nz else 0.0}
    return out


def _guard_check(host):
    bad = {k: v for k, v in _guard_shares(host).items() if v["share"] > RANGE_GUARD_SHARE}
    if bad and not _guard["warned"]:
        import warnings
        _guard["warned"] = True
        worst = max(bad.items(), key=lambda kv: kv[1]["share"])
        warnings.warn("mp_former_amd: fp16 x 2 GEMM operand '%s' has %.3f %% of its non-zero rows below 2^-%d of the operand's largest "
                      "magnitude (%d of %d): those rows keep fewer than 22 bits in the pixel decoder's fp32 GEMMs (DESIGN.md section 2); "
                      "%d operand(s) over the %.1f %% bar" % (worst[0], 100 * worst[1]["share"], RANGE_GUARD_LOG2, worst[1]["below"],
                                                               worst[1]["rows"], len(bad), 100 * RANGE_GUARD_SHARE))


def range_guard_report(sync=False, reset=False):
    """{operand: {"rows", "below", "share"}} of the guarded calls so far: from the last landed copy, or (sync=True) from the
    device counters now — which also applies the warning check."""
    if _guard["counters"] is None:
        return {}
    if sync:
        host = _guard["counters"].cpu()
        _guard_check(host)
    else:
        host = _guard["host"]
        if host is None:
            return {}
    rep = _guard_shares(host)
    if reset:
        _guard["counters"].zero_()
        _guard["host"] = _guard["pending"] = None
        _guard["warned"] = False
    return rep


def _audit(name, t, slot):
    if _guard["active"]:
        if _guard["counters"] is None or _guard["counters"].device != t.device:
            _guard["counters"] = torch.zeros((_GUARD_SLOTS, 2), dtype=torch.int64, device=t.device)
        i = _guard["names"].setdefault(name, len(_guard["names"]))
        if i < _GUARD_SLOTS and t.dim() == 2 and t.stride(1) == 1 and t.shape[1] % 4 == 0 and t.stride(0) % 4 == 0:
            _lib.call("mpf_h2_range_stats", t.device, t.data_ptr(), t.shape[0], t.shape[1], t.stride(0), slot.data_ptr(), RANGE_GUARD_LOG2,
                      _guard["counters"][i].data_ptr(), _lib.stream_ptr(t.device))
    if RANGE_AUDIT is None:
        return
    from .gemm3 import amax_value
    ref = amax_value(slot).clamp_min(1e-38)
    r = (t.detach().abs().amax(1) / ref).clamp(2.0 ** -41, 1.0)
    b = torch.floor(-torch.log2(r)).clamp(0, 40).long()
    h = torch.bincount(b, minlength=41)
    RANGE_AUDIT[name] = h if name not in RANGE_AUDIT else RANGE_AUDIT[name] + h


# ---- the per-layer state, by name ----------------------------------------------------------------------------------------------
# the 16 parameters of a layer in EncoderFn's order: (path of the owning module, field of its weight, field of its bias)
_PARAM_SLOTS = ((("self_attn", "sampling_offsets"), "wso", "bso"), (("self_attn", "attention_weights"), "waw", "baw"),
                (("self_attn", "value_proj"), "wv", "bv"), (("self_attn", "output_proj"), "wo", "bo"), (("norm1",), "g1", "b1"),
                (("linear1",), "w1", "bb1"), (("linear2",), "w2", "bb2"), (("norm2",), "g2", "b2"))
LayerParams = namedtuple("LayerParams", [n for _, w, b in _PARAM_SLOTS for n in (w, b)], defaults=(None,) * (2 * len(_PARAM_SLOTS)))
PARAMS_PER_LAYER = len(LayerParams._fields)
# what a layer's forward keeps for its backward (hbits: the bit mask of the FFN's ReLU gate; None where linear1 is no multiple of 128 wide)
Saved = namedtuple("Saved", "x q value loc attn ao s1 mean1 rstd1 x1 h s2 mean2 rstd2 x_am ao_am x1_am h_am q_am hbits")
# fp16 x 2 planes + amax slot of a layer's weights, W for the forward (p..) and W^T for the input gradients (t..): (suffix, stacked weights)
_PLANE_SRCS = (("v", ("wv",)), ("o", ("wo",)), ("1", ("w1",)), ("2", ("w2",)), ("288", ("wso", "waw")))
FwdPlanes = namedtuple("FwdPlanes", [f"p{k}{am}" for k, _ in _PLANE_SRCS for am in ("", "_am")])
BwdPlanes = namedtuple("BwdPlanes", [f"t{k}{am}" for k, _ in _PLANE_SRCS for am in ("", "_am")])
# amax slots (largest magnitude, or an upper bound of it) of the GEMM operands a layer produces: forward (xn / qn: the next layer's x / q; the
# call's own x, q and positional term follow the layers' slots) and backward
FwdAmax = namedtuple("FwdAmax", "ao_am x1_am h_am xn_am qn_am")
BwdAmax = namedtuple("BwdAmax", "ds2_am dh_am ds1_am draw_am gv_am")


def _records(cls, items, n):
    """-> (n records of ``cls`` filled from consecutive items, the items left over)"""
    it = iter(items)
    return [cls._make(islice(it, len(cls._fields))) for _ in range(n)], tuple(it)


def _put(row, at, rec):
    """the addresses of a record's tensors into a native table's row, each at its field's place (at: {field: index}; other fields are skipped)"""
    for k, t in zip(rec._fields, rec):
        if k in at:
            row[at[k]] = t.data_ptr()


def layer_params(layer):
    """The 16 parameters of an encoder layer as a LayerParams.  The owning modules are looked up once per layer object and
    re-validated per call against the module tree (identity of every child along the path: a swapped submodule rebuilds the
    list); then 16 dict reads — a re-assigned parameter is picked up, and no ``Module.__getattr__`` chain runs (it was ~200 of
    them per step)."""
    owners = layer.__dict__.get("_mpf_param_owners")
    if owners is not None:
        for path, m in owners:
            cur = layer
            for name in path:
                cur = cur._modules.get(name)
                if cur is None:
                    break
            if cur is not m:
                owners = None
                break
    if owners is None:
        owners = []
        for path, _, _ in _PARAM_SLOTS:
            m = layer
            for name in path:
                m = getattr(m, name)
            owners.append((path, m))
        layer.__dict__["_mpf_param_owners"] = owners
    return LayerParams._make(m._parameters[k] for _, m in owners for k in ("weight", "bias"))


def _weight_planes(prm):
    """[(FwdPlanes, BwdPlanes)] of every layer: the fp16 x 2 planes (+ largest magnitude) of every weight in both orientations
    (sampling_offsets | attention_weights stacked into one 288-row operand on the way): two launches for all layers"""
    groups = []
    for p in prm:
        srcs = [[getattr(p, n) for n in names] for _, names in _PLANE_SRCS]
        groups += [(w, False) for w in srcs] + [(w, True) for w in srcs]
    it = chain.from_iterable(split_weights_grouped_h2(groups))
    return [(FwdPlanes._make(islice(it, len(FwdPlanes._fields))), BwdPlanes._make(islice(it, len(BwdPlanes._fields)))) for _ in prm]


def rows_per_split(sizes):
    """Rows per split of the weight-gradient GEMMs: 512 measured best at config B; a divisor of every
    level size when one exists (then no split straddles a level and the per-level column sums of the
    288-wide gradient fall out of the per-split sums), else 512 and ``aligned`` is False."""
    g = 0
    for s_ in sizes:
        g = math.gcd(g, s_)
    for r in (512, 256, 128, 1024, 64, 32):
        if g % r == 0:
            return r, True
    return 512, False


def _wgrad_rps(R, shapes, device, h2=True):
    """Rows per split of ONE grouped launch for the weight gradients [(M_i, N_i)] over the same R rows: as long as the tiles of all
    problems together allow at one round of workgroups (R = 43 008: 40 tiles x 12 splits of 3 584 rows — 19 of 2 272 in the
    fp16 x 2 form — instead of 4 x (4 | 16 tiles x 123 | 31 splits of 352 | 1 376 rows))."""
    slots = workgroup_slots(device)
    tiles = sum(((m + 127) // 128) * ((n + 127) // 128) for m, n in shapes)
    if h2 and all(m % 256 == 0 and n % 256 == 0 for m, n in shapes):
        # 256 x 256 tiles (csrc/gemm3_nt2.h): one 8-wave workgroup per CU, half the operand traffic of the 128 x 128 tiles
        tiles = sum((m // 256) * (n // 256) for m, n in shapes)
        slots = slots // 2
    elif h2:
        slots = slots // 2 * 3        # the fp16 x 2 kernel (159 registers, 32 KB of LDS) is resident three times per CU: measured
    ns = max(1, slots // tiles)       # 1.81 -> 1.45 ms/step against splits sized for two (and 1.86 for four)
    return max(128, ((-(-R // ns)) + 31) // 32 * 32)


def _wgrad_group(pairs, amax_pairs=None):
    """[(dW_i, db_i)] of several Linear layers over the same rows: ONE split-K launch (splits: _wgrad_rps) and ONE reduction."""
    g0 = pairs[0][0]
    rps = _wgrad_rps(g0.shape[0], [(g.shape[1], x.shape[1]) for g, x in pairs], g0.device, amax_pairs is not None)
    return gemm3_nt_grouped(pairs, rps, amax_pairs)


# ---- native forward: one call for all layers (csrc/encoder_layer.hip) -------------------------------------------------------
_ENC_FIELDS = ("pv", "pv_am", "po", "po_am", "p1", "p1_am", "p2", "p2_am", "p288", "p288_am", "bv", "bo", "bb1", "bb2", "b288", "g1", "b1",
               "g2", "b2", "value", "raw", "loc", "attn", "ao", "s1", "mean1", "rstd1", "x1", "h", "hbits", "s2", "mean2", "rstd2", "x2", "qn",
               "ao_am", "x1_am", "h_am", "xn_am", "qn_am")
_ENC_AT = {k: i for i, k in enumerate(_ENC_FIELDS)}
_NATIVE_FWD = os.environ.get("MPF_ENCODER_NATIVE", "1") != "0"        # (0: the python-sequenced forward / backward the tests compare with)
_NATIVE_BWD = _NATIVE_FWD
# calls of EncoderFn by the route they took (the two routes launch the same kernels, so nothing in the kernel log tells them apart;
# the tests that compare the routes assert on these)
ROUTE_CALLS = {"native_fwd": 0, "python_fwd": 0, "native_bwd": 0, "python_bwd": 0}


class MpfEncoderCall(ctypes.Structure):
    _fields_ = [("N", ctypes.c_int32), ("S", ctypes.c_int32), ("M", ctypes.c_int32), ("L", ctypes.c_int32), ("P", ctypes.c_int32),
                ("nl", ctypes.c_int32), ("F", ctypes.c_int32), ("reserved", ctypes.c_int32), ("eps", ctypes.c_float), ("pad_", ctypes.c_float),
                ("host_shapes", ctypes.c_void_p), ("shapes_dev", ctypes.c_void_p), ("lsi_dev", ctypes.c_void_p), ("ref", ctypes.c_void_p),
                ("pos_full", ctypes.c_void_p), ("pos_am", ctypes.c_void_p), ("x0", ctypes.c_void_p), ("x0_am", ctypes.c_void_p),
                ("q0", ctypes.c_void_p), ("q0_am", ctypes.c_void_p), ("layers", ctypes.c_void_p)]


def _native_forward_applies(guarded, meta, C, prm):
    """the one-call forward takes: an unguarded, unaudited call, level shapes with a host copy, C = 256, 8 heads, one FFN width in
    every layer, a multiple of 128 (the ReLU gate's bit mask)"""
    F = prm[0].w1.shape[0]
    return (_NATIVE_FWD and RANGE_AUDIT is None and not guarded and getattr(meta["shapes"], "_mpf_host", None) is not None and C == 256
            and meta["n_heads"] == 8 and F % 128 == 0 and all(p.w1.shape[0] == F for p in prm))


def _arena_members(rows, C, F, no, M, L, P):
    """(name, shape, dtype) of what the native forward leaves per layer, in arena order; rows = (R,) or (N, S): loc / attn keep the
    row dimensions as the MSDA calls take them.  (hbits: a bit per element of h in bytes, R F / 32 floats for every F % 32 == 0)"""
    R, f32 = math.prod(rows), torch.float32
    return (("value", (R, C), f32), ("raw", (R, no), f32), ("loc", (*rows, M, L, P, 2), f32), ("attn", (*rows, M, L, P), f32), ("ao", (R, C), f32),
            ("s1", (R, C), f32), ("mean1", (R,), f32), ("rstd1", (R,), f32), ("x1", (R, C), f32), ("h", (R, F), f32),
            ("hbits", (R, F // 8), torch.uint8), ("s2", (R, C), f32), ("mean2", (R,), f32), ("rstd2", (R,), f32), ("x2", (R, C), f32),
            ("qn", (R, C), f32))


_arena_layouts = {}


def _arena_layout(R, C, F, no, M, L, P):
    """float offsets of a layer's results inside its slice of the arena (every tensor 16-byte aligned); -> ({name: (offset, numel)}, floats per layer)"""
    key = (R, C, F, no, M, L, P)
    hit = _arena_layouts.get(key)
    if hit is None:
        offs, tot = {}, 0
        for name, shape, dt in _arena_members((R,), C, F, no, M, L, P):
            n = math.prod(shape) * dt.itemsize // 4
            offs[name] = (tot, n)
            tot += (n + 3) // 4 * 4
        hit = _arena_layouts[key] = (offs, tot)
    return hit


def _native_forward(x, x_am, q_am, pos_full, pos_am, prm, planes, b288_all, ams, meta, dims):
    """The forward of all layers as ONE native call writing into one arena; -> ([Saved], the last layer's output [R, C]): views of it"""
    N, S, C = dims
    R, nl, F = N * S, len(prm), prm[0].w1.shape[0]
    M, L, P = meta["n_heads"], meta["n_levels"], meta["n_points"]
    no3 = M * L * P * 3
    lib = _lib.lib()
    if lib.mpf_encoder_fields() != len(_ENC_FIELDS):
        raise RuntimeError("MpfEncoderCall field table differs between encoder_fused.py and libmpformer_hip.so")
    q = (x.view(N, S, C) + pos_full).view(R, C)
    amax(q, q_am)
    offs, per = _arena_layout(R, C, F, no3, M, L, P)
    arena = torch.empty((nl, per), dtype=torch.float32, device=x.device)
    tab = np.zeros((nl, len(_ENC_FIELDS)), dtype=np.uint64)
    for row, p, w, am, b288, a in zip(tab, prm, planes, ams, b288_all, arena):
        for rec in (p, w, am):
            _put(row, _ENC_AT, rec)
        row[_ENC_AT["b288"]] = b288.data_ptr()
        for k, (o, _) in offs.items():
            row[_ENC_AT[k]] = a.data_ptr() + 4 * o
    assert tab.all(), "a field of _ENC_FIELDS that no record fills"
    host_shapes = meta["shapes"]._mpf_host
    call = MpfEncoderCall(N, S, M, L, P, nl, F, 0, _EPS, 0.0, host_shapes.data_ptr(), meta["shapes"].data_ptr(), meta["lsi"].data_ptr(),
                          meta["ref"].data_ptr(), pos_full.data_ptr(), pos_am.data_ptr(), x.data_ptr(), x_am.data_ptr(), q.data_ptr(),
                          q_am.data_ptr(), tab.ctypes.data)
    _lib.call("mpf_encoder_forward", x.device, ctypes.byref(call), _lib.stream_ptr(x.device))
    saved, members = [], _arena_members((N, S), C, F, no3, M, L, P)
    for am, a in zip(ams, arena):
        t = {k: a[offs[k][0]:sum(offs[k])].view(dt).view(shape) for k, shape, dt in members}      # the layer's arena slice by member
        saved.append(Saved(x=x, q=q, x_am=x_am, q_am=q_am, ao_am=am.ao_am, x1_am=am.x1_am, h_am=am.h_am,
                           **{k: v for k, v in t.items() if k in Saved._fields}))
        x, q, x_am, q_am = t["x2"], t["qn"], am.xn_am, am.qn_am
    return saved, x


def _python_forward(x, x_am, q_am, pos_full, pos_am, prm, planes, b288_all, ams, meta, dims):
    """The same forward sequenced here, one ctypes call and one allocation per kernel (the range guard and the audit see every
    GEMM operand on this route); -> ([Saved], the last layer's output [R, C])"""
    N, S, C = dims
    R, M, shapes = N * S, meta["n_heads"], meta["shapes"]
    host_shapes = getattr(shapes, "_mpf_host", None)
    saved, q = [], None
    for i, (p, w, am, b288) in enumerate(zip(prm, planes, ams, b288_all)):
        _audit("fwd x (value_proj)", x, x_am)
        value = gemm3_h2(x, x_am, w.pv, w.pv_am, p.bv, out_amax=am.ao_am)
        if q is None:       # layer 0; later layers get src + pos from the previous layer's norm2 pass
            q = (x.view(N, S, C) + pos_full).view(R, C)
            amax(q, q_am)
        _audit("fwd q (offsets | weights)", q, q_am)
        raw = gemm3_h2(q, q_am, w.p288, w.p288_am, b288)
        # softmax over the 12 logits, loc = ref + offset / (W_l, H_l) happen inside the MSDA kernel
        ao, loc, attn = ms_deform_attn_forward_raw(value.view(N, S, M, C // M), shapes, meta["lsi"], raw, meta["ref"], host_shapes)
        ao = ao.view(R, C)
        _audit("fwd attention output (output_proj)", ao, am.ao_am)
        s1 = gemm3_h2(ao, am.ao_am, w.po, w.po_am, p.bo, cin=x)
        x1, mean1, rstd1, _ = ln256_forward(s1, p.g1, p.b1, _EPS, y_bound=am.x1_am)
        # (the ReLU's gate leaves the product as a bit mask: the backward then reads 1 bit instead of 4 bytes per element of h)
        if w.p1.shape[1] % 128 == 0:
            h, hbits = gemm3_h2_bits(x1, am.x1_am, w.p1, w.p1_am, p.bb1, relu=True, out_amax=am.h_am, want_bits=True)
        else:
            h, hbits = gemm3_h2(x1, am.x1_am, w.p1, w.p1_am, p.bb1, relu=True, out_amax=am.h_am), None
        _audit("fwd x1 (linear1)", x1, am.x1_am)
        _audit("fwd hidden (linear2)", h, am.h_am)
        s2 = gemm3_h2(h, am.h_am, w.p2, w.p2_am, p.bb2, cin=x1)
        last = i + 1 == len(prm)
        x2, mean2, rstd2, qn = ln256_forward(s2, p.g2, p.b2, _EPS, padd=None if last else pos_full, y_bound=am.xn_am,
                                             padd_amax=None if last else pos_am, yplus_bound=None if last else am.qn_am)
        saved.append(Saved(x, q, value, loc, attn, ao, s1, mean1, rstd1, x1, h, s2, mean2, rstd2, x_am, am.ao_am, am.x1_am, am.h_am, q_am, hbits))
        x, q, x_am, q_am = x2, qn, am.xn_am, am.qn_am
    return saved, x


# ---- native backward: one call for all layers ---------------------------------------------------------------------------------
_ENCB_FIELDS = ("x", "q", "value", "loc", "attn", "ao", "s1", "mean1", "rstd1", "x1", "h", "hbits", "s2", "mean2", "rstd2",
                "x_am", "q_am", "ao_am", "x1_am", "h_am", "g1", "g2", "tv", "tv_am", "to", "to_am", "t1", "t1_am", "t2", "t2_am", "t288", "t288_am",
                "ds2_am", "dh_am", "ds1_am", "draw_am", "gv_am", "wgrad", "dw288", "lvl", "db288")
_ENCB_AT = {k: i for i, k in enumerate(_ENCB_FIELDS)}


class MpfEncoderBwdCall(ctypes.Structure):
    _fields_ = [("N", ctypes.c_int32), ("S", ctypes.c_int32), ("M", ctypes.c_int32), ("L", ctypes.c_int32), ("P", ctypes.c_int32),
                ("nl", ctypes.c_int32), ("F", ctypes.c_int32), ("rps288", ctypes.c_int32), ("rps_group", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("group_stride", ctypes.c_int64), ("host_shapes", ctypes.c_void_p), ("gout", ctypes.c_void_p),
                ("split_level", ctypes.c_void_p), ("ds2", ctypes.c_void_p), ("dh", ctypes.c_void_p), ("dx1", ctypes.c_void_p),
                ("ds1", ctypes.c_void_p), ("dao", ctypes.c_void_p), ("gv", ctypes.c_void_p), ("draw", ctypes.c_void_p),
                ("dq", ctypes.c_void_p * 2), ("g", ctypes.c_void_p * 2), ("cpart288", ctypes.c_void_p), ("cs288", ctypes.c_void_p),
                ("part_group", ctypes.c_void_p), ("ln_parts", ctypes.c_void_p), ("ln_stride", ctypes.c_uint64), ("msda_ws", ctypes.c_void_p),
                ("msda_ws_bytes", ctypes.c_uint64), ("dgb_out", ctypes.c_void_p), ("layers", ctypes.c_void_p)]


def _native_backward_applies(guarded, meta, aligned, C, prm, saved):
    """the one-call backward takes what the one-call forward takes and left behind (a gate bit mask in every layer), with an FFN
    width that is a multiple of 256 (the 256 x 256 weight-gradient tiles), level-aligned splits and at most 4 levels"""
    F = prm[0].w1.shape[0]
    return (_NATIVE_BWD and RANGE_AUDIT is None and not guarded and getattr(meta["shapes"], "_mpf_host", None) is not None and aligned
            and meta["n_levels"] <= 4 and C == 256 and meta["n_heads"] == 8 and F % 256 == 0
            and all(s.hbits is not None and p.w1.shape[0] == F for s, p in zip(saved, prm)))


def _native_backward(gout, prm, saved, planes_t, meta, dims, rps, split_level):
    """The backward of all layers as ONE native call (csrc/encoder_layer.hip, mpf_encoder_backward): same launches, same
    arguments as _python_backward.  -> (d input [R, C], [LayerParams of gradients] (LayerNorm's still open), dgb [2 nl, 2, 256],
    per-level column sums of every layer's d raw [nl, L, 288])"""
    N, S, C = dims
    R, nl, F = N * S, len(prm), prm[0].w1.shape[0]
    M, L, P = meta["n_heads"], meta["n_levels"], meta["n_points"]
    no, no3 = M * L * P * 2, M * L * P * 3
    dev, lib = gout.device, _lib.lib()
    if lib.mpf_encoder_bwd_fields() != len(_ENCB_FIELDS):
        raise RuntimeError("MpfEncoderBwdCall field table differs between encoder_fused.py and libmpformer_hip.so")
    wgrads = (("w2", "bb2", C, F), ("w1", "bb1", F, C), ("wo", "bo", C, C), ("wv", "bv", C, C))      # the grouped launch's order
    rpg = _wgrad_rps(R, [(m_, n_) for _, _, m_, n_ in wgrads], dev)
    ns288, nsg = (R + rps - 1) // rps, (R + rpg - 1) // rpg
    gstride = sum(m_ * n_ + m_ for _, _, m_, n_ in wgrads)
    # results of every layer, and the temporaries all layers share: name -> float offset
    outs = (("wgrad", gstride), ("dw288", no3 * C), ("lvl", L * no3), ("db288", no3))      # wgrad: the four weight gradients + biases; dw288: dW288^T
    tmps = (("ds2", R * C), ("dx1", R * C), ("ds1", R * C), ("dao", R * C), ("gv", R * C), ("dh", R * F), ("draw", R * no3), ("dq0", R * C),
            ("dq1", R * C), ("g0", R * C), ("g1", R * C), ("cpart", ns288 * no3 * C), ("cs", ns288 * no3), ("pgroup", nsg * gstride))
    oo = dict(zip((k for k, _ in outs), accumulate((n for _, n in outs), initial=0)))
    ot = dict(zip((k for k, _ in tmps), accumulate((n for _, n in tmps), initial=0)))
    out = torch.empty((nl, sum(n for _, n in outs)), dtype=torch.float32, device=dev)
    tmp = torch.empty(sum(n for _, n in tmps), dtype=torch.float32, device=dev)
    t = {k: tmp.data_ptr() + 4 * o for k, o in ot.items()}
    ln_stride = ln_partial_stride(R)
    ln_parts = torch.empty(2 * nl * ln_stride, dtype=torch.uint8, device=dev)
    host_shapes = meta["shapes"]._mpf_host
    stream = _lib.stream_ptr(dev)
    ws = host_workspace(dev, stream, N, M, L, S, P, host_shapes)
    dgb = torch.empty((2 * nl, 2, 256), dtype=torch.float32, device=dev)
    ams, _ = _records(BwdAmax, amax_slots(len(BwdAmax._fields) * nl, dev).unbind(0), nl)
    tab = np.zeros((nl, len(_ENCB_FIELDS)), dtype=np.uint64)
    for row, p, s, w, am, o_ in zip(tab, prm, saved, planes_t, ams, out):
        for rec in (s, p, w, am):                  # (of the parameters the table has g1 and g2)
            _put(row, _ENCB_AT, rec)
        for k, o in oo.items():
            row[_ENCB_AT[k]] = o_.data_ptr() + 4 * o
    assert tab.all(), "a field of _ENCB_FIELDS that no record fills"
    call = MpfEncoderBwdCall(N, S, M, L, P, nl, F, rps, rpg, 0, gstride, host_shapes.data_ptr(), gout.data_ptr(), split_level.data_ptr(),
                             t["ds2"], t["dh"], t["dx1"], t["ds1"], t["dao"], t["gv"], t["draw"], (ctypes.c_void_p * 2)(t["dq0"], t["dq1"]),
                             (ctypes.c_void_p * 2)(t["g0"], t["g1"]), t["cpart"], t["cs"], t["pgroup"],
                             ln_parts.data_ptr(), ln_stride, ws.data_ptr(), ws.numel(), dgb.data_ptr(), tab.ctypes.data)
    _lib.call("mpf_encoder_backward", dev, ctypes.byref(call), stream)
    dprm = []
    for o_ in out:
        dw288, db288 = o_[oo["dw288"]:oo["lvl"]].view(no3, C), o_[oo["db288"]:]
        d, k = {}, 0
        for w, b, m_, n_ in wgrads:
            d[w], d[b] = o_[k:k + m_ * n_].view(m_, n_), o_[k + m_ * n_:k + m_ * n_ + m_]
            k += m_ * n_ + m_
        dprm.append(LayerParams(wso=dw288[:no], bso=db288[:no], waw=dw288[no:], baw=db288[no:], **d))
    g = tmp[ot["g0"]:ot["g0"] + R * C].view(R, C)              # g[0]: what layer 0 hands down
    return g, dprm, dgb, out[:, oo["lvl"]:oo["db288"]].view(nl, L, no3)


def _python_backward(g, prm, saved, planes_t, meta, dims, rps, aligned, split_level):
    """The same backward sequenced here; -> as _native_backward"""
    N, S, C = dims
    R, nl = N * S, len(prm)
    M, L = meta["n_heads"], meta["n_levels"]
    sizes, host_shapes = meta["sizes"], getattr(meta["shapes"], "_mpf_host", None)
    no = M * L * meta["n_points"] * 2
    ams, _ = _records(BwdAmax, amax_slots(len(BwdAmax._fields) * nl, g.device).unbind(0), nl)
    dprm, lvls, gq = [None] * nl, [None] * nl, None
    lng = LnGradGroup(2 * nl, R, g.device)           # the 2 nl LayerNorm parameter gradients: one reduce launch at the end
    for i in reversed(range(nl)):
        p, s, t, am = prm[i], saved[i], planes_t[i], ams[i]
        # norm2 <- ffn
        ds2 = lng.backward(s.s2, s.mean2, s.rstd2, p.g2, g, gq, ds_amax=am.ds2_am)
        if s.hbits is not None:
            dh = gemm3_h2_bits(ds2, am.ds2_am, t.t2, t.t2_am, gate_bits=s.hbits, out_amax=am.dh_am)
        else:
            dh = gemm3_h2(ds2, am.ds2_am, t.t2, t.t2_am, gate=s.h, out_amax=am.dh_am)
        _audit("bwd ds2 (d linear2 output)", ds2, am.ds2_am)
        _audit("bwd dh (d hidden)", dh, am.dh_am)
        dx1 = gemm3_h2(dh, am.dh_am, t.t1, t.t1_am, cin=ds2)
        # norm1 <- attention
        ds1 = lng.backward(s.s1, s.mean1, s.rstd1, p.g1, dx1, ds_amax=am.ds1_am)
        _audit("bwd ds1 (d output_proj output)", ds1, am.ds1_am)
        dao = gemm3_h2(ds1, am.ds1_am, t.to, t.to_am)
        # d(raw): the softmax / offset-normaliser backward is the epilogue of the push kernel
        # (the bin + tile kernels record the largest magnitudes of gv / draw themselves: no amax pass over the two tensors)
        gv, draw = ms_deform_attn_backward_raw(s.value.view(N, S, M, C // M), host_shapes, s.loc, s.attn, dao.view(N, S, C), s.ao.view(N, S, C),
                                               am.draw_am, am.gv_am)
        _audit("bwd draw (d offsets | weights)", draw, am.draw_am)
        _audit("bwd grad_value (d value_proj output)", gv.view(R, C), am.gv_am)
        dq = gemm3_h2(draw, am.draw_am, t.t288, t.t288_am)
        # dW288^T = q^T . draw (288 on the 96-wide tile side) + per-split column sums of draw: the
        # bias gradient and, summed per level, the level_embed gradient
        cpart, _, cs = gemm3_nt(s.q, draw, rps, want_csum_b=True, transpose_out=True, amax_ab=(s.q_am, am.draw_am))
        if aligned and L <= 4 and cpart[0].numel() % 4 == 0:
            dw288, lvl, db288 = nt_reduce_levels(cpart, cs, split_level, L)     # one launch, fixed order
        else:
            dw288 = cpart.sum(0)
            if aligned:
                lvl = torch.zeros((L, draw.shape[1]), dtype=torch.float32, device=g.device).index_add_(0, split_level, cs)
            else:
                lvl = torch.stack([sl.sum((0, 1)) for sl in draw.view(N, S, -1).split(sizes, 1)])   # [L, 288]
            db288 = lvl.sum(0)
        lvls[i] = lvl
        gv2 = gv.view(R, C)
        # grad wrt this layer's input: through value_proj + the residual; the (src + pos) path (dq)
        # joins inside the previous layer's norm2 backward (layer 0: added here)
        g = gemm3_h2(gv2, am.gv_am, t.tv, t.tv_am, cin=ds1, cin2=dq if i == 0 else None)
        gq = dq
        # the four plain weight gradients of the layer (their operands are all alive here) as one launch
        (w2, bb2), (w1, bb1), (wo, bo), (wv, bv) = _wgrad_group(
            [(ds2, s.h), (dh, s.x1), (ds1, s.ao), (gv2, s.x)], [(am.ds2_am, s.h_am), (am.dh_am, s.x1_am), (am.ds1_am, s.ao_am), (am.gv_am, s.x_am)])
        dprm[i] = LayerParams(wso=dw288[:no], bso=db288[:no], waw=dw288[no:], baw=db288[no:], wv=wv, bv=bv, wo=wo, bo=bo, w1=w1, bb1=bb1,
                              w2=w2, bb2=bb2)
    return g, dprm, lng.finish(), torch.stack(lvls)


class EncoderFn(Function):
    @staticmethod
    def forward(ctx, src, pos_const, level_embed, meta, *params):
        # src [N, S, C] fp32; pos_const [S, C] (sine embedding, constant); level_embed [L, C]; params: LayerParams x layers, flat
        N, S, C = src.shape
        prm, _ = _records(LayerParams, params, len(params) // PARAMS_PER_LAYER)
        nl = len(prm)
        pos_full = pos_const + level_embed.index_select(0, meta["level_idx"])           # [S, C]
        x = src.reshape(N * S, C)
        planes = _weight_planes(prm)
        # the 288-wide bias of every layer in one concatenation
        b288_all = torch.cat([t for p in prm for t in (p.bso, p.baw)]).view(nl, -1)
        # amax slots of every GEMM operand: x / q of layer 0 and the positional term by a pass over the data; the rest from their producers —
        # LayerNorm outputs bounded from (gamma, beta), the attention output by max |value| (a convex combination of rows), the FFN hidden from its GEMM
        ams, (x_am, q_am, pos_am) = _records(FwdAmax, amax_slots(len(FwdAmax._fields) * nl + 3, src.device).unbind(0), nl)
        amax(x, x_am)
        amax(pos_full, pos_am)
        ctx.guarded = guarded = _guard_begin()
        native = _native_forward_applies(guarded, meta, C, prm)
        ROUTE_CALLS["native_fwd" if native else "python_fwd"] += 1
        _guard["active"] = guarded                  # (the operands of this call go through mpf_h2_range_stats in _audit)
        try:
            saved, x = (_native_forward if native else _python_forward)(x, x_am, q_am, pos_full, pos_am, prm, [f for f, _ in planes], b288_all,
                                                                        ams, meta, (N, S, C))
        finally:
            _guard["active"] = False
        ctx.save_for_backward(*params, *chain.from_iterable(saved))
        ctx.meta, ctx.nl, ctx.dims = meta, nl, (N, S, C)
        ctx.planes_t = [t for _, t in planes]       # (W^T planes, amax) for the backward
        # the native route's x2 is a view of the arena every layer's saved tensors live in.  When nothing will back-propagate
        # (eval / no_grad: autograd drops the saved tensors) a view would keep those ~0.6 GB per layer alive for as long as
        # the caller holds `memory` — hand out a copy then
        return x.view(N, S, C).clone() if native and not any(ctx.needs_input_grad) else x.view(N, S, C)

    @staticmethod
    def backward(ctx, gout):
        N, S, C = ctx.dims
        meta, nl = ctx.meta, ctx.nl
        prm, rest = _records(LayerParams, ctx.saved_tensors, nl)
        saved, _ = _records(Saved, rest, nl)
        g = gout.reshape(N * S, C).contiguous()
        rps, aligned = rows_per_split(meta["sizes"])
        split_level = None
        if aligned:
            key = ("split_level", rps, N)
            split_level = meta.get(key)
            if split_level is None:
                split_level = meta["level_idx"][::rps].repeat(N)          # level of every split's rows
                meta[key] = split_level
        guarded = bool(getattr(ctx, "guarded", False))
        native = _native_backward_applies(guarded, meta, aligned, C, prm, saved)
        ROUTE_CALLS["native_bwd" if native else "python_bwd"] += 1
        if native:
            g, dprm, dgb, lvls_all = _native_backward(g, prm, saved, ctx.planes_t, meta, (N, S, C), rps, split_level)
        else:
            _guard["active"] = guarded
            try:
                g, dprm, dgb, lvls_all = _python_backward(g, prm, saved, ctx.planes_t, meta, (N, S, C), rps, aligned, split_level)
            finally:
                _guard["active"] = False
        # LayerNorm parameter gradients into their places; dgb [2 nl, (gamma, beta), 256] in call order: (norm2, norm1) of layers nl - 1 .. 0
        for z, i in enumerate(reversed(range(nl))):
            dprm[i] = dprm[i]._replace(g2=dgb[2 * z, 0], b2=dgb[2 * z, 1], g1=dgb[2 * z + 1, 0], b1=dgb[2 * z + 1, 1])
        # d level_embed = sum_i lvl_i . [W_offsets_i ; W_weights_i] (lvls_all [nl, L, 288]: per-level column sums of every layer's
        # d raw): one stacked product for all layers
        w288_all = torch.cat([t for p in prm for t in (p.wso, p.waw)]).view(nl, -1, C)
        # [nl, L, 288] x [nl, 288, C] summed over the layers: 1.3 M multiply-adds — as a broadcast product + one reduction
        # (the library's batched fp32 GEMM for it was the head's last hipBLASLt launch)
        d_level = (lvls_all[:, :, :, None] * w288_all[:, None, :, :]).sum((0, 2))
        return (g.view(N, S, C), None, d_level, None, *chain.from_iterable(dprm))
