"""Route table of the gemm3 host layer (csrc/gemm3.hip): which kernel every entry point picks for the smallest shapes on each
side of each routing threshold, what it logs as algorithmic bytes / flops, and the bits it writes.

    python tools/record_gemm3_routes.py [--out tests/golden/gemm3_routes.json]

runs CASES on cuda:0 and writes the fixture that tests/test_gemm3_routes_gpu.py compares the library against.  Record it from
the library BEFORE a change of the host layer; the test then pins the change.  Every case names the route it is there for
(``expect`` / ``avoid``, valid on a 256-CU device); recording fails if a case does not reach it.

Per case the fixture holds: the kernel name (mpf_last_kernel), the launch log's bytes and flops, and the SHA-256 of every
output buffer whose bits are a function of the inputs.  The per-split COLUMN SUMS are not: the NT kernels add the threads'
running sums of a column with float atomics in LDS, in whatever order the waves arrive, so two runs of one library differ in
the last bits (``--hash-sums`` records their hashes next to the others to show it).  They are checked against the exact sums
instead, within the rounding of an fp32 sum of that many terms in any order (``sums``: worst |got - exact| / bound per buffer,
must be <= 1; the fixture keeps the buffer names).  The out_amax slot is hashed twice: ``out_amax`` is the value its consumers
read (the largest of the 16 sub-slots), ``out_amax_slot`` the raw slot — which sub-slot a workgroup writes follows the tiling,
so like the kernel name the raw slot is only comparable between devices with the same number of CUs.
"""
import argparse
import contextlib
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm3_routes.json")

DEFAULTS = {"gemm3_mixed_tiles": 1, "gemm3_two_pass": 256, "gemm3_two_pass_rows": 0, "gemm3_ws": 512, "gemm3_tn3": 1,
            "gemm3_tn3_176": 1, "gemm3_nt2": 1}
DEVICE_DEPENDENT = ("out_amax_slot",)      # hashes that follow the tiling (compared like the kernel name)

TN = "gemm3_tn_kernel"
TWO_PASS_H2 = (TN + "<h2 96x256>", TN + "<h2 128x256>")


def _case(cid, entry, shape, expect=None, avoid=None, opts=None, **kw):
    """expect: the kernel name (or a tuple of acceptable names, or ``~substring``); avoid: a substring the name must not have"""
    return dict(id=cid, entry=entry, shape=shape, expect=expect, avoid=avoid, opts=opts or {}, **kw)


def _cases():
    c = []
    # ---- mpf_gemm3_tn: (M, N), K = 32
    for a2 in (False, True):
        s = "+a2" if a2 else ""
        c.append(_case(f"tn 130x128{s}", "tn", (130, 128, 32), TN + "<128>", a2=a2))
        c.append(_case(f"tn 130x288{s}", "tn", (130, 288, 32), TN + "<96>", a2=a2, bias=a2, relu=a2))
    c.append(_case("tn 130x100 partial column tile", "tn", (130, 100, 32), TN + "<128>", bias=True, cin=True))
    c.append(_case("tn 66500x128", "tn", (66500, 128, 32), TN + "<128+64>"))
    c.append(_case("tn 33200x256+a2", "tn", (33200, 256, 32), TN + "<128+64>", a2=True, bias=True))
    c.append(_case("tn 98304x128 tail 256", "tn", (98304, 128, 32), TN + "<128+64>"))
    c.append(_case("tn 98305x128 tail 257", "tn", (98305, 128, 32), TN + "<128>"))
    c.append(_case("tn 66500x128 mixed off", "tn", (66500, 128, 32), TN + "<128>", opts={"gemm3_mixed_tiles": 0}))
    c.append(_case("tn 1000x256", "tn", (1000, 256, 32), TN + "<96x256>", bias=True, cin=True, relu=True))
    c.append(_case("tn 65536x256", "tn", (65536, 256, 32), TN + "<128x256>"))
    c.append(_case("tn 1000x256 rows=128", "tn", (1000, 256, 32), TN + "<128x256>", opts={"gemm3_two_pass_rows": 128}))
    c.append(_case("tn 1000x256 two_pass=0", "tn", (1000, 256, 32), avoid="x256", opts={"gemm3_two_pass": 0}))
    c.append(_case("tn 1000x256 two_pass=512", "tn", (1000, 256, 32), avoid="x256", opts={"gemm3_two_pass": 512}))
    # ---- mpf_gemm3_tn_h2 / _h2_bits
    ws = (77, 512, 256)
    c.append(_case("h2 ws plain", "tn_h2", ws, TN + "<h2 ws>", out_amax=True))
    c.append(_case("h2 ws addend", "tn_h2", ws, TN + "<h2 ws>", cin=True, bias=True))
    c.append(_case("h2 ws relu", "tn_h2", ws, TN + "<h2 ws>", relu=True))
    c.append(_case("h2 ws relu addend", "tn_h2", ws, TN + "<h2 ws>", relu=True, cin=True))
    c.append(_case("h2 ws relu mask out", "tn_h2_bits", ws, TN + "<h2 ws>", relu=True, bits_out=True, out_amax=True))
    c.append(_case("h2 ws mask gate", "tn_h2_bits", ws, TN + "<h2 ws>", gate_bits=True))
    c.append(_case("h2 ws mask gate addend", "tn_h2_bits", ws, TN + "<h2 ws>", gate_bits=True, cin=True))
    c.append(_case("h2 mask out without relu: no ws instantiation", "tn_h2_bits", ws, TN + "<h2 96x256>", bits_out=True))
    c.append(_case("h2 77x256 K=256: N below the ws threshold", "tn_h2", (77, 256, 256), avoid="ws"))
    c.append(_case("h2 ws shape with gate", "tn_h2", ws, avoid="ws", gate=True))
    c.append(_case("h2 ws shape with cin2", "tn_h2", ws, avoid="ws", cin2=True))
    c.append(_case("h2 ws shape ws=0", "tn_h2", ws, avoid="ws", opts={"gemm3_ws": 0}))
    c.append(_case("h2 43008x256", "tn_h2", (43008, 256, 32), TN + "<h2 192x256:176>", bias=True, out_amax=True))
    c.append(_case("h2 49152x256", "tn_h2", (49152, 256, 32), TN + "<h2 192x256>"))
    c.append(_case("h2 9216x1024 K=64: 192 tiles", "tn_h2", (9216, 1024, 64), "~192x256"))
    c.append(_case("h2 9024x1024 K=64: 188 tiles", "tn_h2", (9024, 1024, 64), TWO_PASS_H2))
    c.append(_case("h2 16800x256", "tn_h2", (16800, 256, 32), TN + "<h2 96x256>", relu=True, cin=True))
    c.append(_case("h2 2047x256 tn3=2", "tn_h2", (2047, 256, 32), avoid="192x256", opts={"gemm3_tn3": 2}))
    c.append(_case("h2 2048x256 tn3=2", "tn_h2", (2048, 256, 32), "~192x256", opts={"gemm3_tn3": 2}))
    c.append(_case("h2 43008x256 tn3=0", "tn_h2", (43008, 256, 32), avoid="192x256", opts={"gemm3_tn3": 0}))
    c.append(_case("h2 43008x256 tn3_176=0", "tn_h2", (43008, 256, 32), TN + "<h2 192x256>", opts={"gemm3_tn3_176": 0}))
    c.append(_case("h2 333x128", "tn_h2", (333, 128, 32), TN + "<h2 128>", bias=True, gate=True))
    c.append(_case("h2 333x288", "tn_h2", (333, 288, 32), TN + "<h2 96>", out_amax=True))
    # ---- mpf_gemm3_tn_ex
    c.append(_case("ex a16 300x288", "tn_ex", (300, 288, 64), TN + "<a16>", a16=True, bias=True))
    c.append(_case("ex a16 300x256", "tn_ex", (300, 256, 64), TN + "<a16>", a16=True, cin=True, relu=True))
    c.append(_case("ex c16 300x128", "tn_ex", (300, 128, 64), TN + "<c16>", c16=True, bias=True))
    c.append(_case("ex c16 300x256", "tn_ex", (300, 256, 64), TN + "<96x256>", c16=True))
    # ---- mpf_gemm3_conv3x3 / _h2: (images, H, W, Cin, Cout)
    for tr in (0, 1):
        c.append(_case(f"conv 5x12 32->96 t{tr}", "conv", (1, 5, 12, 32, 96), "gemm3_conv_kernel", transposed=tr, bias=not tr))
        c.append(_case(f"conv 5x8 32->256 t{tr}", "conv", (1, 5, 8, 32, 256), "gemm3_conv_kernel", transposed=tr))
        c.append(_case(f"conv 5x8 32->256 two_pass=0 t{tr}", "conv", (1, 5, 8, 32, 256), "gemm3_conv_kernel", transposed=tr,
                       opts={"gemm3_two_pass": 0}))
        c.append(_case(f"conv h2 5x8 32->256 t{tr}", "conv_h2", (1, 5, 8, 32, 256), "gemm3_conv_kernel<h2>", transposed=tr,
                       bias=bool(tr), out_amax=True))
    # ---- NT family: (R, Mdim, Ndim, rows_per_split)
    for h2 in (False, True):
        e, s = ("nt_h2", "h2") if h2 else ("nt", "")
        c.append(_case(f"{e} 100x36", e, (1000, 100, 36, 128), "gemm3_nt_kernel<96>" + s, csum_a=True, csum_b=True))
        c.append(_case(f"{e} 100x128", e, (1000, 100, 128, 128), "gemm3_nt_kernel<128>" + s))
        c.append(_case(f"{e} 100x36 transpose_out", e, (1000, 100, 36, 128), "gemm3_nt_kernel<96>" + s, transpose_out=True, csum_a=True))
    c.append(_case("nt 100x128 b2", "nt", (1000, 100, 128, 128), "gemm3_nt_kernel<128>", b2=True, csum_b=True))
    c.append(_case("nt_ex a16", "nt_ex", (1000, 100, 128, 128), "gemm3_nt_kernel<a16>", a16=True, csum_a=True))
    c.append(_case("nt_ex b16", "nt_ex", (1000, 100, 128, 128), "gemm3_nt_kernel<b16>", b16=True))
    c.append(_case("nt_grouped two items", "nt_grouped", (1000, 128), "gemm3_nt_group_kernel", items=((100, 36), (64, 128))))
    big = ((256, 256), (512, 256))
    c.append(_case("nt_grouped_h2 256-multiples", "nt_grouped_h2", (256, 128), "gemm3_nt_group_kernel<h2 256x256>", items=big))
    c.append(_case("nt_grouped_h2 256-multiples nt2=0", "nt_grouped_h2", (256, 128), "gemm3_nt_group_kernel<h2>", items=big,
                   opts={"gemm3_nt2": 0}))
    c.append(_case("nt_grouped_h2 256x288", "nt_grouped_h2", (256, 128), "gemm3_nt_group_kernel<h2>", items=((256, 288),)))
    c.append(_case("wgrad 8x8 128->64", "wgrad", (1, 8, 8, 128, 64), "gemm3_nt_kernel<conv3x3>", rps=32))
    c.append(_case("wgrad_h2 8x8 128->64", "wgrad_h2", (1, 8, 8, 128, 64), "gemm3_nt_kernel<conv3x3 h2>", rps=32))
    c.append(_case("wgrad_h2 8x8 256->256", "wgrad_h2", (1, 8, 8, 256, 256), "gemm3_nt_kernel<conv3x3 h2 256x256>", rps=32))
    c.append(_case("wgrad_h2 8x8 256->256 nt2=0", "wgrad_h2", (1, 8, 8, 256, 256), "gemm3_nt_kernel<conv3x3 h2>", rps=32,
                   opts={"gemm3_nt2": 0}))
    c.append(_case("nt_bf16 100x36", "nt_bf16", (1000, 100, 36, 128), "gemm3_nt_kernel<128, bf16>"))
    ids = [x["id"] for x in c]
    assert len(set(ids)) == len(ids)
    return c


CASES = _cases()


def route_ok(case, kernel):
    """-> None, or why `kernel` is not the route the case is there for (valid where the device has the recorded CU count)"""
    exp, avoid = case["expect"], case["avoid"]
    if isinstance(exp, str) and exp.startswith("~"):
        if exp[1:] not in kernel:
            return f"expected a kernel with {exp[1:]!r}"
    elif exp is not None and kernel not in ((exp,) if isinstance(exp, str) else exp):
        return f"expected {exp!r}"
    if avoid is not None and avoid in kernel:
        return f"expected a kernel without {avoid!r}"
    return None


@contextlib.contextmanager
def options(opts):
    from mp_former_amd import _lib
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k in opts:
            _lib.set_option(k, DEFAULTS[k])


def _sha(t):
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


class _Inputs:
    """host draws of one case, in call order, moved to the device"""

    def __init__(self, cid, dev):
        self.rng = np.random.default_rng(zlib.crc32(cid.encode()))
        self.dev = dev

    def f32(self, *shape, scale=1.0):
        return torch.from_numpy(self.rng.standard_normal(shape, dtype=np.float32) * np.float32(scale)).to(self.dev)

    def bf16(self, *shape):
        return self.f32(*shape).to(torch.bfloat16)

    def u8(self, *shape):
        return torch.from_numpy(self.rng.integers(0, 256, shape, dtype=np.uint8)).to(self.dev)


def _h2_planes(w):
    from mp_former_amd.gemm3 import split_weights_grouped_h2
    (planes, slot), = split_weights_grouped_h2([([w], False)])
    return planes, slot


U = 2.0 ** -24      # unit roundoff of fp32


def _split_sums(x, rps, x2=None):
    """exact per-split column sums of x (+ x2[r % rows]) [ns, cols] in fp64, and the sums of the magnitudes"""
    R = x.shape[0]
    ns = (R + rps - 1) // rps
    v, mag = x.double(), x.double().abs()
    if x2 is not None:
        rows = torch.arange(R, device=x.device) % x2.shape[0]
        v, mag = v + x2.double()[rows], mag + x2.double().abs()[rows]
    pad = ns * rps - R
    if pad:
        z = torch.zeros((pad, x.shape[1]), dtype=torch.float64, device=x.device)
        v, mag = torch.cat((v, z)), torch.cat((mag, z))
    return v.view(ns, rps, -1).sum(1), mag.view(ns, rps, -1).sum(1)


def _sum_ratio(got, x, rps, x2=None):
    """worst |got - exact| / bound of per-split column sums [ns, cols]: a sum of n fp32 terms in ANY order is within
    (n - 1) u sum|x_i| of the exact one (first order); n + 2 covers the rounding of x + x2 and the second-order terms"""
    ref, mag = _split_sums(x, rps, x2)
    bound = (rps + 2) * U * mag + 1e-37
    return float(((got.double() - ref).abs() / bound).max())


_HASH_SUMS = False


def _sums(out, name, got, ratio):
    out.setdefault("sums", {})[name] = ratio
    if _HASH_SUMS:
        out.setdefault("sum_hashes", {})[name] = _sha(got)


def _amax_hashes(out, slot):
    if slot is not None:
        from mp_former_amd.gemm3 import amax_value
        out["out_amax"] = _sha(amax_value(slot).reshape(1))
        out["out_amax_slot"] = _sha(slot)


def _run_tn(case, x, log):
    from mp_former_amd import gemm3 as g
    M, N, K = case["shape"]
    opt = lambda k: bool(case.get(k))
    a = x.bf16(M, K) if opt("a16") else x.f32(M, K)
    w = x.f32(N, K, scale=K ** -0.5)
    bias = x.f32(N) if opt("bias") else None
    cin = x.f32(M, N) if opt("cin") else None
    cin2 = x.f32(M, N) if opt("cin2") else None
    gate = x.f32(M, N) if opt("gate") else None
    a2 = x.f32(7, K) if opt("a2") else None
    gbits = x.u8(M, N // 8) if opt("gate_bits") else None
    entry, out = case["entry"], {}
    if entry == "tn":
        planes = g.split_weight(w)
        with log:
            out["c"] = _sha(g.gemm3(a, planes, bias=bias, a2=a2, cin=cin, cin2=cin2, gate=gate, relu=opt("relu")))
    elif entry == "tn_ex":
        planes = g.split_weight(w)
        with log:
            out["c"] = _sha(g.gemm3_ex(a, planes, bias=bias, cin=cin, relu=opt("relu"),
                                       out_dtype=torch.bfloat16 if opt("c16") else torch.float32))
    else:
        planes, w_am = _h2_planes(w)
        a_am = g.amax(a)
        slot = g.amax_slots(1, a.device)[0] if opt("out_amax") else None
        with log:
            if entry == "tn_h2":
                c = g.gemm3_h2(a, a_am, planes, w_am, bias=bias, cin=cin, cin2=cin2, gate=gate, relu=opt("relu"), out_amax=slot)
            else:
                c = g.gemm3_h2_bits(a, a_am, planes, w_am, bias=bias, cin=cin, cin2=cin2, gate_bits=gbits, relu=opt("relu"),
                                    out_amax=slot, want_bits=opt("bits_out"))
                if opt("bits_out"):
                    c, bits = c
                    out["bits_out"] = _sha(bits)
        out["c"] = _sha(c)
        _amax_hashes(out, slot)
    return out


def _run_conv(case, x, log):
    from mp_former_amd import _lib, gemm3 as g
    n, H, W, Cin, Cout = case["shape"]
    dev = x.dev
    img = x.f32(n * H * W, Cin)
    w = x.f32(Cout, 9 * Cin, scale=(9 * Cin) ** -0.5)
    bias = x.f32(Cout) if case.get("bias") else None
    y = torch.zeros((n * H * W, Cout), dtype=torch.float32, device=dev)
    st, out = _lib.stream_ptr(dev), {}
    if case["entry"] == "conv":
        planes = g.split_weight(w)
        with log:
            _lib.call("mpf_gemm3_conv3x3", dev, img.data_ptr(), planes.data_ptr(), _lib.ptr(bias), y.data_ptr(), n, H, W, Cin, Cout,
                      case["transposed"], st)
    else:
        planes, w_am = _h2_planes(w)
        x_am = g.amax(img)
        slot = g.amax_slots(1, dev)[0] if case.get("out_amax") else None
        with log:
            _lib.call("mpf_gemm3_conv3x3_h2", dev, img.data_ptr(), x_am.data_ptr(), planes.data_ptr(), w_am.data_ptr(), _lib.ptr(bias),
                      y.data_ptr(), _lib.ptr(slot), n, H, W, Cin, Cout, case["transposed"], st)
        _amax_hashes(out, slot)
    out["c"] = _sha(y)
    return out


def _run_nt(case, x, log):
    from mp_former_amd import gemm3 as g
    R, M, N, rps = case["shape"]
    opt = lambda k: bool(case.get(k))
    a = x.bf16(R, M) if opt("a16") else x.f32(R, M)
    b = x.bf16(R, N) if opt("b16") else x.f32(R, N)
    out = {}
    if case["entry"] == "nt_ex":
        with log:
            c, ca = g.gemm3_nt_ex(a, b, rps, want_csum_a=opt("csum_a"))
        cb = None
    else:
        b2 = x.f32(7, N) if opt("b2") else None
        am = (g.amax(a), g.amax(b)) if case["entry"] == "nt_h2" else None
        with log:
            c, ca, cb = g.gemm3_nt(a, b, rps, b2=b2, want_csum_a=opt("csum_a"), want_csum_b=opt("csum_b"),
                                   transpose_out=opt("transpose_out"), amax_ab=am)
    out["c_part"] = _sha(c)
    if ca is not None:
        _sums(out, "csum_a", ca, _sum_ratio(ca, a, rps))
    if cb is not None:
        _sums(out, "csum_b", cb, _sum_ratio(cb, b, rps, b2 if case["entry"] != "nt_ex" else None))
    return out


def _run_grouped(case, x, log):
    from mp_former_amd import _lib, gemm3 as g
    R, rps = case["shape"]
    dev, h2 = x.dev, case["entry"] == "nt_grouped_h2"
    ns = (R + rps - 1) // rps
    pairs = [(x.f32(R, M), x.f32(R, N)) for M, N in case["items"]]
    keep = [(g.amax(a), g.amax(b)) for a, b in pairs] if h2 else None
    offs, tot = [], 0
    for M, N in case["items"]:
        offs.append(tot)
        tot += (M * N + M + 3) // 4 * 4
    part = torch.zeros((ns, tot), dtype=torch.float32, device=dev)
    items = np.empty((len(pairs), 10 if h2 else 8), dtype=np.int64)
    for i, ((a, b), o) in enumerate(zip(pairs, offs)):
        M, N = case["items"][i]
        dst = (part.data_ptr() + 4 * o, part.data_ptr() + 4 * (o + M * N), M, N)
        if h2:
            items[i] = (a.data_ptr(), a.stride(0), keep[i][0].data_ptr(), b.data_ptr(), b.stride(0), keep[i][1].data_ptr()) + dst
        else:
            items[i] = (a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0)) + dst
    with log:
        _lib.call("mpf_gemm3_nt_grouped_h2" if h2 else "mpf_gemm3_nt_grouped", dev, items.ctypes.data, len(pairs), R, rps, tot,
                  _lib.stream_ptr(dev))
    out = {}
    for i, ((a, b), o) in enumerate(zip(pairs, offs)):
        M, N = case["items"][i]
        out[f"c_part{i}"] = _sha(part[:, o:o + M * N])
        ca = part[:, o + M * N:o + M * N + M]
        _sums(out, f"csum_a{i}", ca, _sum_ratio(ca, a, rps))
    return out


def _run_wgrad(case, x, log):
    from mp_former_amd import _lib, gemm3 as g
    n, H, W, Cin, Cout = case["shape"]
    dev, rps = x.dev, case["rps"]
    R = n * H * W
    ns = (R + rps - 1) // rps
    dy, img = x.f32(R, Cout), x.f32(R, Cin)
    c = torch.zeros((ns, Cout, 9 * Cin), dtype=torch.float32, device=dev)
    ca = torch.zeros((ns, Cout), dtype=torch.float32, device=dev)
    st = _lib.stream_ptr(dev)
    if case["entry"] == "wgrad_h2":
        am = (g.amax(dy), g.amax(img))
        with log:
            _lib.call("mpf_gemm3_conv3x3_wgrad_h2", dev, dy.data_ptr(), am[0].data_ptr(), img.data_ptr(), am[1].data_ptr(), c.data_ptr(),
                      ca.data_ptr(), n, H, W, Cin, Cout, rps, st)
    else:
        with log:
            _lib.call("mpf_gemm3_conv3x3_wgrad", dev, dy.data_ptr(), img.data_ptr(), c.data_ptr(), ca.data_ptr(), n, H, W, Cin, Cout, rps, st)
    out = {"c_part": _sha(c)}
    _sums(out, "csum_a", ca, _sum_ratio(ca, dy, rps))
    return out


def _run_nt_bf16(case, x, log):
    from mp_former_amd import _lib
    R, M, N, rps = case["shape"]
    dev = x.dev
    a, b = x.bf16(R, M), x.bf16(R, N)
    nbytes = _lib.lib().mpf_gemm_nt_bf16_workspace_bytes(R, M, N, rps)
    ws = torch.zeros(nbytes // 4, dtype=torch.float32, device=dev)          # split partials, then the column sums
    c = torch.zeros((M, N), dtype=torch.bfloat16, device=dev)
    cs = torch.zeros((M,), dtype=torch.bfloat16, device=dev)
    with log:
        _lib.call("mpf_gemm_nt_bf16", dev, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), cs.data_ptr(), R, M, N, rps,
                  ws.data_ptr(), nbytes, _lib.stream_ptr(dev))
    ns = (R + rps - 1) // rps
    part = ws[:ns * M * N]
    ca = ws[ns * M * N:ns * (M * N + M)].view(ns, M)
    out = {"c": _sha(c), "partials": _sha(part)}
    _sums(out, "csum_partials", ca, _sum_ratio(ca, a, rps))
    # the reduced sums: an fp32 sum of R terms, rounded to nearest bf16 (8 significant bits: unit roundoff 2^-8)
    ref, mag = _split_sums(a, ns * rps)
    e32 = (R + 2) * U * mag
    bound = e32 + 2.0 ** -8 * (ref.abs() + e32) + 1e-37
    _sums(out, "csum", cs, float(((cs.double() - ref[0]).abs() / bound[0]).max()))
    return out


_RUN = {"tn": _run_tn, "tn_ex": _run_tn, "tn_h2": _run_tn, "tn_h2_bits": _run_tn, "conv": _run_conv, "conv_h2": _run_conv,
        "nt": _run_nt, "nt_h2": _run_nt, "nt_ex": _run_nt, "nt_grouped": _run_grouped, "nt_grouped_h2": _run_grouped,
        "wgrad": _run_wgrad, "wgrad_h2": _run_wgrad, "nt_bf16": _run_nt_bf16}


class _Log:
    """launch log around the entry point under test only: kernel name, records, bytes, flops"""

    def __enter__(self):
        from mp_former_amd import _lib
        _lib.profile_enable(True)
        return self

    def __exit__(self, *exc):
        from mp_former_amd import _lib
        try:
            if exc[0] is None:
                self.kernel = _lib.last_kernel()
                torch.cuda.synchronize()
                self.records, _, self.bytes = _lib.profile_get("")
                self.flops = _lib.profile_get_flops("")
        finally:
            _lib.profile_enable(False)
        return False


def run_case(case, dev):
    """-> {"kernel", "records", "bytes", "flops", "hashes": {buffer: sha256}, "sums": {buffer: |got - exact| / bound}}; every
    option the case sets is restored"""
    log = _Log()
    with options(case["opts"]):
        hashes = _RUN[case["entry"]](case, _Inputs(case["id"], dev), log)
    r = {"kernel": log.kernel, "records": log.records, "bytes": log.bytes, "flops": log.flops, "sums": hashes.pop("sums", {})}
    if "sum_hashes" in hashes:
        r["sum_hashes"] = hashes.pop("sum_hashes")
    r["hashes"] = hashes
    return r


def cu_count(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    ap.add_argument("--hash-sums", action="store_true", help="also hash the column sums (run twice and compare: they are not reproducible)")
    args = ap.parse_args()
    global _HASH_SUMS
    _HASH_SUMS = args.hash_sums
    dev = torch.device("cuda:0")
    from mp_former_amd import _lib
    out = {"cu_count": cu_count(dev), "device": torch.cuda.get_device_name(dev), "cases": {}}
    wrong = []
    for case in CASES:
        r = run_case(case, dev)
        why = route_ok(case, r["kernel"])
        print(f"{case['id']:<50} {r['kernel']:<40} bytes {r['bytes']:.0f} flops {r['flops']:.0f}" + (f"   WRONG ROUTE: {why}" if why else ""),
              flush=True)
        if why:
            wrong.append(f"{case['id']}: got {r['kernel']}, {why}")
        off = {k: v for k, v in r["sums"].items() if not v <= 1.0}
        if off:
            wrong.append(f"{case['id']}: column sums outside the rounding of an fp32 sum (|got - exact| / bound): {off}")
        r["sums"] = sorted(r["sums"])            # (the ratios vary from run to run: the fixture keeps the names)
        out["cases"][case["id"]] = r
    print(f"library {_lib.LIB_PATH}; {len(CASES)} cases, {out['cu_count']} CUs")
    if wrong:
        raise SystemExit("cases that miss the route they are there for (fix the SHAPE, not the expectation) or the sums:\n  " + "\n  ".join(wrong))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
