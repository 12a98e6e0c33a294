"""The problems, fp64 references, bounds, geometry mirrors and single-fault emulation of the GroupNorm kernels
(csrc/groupnorm_cl.hip: mpf_gn_cl_forward, mpf_gn_cl_backward, mpf_upsample2x_cl_backward; csrc/elementwise.hip: mpf_group_stats).
No GPU and no library is needed to import this file.  tests/test_groupnorm_cases_cpu.py holds the case tables to the branches they
name, the mirrors to the built library, aten's own fp32 GroupNorm to the bounds at half their width, and every fault of the
emulation to a failing check; tests/test_groupnorm_routes_gpu.py runs the same problems through the C ABI, the autograd wrappers
and the module, and the same check functions.

Buffers: an image is a dense [H*W, C] plane at ``n * batch_stride``; where a case has gaps the stride of every tensor (x, top, gy,
y, dx, dtop) exceeds the plane by another amount.  Input gaps are NaN, every output buffer starts as SENT everywhere; after a call
the gaps must hold SENT bit for bit, every addressed element must be finite and differ from SENT.

References are fp64 on the fp32 values: F.group_norm, F.relu, F.interpolate(bilinear, align_corners=False), autograd for every
gradient, the group mean and 1 / sqrt(var + eps) directly.  With u = 2^-24, a = rstd * gamma, m = (C/G) * H * W, sigma = sqrt(var),
xt = (|x| + |mu|) * rstd, sums over the group and K = 8, every element is held to
    y      K u (|a| (|x| + |mu|) + |beta| + up(|top|))
    mean   K u (|mu| + sigma)
    rstd   K u rstd (1 + |mu| / sigma)         [tightened from (|mu| / sigma)^2: see RSTD FORM below]
    dx     K u (|a| |gy| + rstd sum|gamma gy| / m + xt rstd sum(|gamma gy| xt) / m)
    dgamma K u sum(|gy| xt)      dbeta  K u sum|gy|      dtop  K u adj(|gy|)
K: aten's fp32 group_norm on the CPU stays inside these forms at K = 4 on every case (tests/test_groupnorm_cases_cpu.py has the
figures); K = 8 is twice that.  The two quantities that pass through the bilinear taps, y of the ``top`` mode and dtop, are the
exception: aten is at 4.7 and 4.5 there and is held to K = 8 itself.  At large mean the dx form undoes the cancellation the kernel
has, so the rows of the two large-mean distributions also require max|dx - ref| <= 4 * max|dx_aten - ref| with aten's fp32 backward
on the same device and input (the 4 is for another summation order).

RSTD FORM.  The issue's form K u rstd (1 + (|mu| / sigma)^2) is what a one-pass E[x^2] - mean^2 in fp32 needs; chunked two-pass
moments merged with Chan's formula lose |mu| / sigma only to first order (a chunk mean rounded by u |mu| moves the merged M2 by
2 n d u |mu| with d ~ sigma / sqrt(chunk); the second-order term n (u mu)^2 is negligible).  Against the first-order form at K = 8
the emulation is at most at 0.26 and aten's fp32 moments at 0.15 over all cases, both below 0.01 at |mu| / sigma = 133 and 6000,
so that is the form kept.  The squared form lets fault 4 (variance as E[x^2] - mean^2) through the rstd check: the fault is at 0.3
of it at 40 + 0.3 randn and 0.9 at 300 + 0.05 randn, against 40 and 5000 of the first-order form
(test_the_squared_rstd_form_would_not_see_a_one_pass_variance).

ReLU kink: elements whose fp64 pre-activation is below 1e-4 in magnitude get a zero upstream gradient (fp32 and fp64 may disagree
on the gate there); at most 0.1 % of a case's elements may be such.  The 300 + 0.05 randn rows have no ``relu`` mode: there
|a| (|x| + |mu|) is 12000, the y form itself allows 5e-3, and an fp32 y = x a + (beta - mu a), aten's as much as the kernels',
cannot decide the gate within 1e-4 of zero (the emulation's dbeta is off by 5 at (32, 8, 90x92): whole gy values of flipped gates)."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

F64, F32 = torch.float64, torch.float32
U = 2.0 ** -24
K = 8.0
EPS = 1e-5
KINK, KINK_CAP = 1e-4, 1e-3
ATEN_FACTOR = 4.0
SENT = -3.0e19
NAN = float("nan")
GUARD = 8                                     # sentinel elements behind mean, rstd, dgamma, dbeta

# ---- geometry mirrors (make_plane, fwd_ws, bwd_ws of csrc/groupnorm_cl.hip; the chunk count of mpf_group_stats) --------------------
KT, STAT_PIX, APPLY_PIX, KSUB, RED_SLICES, MERGE_LANES = 256, 128, 64, 8, 32, 64
GS_CHUNK = 256 * 32


def make_plane(HW, C, G):
    """-> the kernels' Plane, or None where make_plane refuses"""
    if HW <= 0 or C <= 0 or G <= 0 or C % G or C % 4 or C > 1024:
        return None
    cpg, tpc = C // G, C // 4
    if cpg % 4 or KT % tpc or G > KT or C % 32 or cpg > 32 or cpg & (cpg - 1):
        return None
    return SimpleNamespace(HW=HW, C=C, G=G, cpg=cpg, tpc=tpc, pr=KT // tpc, chunks=(HW + STAT_PIX - 1) // STAT_PIX, tail=HW % STAT_PIX)


def fwd_ws(N, P):
    return N * P.G * P.chunks * 3 * 4


def bwd_ws(N, P):
    return (N * P.chunks * 2 * P.C + N * 5 * P.C) * 4


def cl_workspace_bytes(N, HW, C, G):
    P = make_plane(HW, C, G)
    return 0 if N <= 0 or P is None else max(fwd_ws(N, P), bwd_ws(N, P))


def group_stats_chunks(row_len):
    return (row_len + GS_CHUNK - 1) // GS_CHUNK


def group_stats_workspace_bytes(rows, row_len):
    return 0 if rows <= 0 or row_len <= 0 else rows * group_stats_chunks(row_len) * 3 * 4


# ---- case tables ----------------------------------------------------------------------------------------------------------------------
# name -> N, C, G, (H, W), modes, distribution, gaps, and the branches the row is there for: pixel rows per workgroup, C / G, 128-pixel
# chunks, pixels of the last chunk (0: full), and optionally ``hw_lt_pr`` (threads without a pixel enter the Chan merge), ``top``
# ("wide": top map one pixel high, "high": one pixel wide, "1x1", "rect")
def _row(N, C, G, hw, modes, tags, dist="std", gaps=False):
    return dict(N=N, C=C, G=G, hw=hw, modes=tuple(modes), dist=dist, gaps=gaps, tags=tags)


PR, PRT = ("plain", "relu"), ("plain", "relu", "top")
CL_CASES = {
    "c32g8_1x3": _row(2, 32, 8, (1, 3), PR, dict(pr=32, cpg=4, chunks=1, tail=3, hw_lt_pr=True)),
    "c32g1_3x5": _row(2, 32, 1, (3, 5), PR, dict(pr=32, cpg=32, chunks=1, tail=15, hw_lt_pr=True)),
    "c32g2_82x100": _row(2, 32, 2, (82, 100), PRT, dict(pr=32, cpg=16, chunks=65, tail=8)),
    "c32g4_128x130": _row(2, 32, 4, (128, 130), PRT, dict(pr=32, cpg=8, chunks=130, tail=0)),
    "c64g16_50x82": _row(2, 64, 16, (50, 82), PRT, dict(pr=16, cpg=4, chunks=33, tail=4), gaps=True),
    "c64g2_8x16": _row(1, 64, 2, (8, 16), PRT, dict(pr=16, cpg=32, chunks=1, tail=0)),
    "c64g2_43x3": _row(2, 64, 2, (43, 3), PR, dict(pr=16, cpg=32, chunks=2, tail=1)),
    "c128g8_34x18": _row(2, 128, 8, (34, 18), ("top",), dict(pr=8, cpg=16, chunks=5, tail=100, top="rect")),
    "c256g32_82x100": _row(2, 256, 32, (82, 100), PRT, dict(pr=4, cpg=8, chunks=65, tail=8), gaps=True),
    "c256g8_9x5": _row(3, 256, 8, (9, 5), PR, dict(pr=4, cpg=32, chunks=1, tail=45)),
    "c256g64_9x5": _row(3, 256, 64, (9, 5), PR, dict(pr=4, cpg=4, chunks=1, tail=45), gaps=True),
    "c512g32_13x10": _row(2, 512, 32, (13, 10), PR, dict(pr=2, cpg=16, chunks=2, tail=2)),
    "c1024g32_9x5": _row(2, 1024, 32, (9, 5), PR, dict(pr=1, cpg=32, chunks=1, tail=45)),
    "c1024g256_9x5": _row(2, 1024, 256, (9, 5), PR, dict(pr=1, cpg=4, chunks=1, tail=45)),
    "c1024g32_19x7": _row(2, 1024, 32, (19, 7), PR, dict(pr=1, cpg=32, chunks=2, tail=5)),
    "c1024g256_19x7": _row(2, 1024, 256, (19, 7), PR, dict(pr=1, cpg=4, chunks=2, tail=5), gaps=True),
    "c256g32_top_2x6": _row(2, 256, 32, (2, 6), ("top",), dict(pr=4, cpg=8, chunks=1, tail=12, top="wide"), gaps=True),
    "c256g32_top_6x2": _row(2, 256, 32, (6, 2), ("top",), dict(pr=4, cpg=8, chunks=1, tail=12, top="high")),
    "c256g32_top_2x2": _row(2, 256, 32, (2, 2), ("top",), dict(pr=4, cpg=8, chunks=1, tail=4, top="1x1")),
    "c256g32_top_4x10": _row(2, 256, 32, (4, 10), ("top",), dict(pr=4, cpg=8, chunks=1, tail=40, top="rect")),
    "c32g8_90x92_m40": _row(2, 32, 8, (90, 92), PRT, dict(pr=32, cpg=4, chunks=65, tail=88), dist="m40"),
    "c32g8_90x92_m300": _row(2, 32, 8, (90, 92), ("plain",), dict(pr=32, cpg=4, chunks=65, tail=88), dist="m300"),
    "c256g32_34x18_m40": _row(2, 256, 32, (34, 18), PR, dict(pr=4, cpg=8, chunks=5, tail=100), dist="m40"),
    "c256g32_34x18_m300": _row(2, 256, 32, (34, 18), ("plain", "top"), dict(pr=4, cpg=8, chunks=5, tail=100), dist="m300", gaps=True),
    "c128g8_6x10_gaps": _row(3, 128, 8, (6, 10), PRT, dict(pr=8, cpg=16, chunks=1, tail=60, top="rect"), gaps=True),
}
CL_RUNS = [(name, mode) for name, row in CL_CASES.items() for mode in row["modes"]]
LARGE_MEAN = {"m40": (40.0, 0.3), "m300": (300.0, 0.05)}
# batch stride minus plane, per tensor, of a case with gaps (multiples of 4, all different)
GAPS = dict(x=64, top=36, gy=128, y=12, dx=260, dtop=4)
FLATTEN_LEVELS = ((8, 16), (43, 3), (82, 100))          # group_norm_flatten: C = 32, G = 8, N = 2

# name -> rows, row length, distribution: mpf_group_stats called directly
NCHW_CASES = {
    "3x4": (3, 4, "std"), "2x1020": (2, 1020, "std"), "64x1024": (64, 1024, "std"), "5x8188": (5, 8188, "std"), "5x8192": (5, 8192, "std"),
    "5x8196": (5, 8196, "std"), "2x16388": (2, 16388, "std"), "3x24588": (3, 3 * 8192 + 12, "std"), "2x8196_m40": (2, 8196, "m40"),
    "2x8196_m300": (2, 8196, "m300"),
}
# _GroupNormFn on contiguous NCHW input: name -> (N, C, H, W), G; rows x row length as the table entry of the same size
NCHW_MODULE_CASES = {"2x1020": ((1, 8, 15, 17), 2), "5x8196": ((1, 20, 3, 683), 5)}
# GroupNorm.forward on shapes the channel-last kernels refuse: (shape, G, what takes it)
FALLBACK_CASES = [((2, 96, 6, 10), 32, "gn_chunk_stats_kernel"), ((2, 256, 6, 10), 4, "gn_chunk_stats_kernel"), ((2, 64, 3, 3), 32, None)]


def _seed(name, mode=""):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name + "/" + mode)) % (2 ** 31)


def _draw(dist, shape, g, N=None, C=None, G=None):
    """std: a per-(image, group) mean of magnitude 1 .. 2 and either sign, a per-(image, channel) offset 0.25 randn and a
    per-(image, group) spread in 0.5 .. 2, so that the statistics of neighbouring groups and images differ.  The group mean stays
    away from 0 on purpose: the y form has no sigma term, so it does not cover the share a sigma u of the mean's own rounding at
    a pixel with |x| + |mu| << sigma (aten's fp32 moments on the CPU were at 20 u there).  m40 / m300: the two large-mean
    distributions"""
    if dist in LARGE_MEAN:
        mu, sd = LARGE_MEAN[dist]
        return mu + sd * torch.randn(shape, generator=g)
    v = torch.randn(shape, generator=g)
    if N is None:
        return 0.5 + 2.0 * v
    per_g = lambda t: t.expand(N, 1, G, C // G).reshape(N, 1, C)                               # noqa: E731
    off = per_g((1.0 + torch.rand(N, 1, G, 1, generator=g)) * torch.where(torch.rand(N, 1, G, 1, generator=g) < 0.5, -1.0, 1.0))
    off = off + 0.25 * torch.randn(N, 1, C, generator=g)
    return off + per_g(0.5 + 1.5 * torch.rand(N, 1, G, 1, generator=g)) * v


def pack(vals, gap, fill=NAN):
    """[N, ...] values -> flat buffer of N images at stride plane + gap, the gaps (one behind every image) ``fill``"""
    N = vals.shape[0]
    v = vals.reshape(N, -1)
    buf = torch.full((N, v.shape[1] + gap), fill, dtype=F32)
    buf[:, :v.shape[1]] = v
    return buf.reshape(-1)


def cl_problem(name, mode, hw=None, C=None, G=None, N=None, gaps=None):
    """-> namespace of CPU tensors; values are [N, H*W, C] (``x``, ``gy``, ``top`` [N, Ht*Wt, C]), ``*_buf`` the strided buffers"""
    row = CL_CASES.get(name, {})
    N, C, G = N or row["N"], C or row["C"], G or row["G"]
    H, W = hw or row["hw"]
    gaps = row.get("gaps", False) if gaps is None else gaps
    dist = row.get("dist", "std")
    g = torch.Generator().manual_seed(_seed(name, mode))
    HW = H * W
    pb = SimpleNamespace(name=name, mode=mode, N=N, C=C, G=G, H=H, W=W, HW=HW, cpg=C // G, relu=mode == "relu", has_top=mode == "top",
                         dist=dist, gaps=gaps, eps=EPS, plane=HW * C, Ht=H // 2, Wt=W // 2)
    pb.gap = {k: (v if gaps else 0) for k, v in GAPS.items()}
    pb.bs = {k: pb.plane + pb.gap[k] for k in ("x", "gy", "y", "dx")}
    pb.tplane = pb.Ht * pb.Wt * C
    pb.bs.update(top=pb.tplane + pb.gap["top"], dtop=pb.tplane + pb.gap["dtop"])
    pb.x = _draw(dist, (N, HW, C), g, N, C, G)
    pb.gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    pb.beta = torch.randn(C, generator=g)
    pb.gy = torch.randn(N, HW, C, generator=g)
    pb.top = torch.randn(N, pb.Ht * pb.Wt, C, generator=g) if pb.has_top else None
    assert not pb.has_top or (H % 2 == 0 and W % 2 == 0)
    pb.kink_share = 0.0
    if pb.relu:
        pre = F.group_norm(_nchw(pb.x.to(F64), pb), G, pb.gamma.to(F64), pb.beta.to(F64), EPS)
        kink = _cl(pre.abs() < KINK)
        pb.gy = torch.where(kink, torch.zeros(()), pb.gy)
        pb.kink_share = float(kink.float().mean())
    pb.x_buf, pb.gy_buf = pack(pb.x, pb.gap["x"]), pack(pb.gy, pb.gap["gy"])
    pb.top_buf = pack(pb.top, pb.gap["top"]) if pb.has_top else None
    return pb


def _nchw(v, pb, H=None, W=None):
    """[N, H*W, C] -> [N, C, H, W] view"""
    return v.view(pb.N, H or pb.H, W or pb.W, pb.C).permute(0, 3, 1, 2)


def _cl(v):
    """[N, C, H, W] -> [N, H*W, C]"""
    return v.permute(0, 2, 3, 1).reshape(v.shape[0], -1, v.shape[1])


def _group_sum(v, pb):
    """[N, HW, C] -> sum over the pixels and channels of every group, broadcast back to [N, 1, C]"""
    s = v.view(pb.N, pb.HW, pb.G, pb.cpg).sum((1, 3), keepdim=True)
    return s.expand(pb.N, 1, pb.G, pb.cpg).reshape(pb.N, 1, pb.C)


def cl_reference(pb):
    """-> namespace: fp64 y, mean, rstd, dx, dgamma, dbeta, dtop in the layouts of the problem and the bound of each at K = 1
    (``b_<name>``)"""
    N, C, G, HW = pb.N, pb.C, pb.G, pb.HW
    x = _nchw(pb.x.to(F64), pb).clone().requires_grad_(True)
    gm, bt = pb.gamma.to(F64).requires_grad_(True), pb.beta.to(F64).requires_grad_(True)
    pre = F.group_norm(x, G, gm, bt, pb.eps)
    y = F.relu(pre) if pb.relu else pre
    leaves = [x, gm, bt]
    if pb.has_top:
        top = _nchw(pb.top.to(F64), pb, pb.Ht, pb.Wt).clone().requires_grad_(True)
        y = y + F.interpolate(top, size=(pb.H, pb.W), mode="bilinear", align_corners=False)
        leaves.append(top)
    gy = pb.gy.to(F64)
    grads = torch.autograd.grad(y, leaves, _nchw(gy, pb))
    r = SimpleNamespace(y=_cl(y.detach()), dx=_cl(grads[0]), dgamma=grads[1], dbeta=grads[2], dtop=_cl(grads[3]) if pb.has_top else None)
    xg = pb.x.to(F64).view(N, HW, G, pb.cpg)
    r.mean = xg.mean((1, 3))
    var = ((xg - r.mean[:, None, :, None]) ** 2).mean((1, 3))
    r.rstd = 1.0 / torch.sqrt(var + pb.eps)
    sigma = torch.sqrt(var)
    r.b_mean = U * (r.mean.abs() + sigma)
    r.b_rstd = U * r.rstd * (1.0 + r.mean.abs() / sigma)
    r.b_rstd_squared = U * r.rstd * (1.0 + (r.mean.abs() / sigma) ** 2)
    per_c = lambda s: s[:, None, :, None].expand(N, 1, G, pb.cpg).reshape(N, 1, C)           # noqa: E731
    mu, rs = per_c(r.mean), per_c(r.rstd)
    xa = pb.x.to(F64).abs() + mu.abs()
    a = rs * pb.gamma.to(F64).abs()
    r.b_y = U * (a * xa + pb.beta.to(F64).abs())
    if pb.has_top:
        up = F.interpolate(_nchw(pb.top.to(F64).abs(), pb, pb.Ht, pb.Wt), size=(pb.H, pb.W), mode="bilinear", align_corners=False)
        r.b_y = r.b_y + U * _cl(up)
        t0 = torch.zeros(N, C, pb.Ht, pb.Wt, dtype=F64, requires_grad=True)
        upz = F.interpolate(t0, size=(pb.H, pb.W), mode="bilinear", align_corners=False)
        r.b_dtop = U * _cl(torch.autograd.grad(upz, t0, _nchw(gy.abs(), pb))[0]) + 1e-30
    gate = _cl(pre.detach() > 0).to(F64) if pb.relu else 1.0
    ga = gy.abs() * gate                                       # the gradient that reaches the norm
    xt = xa * rs
    m = pb.cpg * HW
    r.b_dx = U * (a * ga + rs * _group_sum(pb.gamma.to(F64).abs() * ga, pb) / m
                  + xt * rs * _group_sum(pb.gamma.to(F64).abs() * ga * xt, pb) / m) + 1e-30
    r.b_dgamma = U * (ga * xt).sum((0, 1)) + 1e-30
    r.b_dbeta = U * ga.sum((0, 1)) + 1e-30
    return r


# ---- checks ----------------------------------------------------------------------------------------------------------------------------
def hold(case, what, got, ref, bound, k=K):
    """print the worst error of this comparison, then assert |got - ref| <= k * bound for every element -> worst err / (k * bound)"""
    got = got.detach().to(F64).cpu()
    assert got.shape == ref.shape, (case, what, got.shape, ref.shape)
    err = (got - ref).abs()
    frac = err / (k * bound)
    bad = int((~(frac <= 1.0)).sum())
    print(f"[groupnorm] {case} | {what} | max abs err {float(err.max()):.3e} | worst err/bound {float(frac.max()):.3e} | "
          f"{bad} of {frac.numel()} outside")
    assert bool(torch.isfinite(got).all()) and bad == 0, (case, what, float(err.max()), float(frac.max()), bad)
    return float(frac.max())


def _bits(t):
    return t.contiguous().view(torch.int32)


def sentinel(n):
    return torch.full((int(n),), SENT, dtype=F32)


def take(case, what, buf, N, plane, bs):
    """a strided output buffer that started as SENT -> its [N, plane] values, after asserting that the gaps still hold SENT bit for
    bit and that every addressed element is finite and was written"""
    buf = buf.detach().cpu().reshape(-1)
    assert buf.numel() == N * bs, (case, what, buf.numel(), N, bs)
    v = buf.view(N, bs)
    sent = int(_bits(sentinel(1)))
    assert bool((_bits(v[:, plane:]) == sent).all()), f"{case}: a gap between the images of {what} was written"
    vals = v[:, :plane]
    assert bool(torch.isfinite(vals).all()), f"{case}: {what} is not finite (a gap was read, or worse)"
    assert bool((_bits(vals) != sent).all()), f"{case}: an addressed element of {what} was not written"
    return vals


def take_all(pb, bufs):
    """the buffers of one forward + backward (y, mean, rstd, dx, dgamma, dbeta, dtop; flat, SENT-prefilled, the small ones with
    GUARD extra elements) -> result namespace in the layouts of the reference"""
    case = f"{pb.name}/{pb.mode}"
    N, HW, C = pb.N, pb.HW, pb.C
    r = SimpleNamespace(dtop=None)
    r.y = take(case, "y", bufs["y"], N, pb.plane, pb.bs["y"]).view(N, HW, C)
    r.dx = take(case, "dx", bufs["dx"], N, pb.plane, pb.bs["dx"]).view(N, HW, C)
    r.mean = take(case, "mean", bufs["mean"], 1, N * pb.G, N * pb.G + GUARD).view(N, pb.G)
    r.rstd = take(case, "rstd", bufs["rstd"], 1, N * pb.G, N * pb.G + GUARD).view(N, pb.G)
    r.dgamma = take(case, "dgamma", bufs["dgamma"], 1, C, C + GUARD).view(C)
    r.dbeta = take(case, "dbeta", bufs["dbeta"], 1, C, C + GUARD).view(C)
    if pb.has_top:
        r.dtop = take(case, "dtop", bufs["dtop"], N, pb.tplane, pb.bs["dtop"]).view(N, pb.Ht * pb.Wt, C)
    return r


def new_buffers(pb):
    b = {k: sentinel(pb.N * pb.bs[k]) for k in ("y", "dx")}
    b.update(mean=sentinel(pb.N * pb.G + GUARD), rstd=sentinel(pb.N * pb.G + GUARD), dgamma=sentinel(pb.C + GUARD), dbeta=sentinel(pb.C + GUARD))
    if pb.has_top:
        b["dtop"] = sentinel(pb.N * pb.bs["dtop"])
    return b


QUANTITIES = ("y", "mean", "rstd", "dx", "dgamma", "dbeta", "dtop")


def check_all(pb, ref, res, k=K, route="", only=QUANTITIES):
    """every quantity of ``res`` that is present against the reference -> {quantity: worst err / bound}"""
    case = f"{pb.name}/{pb.mode} {route}".strip()
    out = {}
    for q in only:
        got = getattr(res, q, None)
        if got is not None:
            out[q] = hold(case, q, got, getattr(ref, q), getattr(ref, "b_" + q), k)
    return out


def check_vs_aten(pb, ref, dx, dx_aten, route=""):
    """large-mean cases: max|dx - ref| <= 4 * max|dx_aten - ref| -> the ratio"""
    e = float((dx.detach().to(F64).cpu() - ref.dx).abs().max())
    ea = float((dx_aten.detach().to(F64).cpu() - ref.dx).abs().max())
    print(f"[groupnorm] {pb.name}/{pb.mode} {route} | dx against aten fp32 | max abs err {e:.3e} | aten {ea:.3e} | ratio {e / ea:.3e}")
    assert e <= ATEN_FACTOR * ea, (pb.name, pb.mode, e, ea)
    return e / ea


def aten_results(pb, device="cpu"):
    """aten's own fp32 GroupNorm (+ ReLU / + bilinear upsampling) and autograd on ``device`` -> result namespace"""
    x = _nchw(pb.x, pb).contiguous().to(device).requires_grad_(True)
    gm, bt = pb.gamma.to(device).requires_grad_(True), pb.beta.to(device).requires_grad_(True)
    pre, mean, rstd = torch.native_group_norm(x, gm, bt, pb.N, pb.C, pb.HW, pb.G, pb.eps)
    y = F.relu(pre) if pb.relu else pre
    leaves = [x, gm, bt]
    if pb.has_top:
        top = _nchw(pb.top, pb, pb.Ht, pb.Wt).contiguous().to(device).requires_grad_(True)
        y = y + F.interpolate(top, size=(pb.H, pb.W), mode="bilinear", align_corners=False)
        leaves.append(top)
    grads = torch.autograd.grad(y, leaves, _nchw(pb.gy, pb).contiguous().to(device))
    return SimpleNamespace(y=_cl(y.detach()), mean=mean.detach().view(pb.N, pb.G), rstd=rstd.detach().view(pb.N, pb.G), dx=_cl(grads[0]),
                           dgamma=grads[1], dbeta=grads[2], dtop=_cl(grads[3]) if pb.has_top else None)


# ---- NCHW route: mpf_group_stats ---------------------------------------------------------------------------------------------------------
NCHW_PAD = 64                                  # NaN elements in front of the first row and behind the last


def nchw_problem(name):
    rows, row_len, dist = NCHW_CASES[name]
    g = torch.Generator().manual_seed(_seed(name, "nchw"))
    x = _draw(dist, (rows, row_len), g)
    if dist == "std":
        x = x * (0.5 + 2.0 * torch.rand(rows, 1, generator=g)) + torch.randn(rows, 1, generator=g)
    buf = torch.full((rows * row_len + 2 * NCHW_PAD,), NAN, dtype=F32)
    buf[NCHW_PAD:NCHW_PAD + rows * row_len] = x.reshape(-1)
    return SimpleNamespace(name=name, rows=rows, row_len=row_len, x=x, buf=buf, eps=EPS)


def stats_reference(x, eps):
    """rows of fp32 values -> fp64 mean, rstd and their bounds at K = 1"""
    x = x.to(F64)
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd, sigma = 1.0 / torch.sqrt(var + eps), torch.sqrt(var)
    return SimpleNamespace(mean=mean, rstd=rstd, b_mean=U * (mean.abs() + sigma), b_rstd=U * rstd * (1.0 + mean.abs() / sigma))


def check_stats(np_, mean_buf, rstd_buf, k=K, route="mpf_group_stats"):
    ref = stats_reference(np_.x, np_.eps)
    case = f"nchw {np_.name} {route}"
    out = {}
    for q, buf in (("mean", mean_buf), ("rstd", rstd_buf)):
        got = take(case, q, buf, 1, np_.rows, np_.rows + GUARD).view(-1)
        out[q] = hold(case, q, got, getattr(ref, q), getattr(ref, "b_" + q), k)
    return out


def module_problem(shape, G, seed_name, dist="std"):
    """contiguous NCHW problem of the _GroupNormFn route and of the fallback chain, as a channel-last problem namespace (the
    reference and the checks are the same)"""
    N, C, H, W = shape
    return cl_problem(seed_name, "plain", hw=(H, W), C=C, G=G, N=N, gaps=False)


# ---- torch emulation of the channel-last algorithm, one fault at a time ---------------------------------------------------------------
FAULTS = ("merge_trip", "reduce_trip", "tail_count", "naive_var", "quad_group", "image0", "relu_stats_gate", "i1_clamp", "border_weight",
          "top_hw_swap", "batch_stride", "d_mu", "eps_outside", "sub_div8")
# the (case, mode) every fault is held to (tests/test_groupnorm_cases_cpu.py)
FAULT_CASE = {
    "merge_trip": [("c32g2_82x100", "plain"), ("c256g32_82x100", "plain")],      # 1 the merge drops chunks >= 64
    "reduce_trip": [("c64g16_50x82", "plain"), ("c32g2_82x100", "relu")],        # 2 the bwd reduce drops chunks >= 32
    "tail_count": [("c64g2_43x3", "plain"), ("c32g8_1x3", "plain")],             # 3 a partial chunk is counted as 128 pixels
    "naive_var": [("c32g8_90x92_m40", "plain"), ("c256g32_34x18_m300", "plain")],  # 4 variance as E[x^2] - mean^2 in fp32
    "quad_group": [("c256g8_9x5", "plain"), ("c512g32_13x10", "relu")],          # 5 last channel quad takes the next group's statistics
    "image0": [("c256g64_9x5", "plain"), ("c128g8_6x10_gaps", "top")],           # 6 dgamma / dbeta take image 0 only
    "relu_stats_gate": [("c256g8_9x5", "relu"), ("c64g2_8x16", "relu")],         # 7 ReLU gate in the apply pass, not in the statistics pass
    "i1_clamp": [("c256g32_top_2x6", "top"), ("c256g32_top_6x2", "top")],        # 8 i1 not clamped at the last row / column of top
    "border_weight": [("c256g32_top_2x6", "top"), ("c256g32_top_2x2", "top")],   # 9 adjoint border weight 0.75 instead of 1
    "top_hw_swap": [("c256g32_top_2x6", "top"), ("c256g32_top_4x10", "top")],    # 10 H and W of top swapped
    "batch_stride": [("c128g8_6x10_gaps", "plain"), ("c128g8_6x10_gaps", "relu"), ("c128g8_6x10_gaps", "top")],   # 11 stride taken as H W C
    "d_mu": [("c256g64_9x5", "plain"), ("c256g32_34x18_m40", "plain")],          # 12 D is missing -B mu
    "eps_outside": [("c256g8_9x5", "plain"), ("c64g2_8x16", "plain")],           # 13 eps added outside the square root
    "sub_div8": [("c1024g32_19x7", "plain"), ("c512g32_13x10", "plain"), ("c32g8_1x3", "plain")],   # 14 short register block divided by 8
}


def _chan32(n, mu, m2, nb, mb, qb):
    """chan_merge of the statistics kernel, element-wise in fp32 (a block without pixels is skipped)"""
    skip = nb == 0
    nn = torch.where(skip, torch.ones_like(n), n + nb)
    d = mb - mu
    mu2 = mu + d * (nb / nn)
    m22 = m2 + qb + d * d * (n * nb / nn)
    return torch.where(skip, n, n + nb), torch.where(skip, mu, mu2), torch.where(skip, m2, m22)


def _chunk_pixels(HW, chunks, L):
    q = torch.arange(L)
    pix = torch.arange(chunks)[:, None] * STAT_PIX + q[None, :]
    return pix, (q[None, :] < STAT_PIX) & (pix < HW)


def _emu_chunk_stats(x, P, fault):
    """x [HW, C] fp32 -> (count, mean, M2) [chunks, G] fp32: register blocks of KSUB pixels per thread, Chan merges per thread,
    then over the threads of a group"""
    L = max(STAT_PIX, P.pr * KSUB)
    pix, valid = _chunk_pixels(P.HW, P.chunks, L)
    its = L // (P.pr * KSUB)
    v = torch.where(valid[:, :, None], x[pix.clamp(max=P.HW - 1)], torch.zeros(())).view(P.chunks, its, KSUB, P.pr, P.tpc, 4)
    ok = valid.view(P.chunks, its, KSUB, P.pr)
    cnt = ok.sum(2).to(F32)[..., None].expand(P.chunks, its, P.pr, P.tpc)
    s = v.sum((2, 5))
    nb = 4.0 * cnt
    div = torch.where(cnt < KSUB, torch.full_like(nb, 4.0 * KSUB), nb) if fault == "sub_div8" else nb
    mb = s / div
    dv = (v - mb[:, :, None, :, :, None]) * ok[:, :, :, :, None, None]
    qb = (dv * dv).sum((2, 5))
    n, mu, m2 = (torch.zeros(P.chunks, P.pr, P.tpc) for _ in range(3))
    for it in range(its):
        n, mu, m2 = _chan32(n, mu, m2, nb[:, it], mb[:, it], qb[:, it])
    tpg = P.tpc // P.G
    n, mu, m2 = (t.view(P.chunks, P.pr, P.G, tpg) for t in (n, mu, m2))
    an, am, aq = (torch.zeros(P.chunks, P.G) for _ in range(3))
    for r in range(P.pr):
        for k in range(tpg):
            an, am, aq = _chan32(an, am, aq, n[:, r, :, k], mu[:, r, :, k], m2[:, r, :, k])
    if fault == "tail_count":
        an = torch.full_like(an, float(STAT_PIX * P.cpg))
    return an, am, aq


def _emu_merge(an, am, aq, eps, fault):
    """[chunks, G] fp32 -> mean, rstd [G] fp32: every lane walks its chunks (c = lane, lane + 64, ...) in fp64, then a butterfly"""
    chunks, G = an.shape
    trips = (chunks + MERGE_LANES - 1) // MERGE_LANES
    padded = [torch.cat([t.to(F64), torch.zeros(trips * MERGE_LANES - chunks, G, dtype=F64)]).view(trips, MERGE_LANES, G) for t in (an, am, aq)]
    n, mu, m2 = (torch.zeros(MERGE_LANES, G, dtype=F64) for _ in range(3))
    for t in range(1 if fault == "merge_trip" else trips):
        nb, mb, qb = (p[t] for p in padded)
        skip = nb == 0
        nn = torch.where(skip, torch.ones_like(n), n + nb)
        d = mb - mu
        mu, m2, n = (torch.where(skip, mu, mu + d * nb / nn), torch.where(skip, m2, m2 + qb + d * d * n * nb / nn), torch.where(skip, n, n + nb))
    lanes = torch.arange(MERGE_LANES)
    o = 1
    while o < MERGE_LANES:
        nb, mb, qb = n[lanes ^ o], mu[lanes ^ o], m2[lanes ^ o]
        live = (n + nb) > 0
        nn = torch.where(live, n + nb, torch.ones_like(n))
        d = mb - mu
        mu, m2, n = (torch.where(live, (n * mu + nb * mb) / nn, mu), torch.where(live, m2 + qb + d * d * n * nb / nn, m2), n + nb)
        o <<= 1
    var = m2[0] / n[0]
    rstd = 1.0 / (torch.sqrt(var) + eps) if fault == "eps_outside" else 1.0 / torch.sqrt(var + eps)
    return mu[0].to(F32), rstd.to(F32)


def _emu_naive_stats(x, P, eps):
    """fault 4: fp32 sums of x and x * x per chunk, var = E[x^2] - mean^2 in fp32"""
    pix, valid = _chunk_pixels(P.HW, P.chunks, STAT_PIX)
    v = torch.where(valid[:, :, None], x[pix.clamp(max=P.HW - 1)], torch.zeros(())).view(P.chunks, STAT_PIX, P.G, P.cpg)
    m = torch.tensor(float(P.cpg * P.HW))
    mean = v.sum((1, 3)).sum(0) / m
    var = ((v * v).sum((1, 3)).sum(0) / m - mean * mean).clamp(min=0)
    return mean, 1.0 / torch.sqrt(var + eps)


def _taps(o, n_in, clamp=True):
    """up2_taps for a vector of output indices"""
    src = (0.5 * (o.to(F32) + 0.5) - 0.5).clamp(min=0)
    i0 = src.long()
    i1 = i0 + ((i0 < n_in - 1).long() if clamp else 1)
    w1 = src - i0.to(F32)
    return i0, i1, 1.0 - w1, w1


def _adj(k_in, fault):
    """up2_adj for every source index -> rows [in, 4], weights [in, 4]"""
    k = torch.arange(k_in)
    first, last = k == 0, k == k_in - 1
    border = 0.75 if fault == "border_weight" else 1.0
    o = torch.stack([torch.where(first, 0, 2 * k - 1), 2 * k, 2 * k + 1, torch.where(last, 2 * k + 1, 2 * k + 2)], 1)
    w = torch.stack([torch.where(first, 0.0, 0.25), torch.where(first, border, 0.75), torch.where(last, border, 0.75),
                     torch.where(last, 0.0, 0.25)], 1).to(F32)
    return o, w


def _image(buf, n, bs, plane, C, extra=0):
    """image n of a strided buffer as [pixels, C]; ``extra`` further pixels behind it (NaN where the buffer ends)"""
    need = n * bs + plane + extra * C
    if need > buf.numel():
        buf = torch.cat([buf, torch.full((need - buf.numel(),), NAN)])
    return buf[n * bs:n * bs + plane + extra * C].view(-1, C)


def _fma(a, b, c):
    """fmaf: the product of two fp32 values is exact in fp64, so this rounds once"""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def _coeffs(pb, mean_n, rstd_n, quad_fault=False):
    """a = rstd * gamma, b = beta - mean * a per channel of one image (fp32)"""
    c = torch.arange(pb.C)
    g = c // pb.cpg
    if quad_fault:
        g = torch.where(c % pb.cpg >= pb.cpg - 4, (g + 1) % pb.G, g)
    a = rstd_n[g] * pb.gamma
    return a, _fma(-mean_n[g], a, pb.beta)


def emulate(pb, fault=None):
    """the channel-last forward, backward and top-map adjoint in fp32 / fp64 as the kernels group them, written into SENT-prefilled
    strided buffers -> the buffers (as ``new_buffers``)"""
    assert fault is None or fault in FAULTS
    P = make_plane(pb.HW, pb.C, pb.G)
    N, C, HW, W = pb.N, pb.C, pb.HW, pb.W
    out = new_buffers(pb)
    bs = {k: (pb.tplane if k in ("top", "dtop") else pb.plane) for k in pb.bs} if fault == "batch_stride" else pb.bs
    mean, rstd = torch.zeros(N, pb.G), torch.zeros(N, pb.G)
    dgb = []
    p = torch.arange(HW)
    for n in range(N):
        x = _image(pb.x_buf, n, bs["x"], pb.plane, C)
        # ---- forward: chunk statistics, fp64 merge, apply
        if fault == "naive_var":
            mean[n], rstd[n] = _emu_naive_stats(x, P, pb.eps)
        else:
            mean[n], rstd[n] = _emu_merge(*_emu_chunk_stats(x, P, fault), pb.eps, fault)
        a, b = _coeffs(pb, mean[n], rstd[n], fault == "quad_group")
        y = _fma(x, a, b)
        if pb.has_top:
            Ht, Wt = (pb.Wt, pb.Ht) if fault == "top_hw_swap" else (pb.Ht, pb.Wt)
            t = _image(pb.top_buf, n, bs["top"], pb.tplane, C, extra=Wt + 2)
            y0, y1, wy0, wy1 = _taps(p // W, Ht, fault != "i1_clamp")
            x0, x1, wx0, wx1 = _taps(p % W, Wt, fault != "i1_clamp")
            wy0, wy1, wx0, wx1 = (w[:, None] for w in (wy0, wy1, wx0, wx1))
            y = y + (wy0 * (wx0 * t[y0 * Wt + x0] + wx1 * t[y0 * Wt + x1]) + wy1 * (wx0 * t[y1 * Wt + x0] + wx1 * t[y1 * Wt + x1]))
        if pb.relu:
            y = y.clamp(min=0)
        out["y"][n * bs["y"]:n * bs["y"] + pb.plane] = y.reshape(-1)
        # ---- backward: fp32 chunk sums, fp64 reduce over the chunks (slice = chunk % 32), group sums, coefficients, apply
        a, b = _coeffs(pb, mean[n], rstd[n])
        gy = _image(pb.gy_buf, n, bs["gy"], pb.plane, C)
        gated = torch.where(_fma(x, a, b) > 0, gy, torch.zeros(())) if pb.relu else gy
        q = gy if fault == "relu_stats_gate" else gated
        pix, valid = _chunk_pixels(HW, P.chunks, STAT_PIX)
        qv = torch.where(valid[:, :, None], q[pix.clamp(max=HW - 1)], torch.zeros(()))
        xv = torch.where(valid[:, :, None], x[pix.clamp(max=HW - 1)], torch.zeros(()))
        sg, sx = qv.sum(1), (qv * xv).sum(1)                                   # [chunks, C] fp32
        use = min(P.chunks, RED_SLICES) if fault == "reduce_trip" else P.chunks
        sgy, sgx = sg[:use].to(F64).sum(0), sx[:use].to(F64).sum(0)
        g = torch.arange(C) // pb.cpg
        mu, rs, gm = mean[n][g].to(F64), rstd[n][g].to(F64), pb.gamma.to(F64)
        t2 = (sgx - mu * sgy) * rs
        gsum = lambda v: v.view(pb.G, pb.cpg).sum(1)[g]                          # noqa: E731
        s1, s2 = gsum(gm * sgy), gsum(gm * t2)
        m = float(pb.cpg * HW)
        Bc = -rs * rs * s2 / m
        cA, cB = (rs * gm).to(F32), Bc.to(F32)
        cD = (-rs * s1 / m - (0.0 if fault == "d_mu" else Bc * mu)).to(F32)
        dgb.append((t2.to(F32), sgy.to(F32)))
        dx = _fma(cA, gated, _fma(cB, x, cD))
        out["dx"][n * bs["dx"]:n * bs["dx"] + pb.plane] = dx.reshape(-1)
        # ---- adjoint of the upsampling: every top pixel gathers 4 x 4 output pixels
        if pb.has_top:
            oy, wy = _adj(pb.Ht, fault)
            ox, wx = _adj(pb.Wt, fault)
            gimg = gy.view(pb.H, W, C)
            acc = torch.zeros(pb.Ht, pb.Wt, C)
            for i in range(4):
                rowacc = torch.zeros(pb.Ht, pb.Wt, C)
                for j in range(4):
                    rowacc = rowacc + wx[None, :, j, None] * gimg[oy[:, i]][:, ox[:, j]]
                acc = acc + wy[:, None, i, None] * rowacc
            out["dtop"][n * bs["dtop"]:n * bs["dtop"] + pb.tplane] = acc.reshape(-1)
    out["mean"][:N * pb.G], out["rstd"][:N * pb.G] = mean.reshape(-1), rstd.reshape(-1)
    dg, db = torch.zeros(C), torch.zeros(C)
    for t2, sgy in dgb[:1] if fault == "image0" else dgb:
        dg, db = dg + t2, db + sgy
    out["dgamma"][:C], out["dbeta"][:C] = dg, db
    return out


@functools.lru_cache(maxsize=4)
def cl_case(name, mode):
    pb = cl_problem(name, mode)
    return pb, cl_reference(pb)
