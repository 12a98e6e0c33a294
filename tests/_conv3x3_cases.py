"""The 3x3 convolution on the GEMM family (csrc/gemm3.hip, gemm3_nt2.h: forward, input gradient, weight and bias gradient):
case tables, an independent fp64 statement of what the kernels claim to compute, the per-element bound, and a torch model of
the kernels' operand planes.  Plain torch, importable without a GPU.  tests/test_conv3x3_cases_cpu.py checks this file (the
definition against F.conv2d / autograd, the tables against the branches they name, the bound against five single faults);
tests/test_conv3x3_routes_gpu.py runs the kernels against it.

Layout: images are channel-last [n, H, W, C]; row r = (i * H + y) * W + x.  TAPS[t] = (ky - 1, kx - 1), t = ky * 3 + kx.
  forward            y[r][co]  = sum_t sum_ci x[r + shift(t)][ci] * W2[co][t * Cin + ci] + b[co]
  input gradient     the same sum with shift(t) negated (`transposed`) and W2 the matrix of the transposed weights
  weight gradient    dW2[s][co][t * Cin + ci] = sum_{r in split s} dy[r][co] * x[r + shift(t)][ci]     (split s = rows [s rps, (s + 1) rps))
  bias gradient      db[s][co] = sum_{r in split s} dy[r][co]
r + shift(t) means pixel (y + dy, x + dx) of the SAME image; a tap off the image contributes nothing.

Bound: |got - ref| <= K * 2^-24 * S per element, S = the same sum over magnitudes (sum |x||w| + |b|, sum |dy||x|, sum |dy|).
K per operand form is measured on the device (table in tests/test_conv3x3_routes_gpu.py) and capped at 32: a kernel that lost
its lowest operand plane sits near 2^-17 S, which a larger K would no longer separate.
"""
import torch

U = 2.0 ** -24
K_CAP = 32
# one K per operand form: 4 x the largest |err| / (2^-24 S) measured on an MI355X, rounded up to a power of two (the table
# with the measured ratios is in the docstring of tests/test_conv3x3_routes_gpu.py)
K = {"bf16x3": 32, "fp16x2": 32, "bf16x3_wgrad": 32, "fp16x2_wgrad": 32}
assert all(k <= K_CAP for k in K.values())

TAPS = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]
F64 = torch.float64


def cdiv(a, b):
    return -(-a // b)


# ---- the definition: nine shifted sums ------------------------------------------------------------------------------------------
def shifted(x, dy, dx):
    """z[i, y, x] = x[i, y + dy, x + dx] where that pixel is on the image, else 0"""
    n, H, W, C = x.shape
    z = torch.zeros_like(x)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        z[:, y0:y1, x0:x1] = x[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return z


def conv_ref(x, w2, bias, transposed):
    """x [n, H, W, Cin], w2 [Cout, 9 * Cin], bias [Cout] or None -> y [n, H, W, Cout] in fp64"""
    x, w2 = x.to(F64), w2.to(F64)
    n, H, W, Cin = x.shape
    sign = -1 if transposed else 1
    y = torch.zeros((n, H, W, w2.shape[0]), dtype=F64)
    for t, (dy, dx) in enumerate(TAPS):
        y += shifted(x, sign * dy, sign * dx) @ w2[:, t * Cin:(t + 1) * Cin].T
    return y if bias is None else y + bias.to(F64)


def conv_scale(x, w2, bias, transposed):
    return conv_ref(x.abs(), w2.abs(), None if bias is None else bias.abs(), transposed)


def wgrad_ref(dy, x, rps):
    """dy [n, H, W, Cout], x [n, H, W, Cin] -> (dW2 per split [ns, Cout, 9 * Cin], db per split [ns, Cout]) in fp64"""
    dy, x = dy.to(F64), x.to(F64)
    n, H, W, Cin = x.shape
    Cout, R = dy.shape[3], n * H * W
    ns = cdiv(R, rps)
    d2 = dy.reshape(R, Cout)
    c = torch.zeros((ns, Cout, 9 * Cin), dtype=F64)
    cs = torch.zeros((ns, Cout), dtype=F64)
    for t, (ty, tx) in enumerate(TAPS):
        xs = shifted(x, ty, tx).reshape(R, Cin)
        for s in range(ns):
            c[s, :, t * Cin:(t + 1) * Cin] = d2[s * rps:(s + 1) * rps].T @ xs[s * rps:(s + 1) * rps]
    for s in range(ns):
        cs[s] = d2[s * rps:(s + 1) * rps].sum(0)
    return c, cs


def wgrad_scale(dy, x, rps):
    return wgrad_ref(dy.abs(), x.abs(), rps)


# ---- the bound ------------------------------------------------------------------------------------------------------------------
def worst(got, ref, S):
    """largest |got - ref| / (2^-24 S) (inf where S == 0 and got != ref, or where got is not finite)"""
    err = (got.to(F64) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / (U * S))
    r = torch.where(torch.isfinite(got.to(F64)), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def within(got, ref, S, k):
    return worst(got, ref, S) <= k


# ---- plane model of the operand splits (gemm3.hip split8 / split8h), products in fp64: for the mutants only ---------------------
def split8(x):
    """fp32 -> three bf16-valued fp32 pieces h, m, l: h and m by truncation (exact remainders), l rounded (+ 0x8000, then cut)"""
    x = x.to(torch.float32).contiguous()

    def cut(v):
        return (v.view(torch.int32) & -65536).view(torch.float32)
    h = cut(x)
    r1 = x - h
    m = cut(r1)
    r2 = r1 - m
    l = ((r2.view(torch.int32) + 0x8000) & -65536).view(torch.float32)
    return h, m, l


def h2_scale(amax):
    """the power of two that puts amax into [2^14, 2^15), from the exponent field (amax below 2^-97 counts as 2^-97)"""
    e = int(torch.tensor(float(amax), dtype=torch.float32).view(torch.int32) >> 23) & 0xFF
    e = max(e, 30)
    return 2.0 ** (14 - (e - 127))


def split8h(x, scale):
    """fp32 -> two fp16-valued fp32 pieces of scale * x: h = fp16(s), l = fp16(s - h), both rounded to nearest"""
    s = x.to(torch.float32) * scale
    h = s.to(torch.float16).to(torch.float32)
    l = (s - h).to(torch.float16).to(torch.float32)
    return h, l


# kept products (piece of A, piece of B): bf16 x 3 keeps six of nine, fp16 x 2 three of four
KEPT = {"bf16x3": [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0)], "fp16x2": [(0, 0), (0, 1), (1, 0)]}
# the lowest plane of both operands gone: bf16 x 2 / fp16 x 1
KEPT_DROPPED = {"bf16x3": [(0, 0), (0, 1), (1, 0), (1, 1)], "fp16x2": [(0, 0)]}


def planes(a, form):
    """-> (pieces, factor that undoes the scale)"""
    if form == "bf16x3":
        return list(split8(a)), 1.0
    sc = h2_scale(a.abs().max())
    return list(split8h(a, sc)), 1.0 / sc


def _gather(x, sign, t, wrong_row=False):
    """the A rows of tap t as the kernels form them: flat row r + shift, clamped into the tensor, zeroed where the tap leaves
    the image of row r.  wrong_row: the fault where the validity of dx = +1 at x = W - 1 is that of the row it wraps onto."""
    n, H, W, C = x.shape
    M = n * H * W
    dy, dx = sign * TAPS[t][0], sign * TAPS[t][1]
    r = torch.arange(M)
    cx, cy = r % W, (r // W) % H
    ok = (cy + dy >= 0) & (cy + dy < H) & (cx + dx >= 0) & (cx + dx < W)
    if wrong_row and dx == 1:
        wraps = (cx == W - 1) & (cy + dy + 1 >= 0) & (cy + dy + 1 < H)
        ok = ok | wraps
    src = (r + dy * W + dx).clamp(0, M - 1)
    return torch.where(ok[:, None], x.reshape(M, C)[src], torch.zeros((), dtype=x.dtype))


def model_conv(x, w2, bias, transposed, form, kept=None, swap=None, wrong_row=False, keep_sign=False):
    """what the TN kernels compute, up to the fp32 accumulation: the kept plane products in fp64.  Faults: `kept` another list of
    products, `swap` two taps exchanged, `wrong_row` (see _gather), `keep_sign` the shift not negated for `transposed`."""
    n, H, W, Cin = x.shape
    M, Cout = n * H * W, w2.shape[0]
    kept = KEPT[form] if kept is None else kept
    xp, xf = planes(x, form)
    wp, wf = planes(w2, form)
    sign = -1 if (transposed and not keep_sign) else 1
    order = list(range(9))
    if swap:
        order[swap[0]], order[swap[1]] = order[swap[1]], order[swap[0]]
    y = torch.zeros((M, Cout), dtype=F64)
    for t in range(9):
        for (i, j) in kept:
            a = _gather(xp[i], sign, order[t], wrong_row).to(F64)
            y += a @ wp[j][:, t * Cin:(t + 1) * Cin].to(F64).T
    y = y * (xf * wf)
    if bias is not None:
        y = y + bias.to(F64)
    return y.view(n, H, W, Cout)


def model_wgrad(dy, x, rps, form, kept=None, late=0):
    """what the NT kernels compute per split, products in fp64.  Fault: `late` = 1, every split starts one row late."""
    n, H, W, Cin = x.shape
    R, Cout = n * H * W, dy.shape[3]
    kept = KEPT[form] if kept is None else kept
    gp, gf = planes(dy.reshape(R, Cout), form)
    xp, xf = planes(x, form)
    ns = cdiv(R, rps)
    c = torch.zeros((ns, Cout, 9 * Cin), dtype=F64)
    for t in range(9):
        xs = [_gather(p, 1, t).to(F64) for p in xp]
        for s in range(ns):
            r0, r1 = s * rps + late, min(R, (s + 1) * rps)
            for (i, j) in kept:
                c[s, :, t * Cin:(t + 1) * Cin] += gp[i][r0:r1].to(F64).T @ xs[j][r0:r1]
    return c * (gf * xf)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def random_operand(shape, seed, spread_log2=4):
    """randn times a per-channel (last dim) power-of-two-range scale spread over 2^spread_log2"""
    g = _gen(seed)
    sc = 2.0 ** (torch.rand(shape[-1], generator=g) * spread_log2 - spread_log2 / 2)
    return (torch.randn(shape, generator=g) * sc).to(torch.float32)


def int_operand(shape, seed, lim):
    return torch.randint(-lim, lim + 1, shape, generator=_gen(seed)).to(torch.float32)


def conv_inputs(case, seed=0, integer=False):
    """-> x [n, H, W, Cin], w2 [Cout, 9 * Cin], bias [Cout] (fp32, CPU)"""
    n, H, W, Cin, Cout = case
    if integer:
        return int_operand((n, H, W, Cin), seed, 8), int_operand((Cout, 9 * Cin), seed + 1, 4), int_operand((Cout,), seed + 2, 16)
    x = random_operand((n, H, W, Cin), seed)
    w2 = random_operand((Cout, 9 * Cin), seed + 1) / (3.0 * Cin ** 0.5)
    return x, w2, torch.randn(Cout, generator=_gen(seed + 2))


def wgrad_inputs(case, seed=0, integer=False):
    """-> dy [n, H, W, Cout], x [n, H, W, Cin] (fp32, CPU)"""
    n, H, W, Cin, Cout, _ = case
    if integer:
        return int_operand((n, H, W, Cout), seed, 4), int_operand((n, H, W, Cin), seed + 1, 8)
    return random_operand((n, H, W, Cout), seed), random_operand((n, H, W, Cin), seed + 1)


# ---- case tables ----------------------------------------------------------------------------------------------------------------
# route -> the kernel a case must land on; the bf16 x 3 routes share the logged name and differ by option and shape
ROUTES = {
    "tile128": dict(form="bf16x3", entry="mpf_gemm3_conv3x3", kernel="gemm3_conv_kernel", opts={}),
    "tile128_forced": dict(form="bf16x3", entry="mpf_gemm3_conv3x3", kernel="gemm3_conv_kernel", opts={"gemm3_two_pass": 0}),
    "two_pass": dict(form="bf16x3", entry="mpf_gemm3_conv3x3", kernel="gemm3_conv_kernel", opts={}),
    "h2": dict(form="fp16x2", entry="mpf_gemm3_conv3x3_h2", kernel="gemm3_conv_kernel<h2>", opts={}),
}
OPTION_DEFAULTS = {"gemm3_two_pass": 256, "gemm3_nt2": 1}

# (route, (n_img, H, W, Cin, Cout), python-level `supported` must admit it)
CONV_CASES = [
    ("tile128", (1, 5, 12, 32, 96), True),        # M = 60: one partial tile, column tail
    ("tile128", (2, 9, 7, 64, 64), True),         # M = 126: image boundary inside the tile
    ("tile128", (3, 7, 9, 32, 160), True),        # M = 189: row 128 is mid-row of image 3; second column tile partial
    ("tile128", (1, 4, 4, 32, 36), False),        # Cout % 4 tail (C ABI only)
    ("tile128", (3, 2, 2, 32, 32), True),         # smallest shape `supported` admits
    ("tile128", (1, 1, 16, 32, 32), False),       # one-pixel-high / -wide / single-pixel images (C ABI only)
    ("tile128", (1, 16, 1, 32, 32), False),
    ("tile128", (4, 1, 1, 32, 32), False),
    ("tile128_forced", (1, 5, 8, 32, 256), True),
    ("two_pass", (1, 5, 8, 32, 256), True),
    ("two_pass", (2, 9, 15, 64, 512), True),
    ("h2", (2, 9, 7, 32, 256), True),
    ("h2", (1, 6, 8, 256, 256), True),
    ("h2", (1, 1, 8, 32, 256), False),
]
CONV_RUNS = [(route, case, tr) for route, case, _ in CONV_CASES for tr in (0, 1)]


def conv_id(route, case, tr=None):
    s = route + "-" + "x".join(str(v) for v in case)
    return s if tr is None else s + ("-T" if tr else "-F")


def conv_geometry(route, case):
    """M, the row / column tile counts and the kernel's column tile width, by the cdiv rules of g3_conv_route"""
    n, H, W, Cin, Cout = case
    M = n * H * W
    bn = 128 if route in ("tile128", "tile128_forced") else 256
    return dict(M=M, tiles_m=cdiv(M, 128), tiles_n=cdiv(Cout, bn) if bn == 128 else Cout // 256, bn=bn, nk=9 * Cin // 32)


def expected_two_pass(route, case, two_pass_opt):
    """g3_conv_route's choice restated: fp16 x 2 always, bf16 x 3 when the option is on and Cout % 256 == 0"""
    return route == "h2" or (two_pass_opt > 0 and case[4] % 256 == 0)


def python_supported_shape(case):
    """the shape part of conv3x3.supported"""
    n, H, W, Cin, Cout = case
    return Cin % 32 == 0 and Cout % 32 == 0 and n * H * W * max(Cin, Cout) < 2 ** 31 and H >= 2 and W >= 2


WGRAD_ROUTES = {
    "nt128": dict(form="bf16x3", entry="mpf_gemm3_conv3x3_wgrad", kernel="gemm3_nt_kernel<conv3x3>", opts={}, bm=128, bn=128),
    "nt128_h2": dict(form="fp16x2", entry="mpf_gemm3_conv3x3_wgrad_h2", kernel="gemm3_nt_kernel<conv3x3 h2>", opts={}, bm=128, bn=128),
    "nt256_h2": dict(form="fp16x2", entry="mpf_gemm3_conv3x3_wgrad_h2", kernel="gemm3_nt_kernel<conv3x3 h2 256x256>", opts={}, bm=256, bn=256),
    "nt128_h2_forced": dict(form="fp16x2", entry="mpf_gemm3_conv3x3_wgrad_h2", kernel="gemm3_nt_kernel<conv3x3 h2>", opts={"gemm3_nt2": 0},
                            bm=128, bn=128),
}
# (n, H, W, Cin, Cout, rows_per_split): W % 8 == 0, Cin % 128 == 0, rps % 32 == 0
WGRAD_128 = [
    (1, 8, 8, 128, 64, 32),        # splits aligned to image rows
    (2, 5, 8, 128, 96, 32),        # R = 80: image boundary at row 40 inside a K step, last split partial (16 rows)
    (3, 3, 8, 128, 200, 64),       # Cout tail 128 + 72, last split of 8 rows
    (3, 3, 8, 128, 64, 128),       # one split, tail path only
    (2, 1, 8, 128, 32, 32),        # H = 1
    (1, 4, 24, 128, 32, 32),       # W = 24
]
WGRAD_256 = [(1, 8, 8, 256, 256, 32), (2, 5, 8, 256, 512, 32)]
WGRAD_RUNS = ([(r, c, cs) for r in ("nt128", "nt128_h2") for c in WGRAD_128 for cs in (False, True)]
              + [(r, c, cs) for r in ("nt256_h2", "nt128_h2_forced") for c in WGRAD_256 for cs in (False, True)])


def wgrad_id(route, case, csum):
    return route + "-" + "x".join(str(v) for v in case) + ("-csum" if csum else "")


def wgrad_geometry(route, case):
    n, H, W, Cin, Cout, rps = case
    R = n * H * W
    ns = cdiv(R, rps)
    r = WGRAD_ROUTES[route]
    return dict(R=R, ns=ns, last_rows=R - (ns - 1) * rps, tiles_m=cdiv(Cout, r["bm"]), tiles_n=cdiv(9 * Cin, r["bn"]))


# ---- one-hot probes and poison pixels -------------------------------------------------------------------------------------------
def probe_pixels(n, H, W):
    """(image, y, x): the four corners, an edge midpoint and the interior of image 0; first and last pixel of a middle image"""
    mid = n // 2
    px = [(0, 0, 0), (0, 0, W - 1), (0, H - 1, 0), (0, H - 1, W - 1), (0, 0, W // 2), (0, H // 2, W // 2), (mid, 0, 0), (mid, H - 1, W - 1)]
    return sorted(set(px))


def probe_expected(n, H, W, pixel, transposed):
    """one-hot pixel p, w[tap] = 1 + tap: y[q] = 1 + t exactly where q + sign * TAPS[t] = p lies on p's image, else 0 -> [n, H, W]"""
    i, py, px = pixel
    sign = -1 if transposed else 1
    e = torch.zeros((n, H, W), dtype=F64)
    for t, (dy, dx) in enumerate(TAPS):
        qy, qx = py - sign * dy, px - sign * dx
        if 0 <= qy < H and 0 <= qx < W:
            e[i, qy, qx] = 1 + t
    return e


def poison_pixels(n, H, W):
    """the isolation pixels: (i, y, 0) for an interior y; (i, 0, 0) with i > 0; (i, H - 1, W - 1) with i < n - 1; one interior pixel"""
    assert n >= 3 and H >= 3 and W >= 3
    return [(1, H // 2, 0), (1, 0, 0), (n - 2, H - 1, W - 1), (1, H // 2, W // 2)]


def neighbourhood(n, H, W, pixel):
    """bool [n, H, W]: the pixel's 3x3 neighbourhood inside its image (the outputs that read it, in either direction)"""
    i, py, px = pixel
    m = torch.zeros((n, H, W), dtype=torch.bool)
    m[i, max(0, py - 1):py + 2, max(0, px - 1):px + 2] = True
    return m


# isolation shapes: three images so that a middle image has neighbours on both sides; the tile boundary (row 128) inside image 1
ISOLATION = [("tile128", (3, 9, 11, 32, 64)), ("two_pass", (3, 9, 11, 32, 256)), ("h2", (3, 9, 11, 32, 256))]
ISOLATION_WGRAD = [("nt128", (3, 5, 8, 128, 64, 32)), ("nt128_h2", (3, 5, 8, 128, 64, 32)), ("nt256_h2", (3, 5, 8, 256, 256, 32))]

# python level: (N, C, Cout, H, W, weight-gradient path)
PYTHON_CASES = [(2, 256, 256, 6, 8, "gemm3_nt_kernel<conv3x3 h2 256x256>"), (2, 128, 64, 5, 8, "gemm3_nt_kernel<conv3x3>"),
                (2, 64, 64, 9, 7, "aten")]
