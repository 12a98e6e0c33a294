"""The problems, fp64 references, bounds, grid-rule mirror and single-fault emulation of the 256-channel residual LayerNorm family
(csrc/elementwise.hip: mpf_res_ln256_forward / _forward_b, the six mpf_res_ln256_backward* entries, mpf_ln_partial_reduce;
csrc/row_chain.hip: mpf_lin256_res_ln_forward, mpf_ln256_mlp3_forward).  No GPU and no library is needed to import this file.
tests/test_resln_cases_cpu.py holds the row counts to the block counts they are listed for, the mirror to the built library, aten's
fp32 LayerNorm to the bounds at half their width, the exact problem to exactness in two summation orders, and every fault of the
emulation to a failing check; tests/test_resln_parity_gpu.py runs the same problems through the C ABI and the Python wrappers and
the same check functions.

Buffers: every input is PAD elements longer than the rows x 256 (or rows) the call addresses, NaN behind them (``padd`` holds exactly
padd_rows rows, then NaN); every output starts as SENT everywhere and is as much longer.  After a call the tail must hold SENT bit
for bit, every addressed element must be finite and differ from SENT (``take``).

References are fp64 on the fp32 values, u = 2^-24, eps = the fp32 value of 1e-5.  Forward, referred to the s the call wrote (x where
t is absent), with mu, var of that s, sd = sqrt(var + eps), rstd = 1 / sd, a = rstd gamma:
    s_out  == x + float(t) in fp32, bit for bit        y16 == bf16 round-to-nearest-even of the y32 of the same call, bit for bit
    mean   K u (|mu| + sqrt(var))                       y_plus == y32 + padd[row % padd_rows] in fp32, bit for bit
    rstd   K u rstd (1 + |mu| / sd)
    y32    K u (|a| (|s| + |mu|) + |beta|)
Backward, with s, mean, rstd taken as given (fp32), g = gy32 + gy16 + gy_plus, |g| the sum of the three magnitudes,
xt = (|s| + |mu|) rstd:
    ds32   K u (|a| |g| + rstd sum_c|gamma g| / 256 + xt rstd sum_c(|gamma g| xt) / 256)
    dgamma (K + D) u sum_rows |g| xt        dbeta (K + D) u sum_rows |g|
D = the longest chain of fp32 adds of the form (``depth``): rows of a wave, the 4 waves, then the blocks as the form sums them.
The rows of the two large-mean distributions also require max|ds - ref| <= 4 max|ds_aten - ref| with aten's fp32 backward on the same
device, input, mean and rstd: the ds form undoes the cancellation the kernel has.
K: aten's fp32 native_layer_norm and its backward on the CPU, at K = 1 over every case (tests/test_resln_cases_cpu.py has the figures):
mean 2.75, rstd 2.01, ds32 2.64, dgamma 1.23, dbeta 1.90 - and y32 16.5.  Twice the worst, rounded up to a power of two, is 64.

Y FORM.  The y32 form has no sigma term, but the mean form allows the mean an error of K u sigma, which reaches y as K u |a| sigma =
K u |gamma|: at an element of a zero-mean row with |s| + |mu| << sigma and a small |beta| the form is a small fraction of that (aten
is at 16.5 where |s| = 9e-4, |mu| = 8e-3; this file's emulation at 6.3).  So the y32 form as stated is held at KY = 64, what the
measurement gives, and every other quantity at K = 8, twice aten's worst of the rest (3.0) rounded up, which is narrower than 64 and so
asks no less.  On top, y32 is held to the form with the missing term, K u (|a| (|s| + |mu| + sigma) + |beta|), at K = 8 (aten: 3.0): that
is the check that is sharp at every element."""
import functools
import zlib
from types import SimpleNamespace

import torch

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
U = 2.0 ** -24
K = 8.0
KY = 64.0                                      # of the y32 form without the sigma term (Y FORM in the docstring)
EPS = float(torch.tensor(1e-5, dtype=F32))
ATEN_FACTOR = 4.0
SENT = -3.0e19
NAN = float("nan")
PAD = 3 * 256 + 4                              # elements behind every buffer: more than a workgroup's further rows of a short block
C = 256

# ---- grid rule of the backward (ln_grid of csrc/elementwise.hip) and the depth of its sums ---------------------------------------------
FWD_ROWS = (1, 3, 4, 5, 17, 1027)
# rows -> blocks it is listed for
BWD_ROWS = {1: 1, 4: 1, 5: 2, 124: 31, 128: 32, 132: 33, 900: 225, 1024: 256, 1028: 257, 4096: 1024, 4097: 513, 8195: 683}
DET_MAX_ROWS = 1028
FORMS = ("atomic", "ws", "partial", "det")
SUBSET_ROWS = 125
OPERANDS = ("gy_plus", "gy16", "gy16+gy_plus", "gy32", "gy32+gy_plus", "gy32+gy16", "gy32+gy16+gy_plus")
OUTPUTS = ("ds32", "ds16", "ds32+ds16")
CHAIN_LIN_ROWS = (1, 15, 16, 17, 230)
CHAIN_MLP_ROWS = (1, 15, 16, 17, 219)
WRAPPER_ROWS = (1024, 1025)


def grid_rule(rows):
    """-> (rows per workgroup, workgroups)"""
    ceil = lambda a, b: -(-a // b)                                   # noqa: E731
    rpb = ceil(ceil(rows, 1024), 4) * 4
    return rpb, ceil(rows, rpb)


def workspace_bytes(rows):
    return 0 if rows <= 0 else grid_rule(rows)[1] * 512 * 4


def det_workspace_bytes(rows):
    return 0 if rows <= 0 else 256 + workspace_bytes(rows)


def depth(form, rows):
    """longest chain of fp32 adds behind one dgamma / dbeta element: rpb / 4 rows of a wave, 3 adds over the waves, then the blocks
    (ws / partial + reduce: ceil(blocks / 32) per slice and 32 slices; det: ceil(blocks / 2) per slice and one add; atomics: blocks)"""
    rpb, blocks = grid_rule(rows)
    over = {"ws": -(-blocks // 32) + 32, "partial": -(-blocks // 32) + 32, "det": -(-blocks // 2) + 1, "atomic": blocks}[form]
    return rpb // 4 + 3 + over


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and bool((bits(a) == bits(b)).all())


def inbuf(vals, pad=PAD):
    """the values, then ``pad`` NaN elements (flat)"""
    return torch.cat([vals.reshape(-1), torch.full((pad,), NAN, dtype=vals.dtype)])


def outbuf(n, dtype=F32, pad=PAD):
    return torch.full((int(n) + pad,), SENT, dtype=dtype)


def take(case, what, buf, n):
    """an output buffer that started as SENT -> its first n elements, after asserting that the tail still holds SENT bit for bit and
    that every addressed element is finite and was written"""
    buf = buf.detach().cpu().reshape(-1)
    assert buf.numel() > n, (case, what, buf.numel(), n)
    sent = int(bits(torch.full((1,), SENT, dtype=buf.dtype)))
    assert bool((bits(buf[n:]) == sent).all()), f"{case}: {what} was written behind its {n} elements"
    vals = buf[:n]
    assert bool(torch.isfinite(vals.float()).all()), f"{case}: {what} is not finite (a NaN tail was read, or worse)"
    assert bool((bits(vals) != sent).all()), f"{case}: an addressed element of {what} was not written"
    return vals


def hold(case, what, got, ref, bound, k=K):
    """print the worst error of this comparison, then assert |got - ref| <= k * bound for every element -> worst err / (k * bound)
    (an element whose bound is 0 must be exact)"""
    got = got.detach().to(F64).cpu()
    assert got.shape == ref.shape, (case, what, got.shape, ref.shape)
    err = (got - ref).abs()
    kb = k * bound
    frac = torch.where(kb > 0, err / kb.clamp(min=1e-300), torch.where(err == 0, 0.0, float("inf")).to(F64))
    bad = int((~(err <= kb)).sum())
    print(f"[resln] {case} | {what} | max abs err {float(err.max()):.3e} | worst err/bound {float(frac.max()):.3e} | "
          f"{bad} of {frac.numel()} outside")
    assert bool(torch.isfinite(got).all()) and bad == 0, (case, what, float(err.max()), float(frac.max()), bad)
    return float(frac.max())


def exact(case, what, got, ref):
    got = got.detach().to(F64).cpu()
    bad = int((got != ref).sum())
    print(f"[resln] {case} | {what} | exact | max abs err {float((got - ref).abs().max()):.3e} | {bad} of {got.numel()} differ")
    assert got.shape == ref.shape and bad == 0, (case, what, bad)


# ---- problems --------------------------------------------------------------------------------------------------------------------------
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def draw(dist, rows, g):
    """-> ([rows, 256] fp32, mask of the large-mean rows)"""
    r = lambda *s: torch.randn(*s, generator=g)                      # noqa: E731
    none, every = torch.zeros(rows, dtype=torch.bool), torch.ones(rows, dtype=torch.bool)
    if dist == "std":
        return r(rows, C), none
    if dist == "m40":
        return 40.0 + 0.3 * r(rows, C), every
    if dist == "m300":
        return 300.0 + 0.05 * r(rows, C), every
    if dist == "const":                                              # a different constant per row, one row all zero
        c = 3.0 * r(rows, 1)
        c[rows // 2] = 0.0
        return c.expand(rows, C).clone(), none
    if dist == "tiny":
        return 1e-20 * r(rows, C), none
    if dist == "big":
        return 1e15 * r(rows, C), none
    assert dist == "mix"                                             # row i: m300, const, std for i % 3 = 0, 1, 2
    v = torch.stack([300.0 + 0.05 * r(rows, C), (3.0 * r(rows, 1)).expand(rows, C), r(rows, C)])
    i = torch.arange(rows)
    out = v[i % 3, i].clone()
    if rows > 1:
        out[4 if rows > 4 else 1] = 0.0
    return out, i % 3 == 0


def _params(g):
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    gamma[7] = 0.0
    gamma[100] = -gamma[100].abs() - 0.25
    return gamma, torch.randn(C, generator=g)


def _fwd_cases():
    c = {}
    for rows in FWD_ROWS:
        for t in ("none", "f32", "bf16"):
            c[f"mix r{rows} t={t}"] = dict(rows=rows, dist="mix", t=t, padd_rows=0)
    for dist in ("std", "m40", "m300", "const", "tiny", "big"):
        c[f"{dist} r17 t=none"] = dict(rows=17, dist=dist, t="none", padd_rows=0)
    for rows in (5, 17):
        for pr in (1, 3, 7):
            c[f"std r{rows} t=bf16 padd{pr}"] = dict(rows=rows, dist="std", t="bf16", padd_rows=pr)
    c["m40 r1027 t=f32 padd3"] = dict(rows=1027, dist="m40", t="f32", padd_rows=3)
    return c


FWD_CASES = _fwd_cases()


def fwd_problem(name, rows=None, dist=None, t=None, padd_rows=None):
    row = FWD_CASES.get(name, {})
    rows, dist, t = rows or row["rows"], dist or row["dist"], t or row["t"]
    padd_rows = row.get("padd_rows", 0) if padd_rows is None else padd_rows
    g = _gen("fwd " + name)
    pb = SimpleNamespace(name=name, rows=rows, dist=dist, t_kind=t, padd_rows=padd_rows, eps=EPS)
    pb.x, pb.large = draw(dist, rows, g)
    scale = {"tiny": 1e-20, "big": 1e15}.get(dist, 0.5)
    pb.t = None if t == "none" else (scale * torch.randn(rows, C, generator=g)).to(BF16 if t == "bf16" else F32)
    pb.gamma, pb.beta = _params(g)
    pb.padd = torch.randn(padd_rows, C, generator=g) if padd_rows else None
    pb.x_buf, pb.t_buf = inbuf(pb.x), (inbuf(pb.t) if pb.t is not None else None)
    pb.padd_buf = inbuf(pb.padd) if padd_rows else None
    pb.s = pb.x if pb.t is None else pb.x + pb.t.float()
    return pb


def fwd_buffers(pb, want=("s_out", "y32", "y16", "y_plus")):
    n = pb.rows * C
    b = SimpleNamespace(s_out=None, y32=None, y16=None, y_plus=None, mean=outbuf(pb.rows), rstd=outbuf(pb.rows))
    for k in want:
        if k != "y_plus" or pb.padd_rows:
            setattr(b, k, outbuf(n, BF16 if k == "y16" else F32))
    return b


def fwd_reference(s, gamma, beta, eps=EPS):
    """fp32 s [rows, 256] -> fp64 mean, rstd, y and the bound of each at K = 1"""
    s = s.to(F64)
    gm, bt = gamma.to(F64), beta.to(F64)
    mu = s.mean(1)
    var = ((s - mu[:, None]) ** 2).mean(1)
    sd = torch.sqrt(var + eps)
    r = SimpleNamespace(mean=mu, rstd=1.0 / sd)
    r.y = (s - mu[:, None]) * r.rstd[:, None] * gm + bt
    r.b_mean = U * (mu.abs() + torch.sqrt(var))
    r.b_rstd = U * r.rstd * (1.0 + mu.abs() / sd)
    a = r.rstd[:, None] * gm.abs()
    r.b_y = U * (a * (s.abs() + mu.abs()[:, None]) + bt.abs())
    r.b_y_sigma = r.b_y + U * a * torch.sqrt(var)[:, None]
    return r


def check_forward(pb, out, k=K, route="", s_given=None):
    """the buffers of one forward call against the problem -> {quantity: worst err / bound}.  ``s_given``: the s the LayerNorm part
    is referred to where the call did not get it as x + t (the row chain)"""
    case, n = f"fwd {pb.name} {route}".strip(), pb.rows * C
    frac = {}
    s = pb.s if s_given is None else s_given
    if out.s_out is not None:
        s = take(case, "s_out", out.s_out, n).view(pb.rows, C)
        if s_given is None:
            assert same_bits(s, pb.s), f"{case}: s_out is not the fp32 sum x + float(t)"
    ref = fwd_reference(s, pb.gamma, pb.beta, pb.eps)
    frac["mean"] = hold(case, "mean", take(case, "mean", out.mean, pb.rows), ref.mean, ref.b_mean, k)
    frac["rstd"] = hold(case, "rstd", take(case, "rstd", out.rstd, pb.rows), ref.rstd, ref.b_rstd, k)
    y32 = None
    if out.y32 is not None:
        y32 = take(case, "y32", out.y32, n).view(pb.rows, C)
        frac["y32"] = hold(case, "y32", y32, ref.y, ref.b_y, k * KY / K)
        frac["y32_sigma"] = hold(case, "y32 (sigma form)", y32, ref.y, ref.b_y_sigma, k)
    if out.y16 is not None:
        y16 = take(case, "y16", out.y16, n).view(pb.rows, C)
        if y32 is not None:
            assert same_bits(y16, y32.to(BF16)), f"{case}: y16 is not the round-to-nearest-even bf16 of y32"
        else:                                                   # one rounding to bf16 on top of the y32 form
            frac["y16"] = hold(case, "y16", y16, ref.y, ref.b_y_sigma + 2.0 ** -8 * ref.y.abs() / k, k)
    if out.y_plus is not None:
        assert y32 is not None
        yp = take(case, "y_plus", out.y_plus, n).view(pb.rows, C)
        assert same_bits(yp, y32 + pb.padd[torch.arange(pb.rows) % pb.padd_rows]), f"{case}: y_plus is not y32 + padd[row % padd_rows] in fp32"
    return frac


def y_bounds(pb):
    """the fp32 values mpf_res_ln256_forward_b writes: 16 max|gamma| + max|beta|, and that + max|padd|"""
    b = torch.tensor(16.0, dtype=F32) * pb.gamma.abs().max() + pb.beta.abs().max()
    return b, (b + pb.padd.abs().max() if pb.padd is not None else None)


def aten_forward(pb, device="cpu"):
    """aten's fp32 native_layer_norm on s -> output buffers as a call that wrote y32 would leave them"""
    y, mean, rstd = torch.native_layer_norm(pb.s.to(device), [C], pb.gamma.to(device), pb.beta.to(device), pb.eps)
    tail = lambda v: torch.cat([v.reshape(-1).cpu(), outbuf(0)])                          # noqa: E731
    return SimpleNamespace(s_out=None, y32=tail(y), y16=None, y_plus=None, mean=tail(mean), rstd=tail(rstd))


# ---- backward problems -----------------------------------------------------------------------------------------------------------------
def _bwd_cases():
    c = {}
    for rows in BWD_ROWS:
        c[f"mix r{rows}"] = dict(rows=rows, dist="mix", ops="gy32", ds="ds32")
    for dist in ("std", "m40", "m300", "const", "tiny", "big"):
        c[f"{dist} r{SUBSET_ROWS}"] = dict(rows=SUBSET_ROWS, dist=dist, ops="gy32", ds="ds32+ds16")
    for ops in OPERANDS:
        for ds in OUTPUTS:
            c[f"std r{SUBSET_ROWS} {ops} -> {ds}"] = dict(rows=SUBSET_ROWS, dist="std", ops=ops, ds=ds)
    return c


BWD_CASES = _bwd_cases()


def _finish_bwd(pb):
    pb.s_buf, pb.mean_buf, pb.rstd_buf = inbuf(pb.s), inbuf(pb.mean), inbuf(pb.rstd)
    pb.gy32_buf, pb.gy16_buf, pb.gyp_buf = (inbuf(v) if v is not None else None for v in (pb.gy32, pb.gy16, pb.gy_plus))
    pb.rpb, pb.blocks = grid_rule(pb.rows)
    return pb


def bwd_problem(name, rows=None, dist=None, ops=None, ds=None):
    row = BWD_CASES.get(name, {})
    rows, dist, ops, ds = rows or row["rows"], dist or row["dist"], ops or row["ops"], ds or row["ds"]
    g = _gen("bwd " + name)
    pb = SimpleNamespace(name=name, rows=rows, dist=dist, ops=ops, ds=ds, eps=EPS, exact=False)
    pb.s, pb.large = draw(dist, rows, g)
    st = fwd_reference(pb.s, torch.ones(C), torch.zeros(C))
    pb.mean, pb.rstd = st.mean.to(F32), st.rstd.to(F32)                # the forward's outputs, taken as given
    pb.gamma, _ = _params(g)
    o = ops.split("+")
    pb.gy32 = torch.randn(rows, C, generator=g) if "gy32" in o else None
    pb.gy16 = torch.randn(rows, C, generator=g).to(BF16) if "gy16" in o else None
    pb.gy_plus = torch.randn(rows, C, generator=g) if "gy_plus" in o else None
    return _finish_bwd(pb)


def exact_problem(rows):
    """a backward whose every product and sum is an integer or a multiple of 2^-11 far below 2^24: s integer in [-4, 4], mean an
    integer per row, rstd 1 or 0.5, gamma in {+-1, +-2, 0}, all three gy integer in [-3, 3].  ds32, dgamma and dbeta are then exact
    in fp32 in ANY order of summation, so a dropped, doubled or misassigned row moves an answer by a whole unit of its grid"""
    g = _gen(f"exact {rows}")
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).to(F32)             # noqa: E731
    pb = SimpleNamespace(name=f"exact r{rows}", rows=rows, dist="exact", ops="gy32+gy16+gy_plus", ds="ds32", eps=EPS, exact=True)
    pb.s, pb.mean = ri(-4, 4, rows, C), ri(-2, 2, rows)
    pb.rstd = torch.where(ri(0, 1, rows) > 0, 1.0, 0.5).to(F32)
    pb.gamma = torch.tensor([1.0, -1.0, 2.0, -2.0, 0.0])[torch.randint(0, 5, (C,), generator=g)]
    pb.gy32, pb.gy16, pb.gy_plus = ri(-3, 3, rows, C), ri(-3, 3, rows, C).to(BF16), ri(-3, 3, rows, C)
    pb.large = torch.zeros(rows, dtype=torch.bool)
    return _finish_bwd(pb)


def _g_parts(pb):
    return [v.to(F64) for v in (pb.gy32, pb.gy16, pb.gy_plus) if v is not None]


def bwd_reference(pb):
    """-> fp64 ds, dgamma, dbeta and the bound of each at K = 1 (``s_dgamma``, ``s_dbeta``: the sums the depth forms scale)"""
    s, mu, rs, gm = pb.s.to(F64), pb.mean.to(F64)[:, None], pb.rstd.to(F64)[:, None], pb.gamma.to(F64)
    parts = _g_parts(pb)
    g, ga = sum(parts), sum(p.abs() for p in parts)
    xh = (s - mu) * rs
    dg = g * gm
    s1, s2 = dg.mean(1, keepdim=True), (dg * xh).mean(1, keepdim=True)
    r = SimpleNamespace(ds=rs * (dg - s1 - xh * s2), dgamma=(g * xh).sum(0), dbeta=g.sum(0))
    xt = (s.abs() + mu.abs()) * rs
    gg = gm.abs() * ga
    r.b_ds = U * (rs * gg + rs * gg.mean(1, keepdim=True) + xt * rs * (gg * xt).mean(1, keepdim=True))
    r.b_dgamma, r.b_dbeta = U * (ga * xt).sum(0), U * ga.sum(0)
    return r


def bwd_buffers(pb, form, ds=None, zero_atomic=True):
    """-> output buffers of one backward call: ds32 / ds16 as the case asks, dgamma / dbeta [256] each (the atomic form accumulates:
    its 256 elements start as zero)"""
    ds = (ds or pb.ds).split("+")
    n = pb.rows * C
    b = SimpleNamespace(ds32=outbuf(n) if "ds32" in ds else None, ds16=outbuf(n, BF16) if "ds16" in ds else None, ds_amax=None)
    b.dgamma, b.dbeta = outbuf(C), outbuf(C)
    if form == "atomic" and zero_atomic:
        b.dgamma[:C], b.dbeta[:C] = 0.0, 0.0
    return b


def check_backward(pb, ref, out, form, k=K, route=""):
    """the buffers of one backward call -> {quantity: worst err / bound}; ``out.ds_amax`` (a float, or None) must equal max|ds32|"""
    case, n = f"bwd {pb.name} {form} {route}".strip(), pb.rows * C
    frac, ds32 = {}, None
    if out.ds32 is not None:
        ds32 = take(case, "ds32", out.ds32, n).view(pb.rows, C)
        frac["ds32"] = hold(case, "ds32", ds32, ref.ds, ref.b_ds, k)
    if out.ds16 is not None:
        ds16 = take(case, "ds16", out.ds16, n).view(pb.rows, C)
        if ds32 is not None:
            assert same_bits(ds16, ds32.to(BF16)), f"{case}: ds16 is not the round-to-nearest-even bf16 of ds32"
        else:
            frac["ds16"] = hold(case, "ds16", ds16, ref.ds, ref.b_ds + 2.0 ** -8 * ref.ds.abs() / k, k)
    if out.ds_amax is not None:
        assert ds32 is not None and float(out.ds_amax) == float(ds32.abs().max()), (case, "ds_amax", float(out.ds_amax), float(ds32.abs().max()))
    if out.dgamma is not None:
        kd = k + depth(form, pb.rows)
        frac["dgamma"] = hold(case, "dgamma", take(case, "dgamma", out.dgamma, C), ref.dgamma, ref.b_dgamma, kd)
        frac["dbeta"] = hold(case, "dbeta", take(case, "dbeta", out.dbeta, C), ref.dbeta, ref.b_dbeta, kd)
    return frac


def check_exact(pb, ref, out, form, route=""):
    case = f"bwd {pb.name} {form} {route}".strip()
    assert pb.exact
    exact(case, "ds32", take(case, "ds32", out.ds32, pb.rows * C).view(pb.rows, C), ref.ds)
    exact(case, "dgamma", take(case, "dgamma", out.dgamma, C), ref.dgamma)
    exact(case, "dbeta", take(case, "dbeta", out.dbeta, C), ref.dbeta)


def g_sum32(pb):
    """g as one fp32 tensor, added in the kernels' order (for aten, which takes one upstream gradient)"""
    parts = [v.float() for v in (pb.gy32, pb.gy16, pb.gy_plus) if v is not None]
    g = parts[0]
    for p in parts[1:]:
        g = g + p
    return g


def aten_backward(pb, device="cpu"):
    """aten's fp32 native_layer_norm_backward on the same s, mean, rstd -> (ds, dgamma, dbeta) fp32 on the CPU"""
    d = lambda v: v.to(device)                                                            # noqa: E731
    ds, dg, db = torch.ops.aten.native_layer_norm_backward(d(g_sum32(pb)), d(pb.s), [C], d(pb.mean)[:, None], d(pb.rstd)[:, None],
                                                           d(pb.gamma), d(torch.zeros(C)), [True, True, True])
    return ds.cpu(), dg.cpu(), db.cpu()


def check_vs_aten(pb, ref, ds, ds_aten, route=""):
    """the large-mean rows: max|ds - ref| <= 4 max|ds_aten - ref| -> the ratio (None where the problem has no such row)"""
    if not bool(pb.large.any()):
        return None
    e = float((ds.detach().to(F64).cpu() - ref.ds)[pb.large].abs().max())
    ea = float((ds_aten.detach().to(F64).cpu() - ref.ds)[pb.large].abs().max())
    print(f"[resln] bwd {pb.name} {route} | ds of the large-mean rows against aten fp32 | max abs err {e:.3e} | aten {ea:.3e} | ratio {e / ea:.3e}")
    assert e <= ATEN_FACTOR * ea, (pb.name, e, ea)
    return e / ea


# ---- the row chain: x + bf16(a W^T + b), then the LayerNorm ---------------------------------------------------------------------------------
def lin_problem(rows):
    g = _gen(f"lin {rows}")
    pb = SimpleNamespace(name=f"lin r{rows}", rows=rows, dist="std", t_kind="chain", padd_rows=0, padd=None, eps=EPS)
    pb.a = torch.randn(rows, C, generator=g).to(BF16)
    pb.w = (torch.randn(C, C, generator=g) / 16).to(BF16)
    pb.b = torch.randn(C, generator=g).to(BF16)
    pb.x = torch.randn(rows, C, generator=g)
    pb.gamma, pb.beta = _params(g)
    pb.a_buf, pb.x_buf = inbuf(pb.a), inbuf(pb.x)
    pb.s = None
    return pb


def check_lin(pb, out, k=K, route=""):
    """s_out against fp64 x + (a W^T + b) within 2^-8 |t| + (256 + 8) 2^-22 S + u |x + t| (t the projection, S = sum|a||w| + |b|: the
    small-row GEMM bound of a bf16 result, plus one fp32 add), then mean, rstd, y32, y16 against that s_out"""
    case = f"fwd {pb.name} {route}".strip()
    s = take(case, "s_out", out.s_out, pb.rows * C).view(pb.rows, C)
    a, w, b = pb.a.to(F64), pb.w.to(F64), pb.b.to(F64)
    t = a @ w.t() + b
    S = a.abs() @ w.abs().t() + b.abs()
    ref = pb.x.to(F64) + t
    frac = {"s_out": hold(case, "s_out", s, ref, 2.0 ** -8 * t.abs() + (256 + 8) * 2.0 ** -22 * S + U * ref.abs(), 1.0)}
    frac.update(check_forward(pb, out, k, route, s_given=s))
    return frac


def mlp_problem(rows):
    g = _gen(f"mlp {rows}")
    pb = SimpleNamespace(name=f"mlp r{rows}", rows=rows, eps=EPS)
    pb.x = 2.0 * torch.randn(rows, C, generator=g)
    pb.gamma, pb.beta = _params(g)
    pb.ws = [(torch.randn(C, C, generator=g) / 16).to(BF16) for _ in range(3)]
    pb.bs = [(0.2 * torch.randn(C, generator=g)).to(BF16) for _ in range(3)]
    pb.x_buf = inbuf(pb.x)
    return pb


# ---- fp32 emulation of the kernels' expressions (torch's own summation order), one fault at a time ------------------------------------------
FAULTS = ("one_pass_var", "eps_after_sqrt", "eps_omitted", "div255", "padd_clamp", "s_out_is_x", "y16_trunc", "no_s1", "no_s2",
          "dgamma_from_dg", "gy16_ignored", "gy_plus_not_in_params", "reduce_skips_last_block", "short_block_skips_last_row", "amax_before_rstd")
FWD_FAULTS = FAULTS[:7]
# the case every fault is held to, and for the backward ones the form
FAULT_CASE = {
    "one_pass_var": "m300 r17 t=none", "eps_after_sqrt": "std r17 t=none", "eps_omitted": "std r17 t=none", "div255": "std r17 t=none",
    "padd_clamp": "std r17 t=bf16 padd3", "s_out_is_x": "mix r5 t=bf16", "y16_trunc": "mix r17 t=f32",
    "no_s1": ("std r125", "ws"), "no_s2": ("std r125", "ws"), "dgamma_from_dg": ("std r125", "ws"),
    "gy16_ignored": (f"std r{SUBSET_ROWS} gy32+gy16 -> ds32", "ws"), "gy_plus_not_in_params": (f"std r{SUBSET_ROWS} gy32+gy_plus -> ds32", "det"),
    "reduce_skips_last_block": ("mix r132", "ws"), "short_block_skips_last_row": ("mix r5", "atomic"), "amax_before_rstd": ("big r125", "ws"),
}
# ... and the faults that drop or move rows also fail the exact problem of these rows
EXACT_FAULTS = {"gy16_ignored": 124, "gy_plus_not_in_params": 5, "reduce_skips_last_block": 900, "short_block_skips_last_row": 4097,
                "dgamma_from_dg": 4, "no_s1": 1, "no_s2": 1}


def emulate_forward(pb, fault=None, want=("s_out", "y32", "y16", "y_plus")):
    assert fault is None or fault in FAULTS
    out = fwd_buffers(pb, want)
    rows, n = pb.rows, pb.rows * C
    x = pb.x_buf[:n].view(rows, C)
    s = x if pb.t is None else x + pb.t_buf[:n].view(rows, C).float()
    inv = torch.tensor(1.0 / 256.0, dtype=F32)
    mu = s.sum(1) * inv
    d = s - mu[:, None]
    if fault == "one_pass_var":
        var = ((s * s).sum(1) * inv - mu * mu).clamp(min=0)
    else:
        var = (d * d).sum(1) * (torch.tensor(1.0 / 255.0, dtype=F32) if fault == "div255" else inv)
    eps = torch.tensor(pb.eps, dtype=F32)
    rs = 1.0 / (torch.sqrt(var) + eps) if fault == "eps_after_sqrt" else 1.0 / torch.sqrt(var if fault == "eps_omitted" else var + eps)
    y = d * rs[:, None] * pb.gamma + pb.beta
    out.mean[:rows], out.rstd[:rows] = mu, rs
    if out.s_out is not None:
        out.s_out[:n] = (x if fault == "s_out_is_x" else s).reshape(-1)
    if out.y32 is not None:
        out.y32[:n] = y.reshape(-1)
    if out.y16 is not None:
        y16 = (y.view(torch.int32) & -65536).view(F32).to(BF16) if fault == "y16_trunc" else y.to(BF16)
        out.y16[:n] = y16.reshape(-1)
    if out.y_plus is not None:
        i = torch.arange(rows)
        i = i.clamp(max=pb.padd_rows - 1) if fault == "padd_clamp" else i % pb.padd_rows
        out.y_plus[:n] = (y + pb.padd_buf[:pb.padd_rows * C].view(-1, C)[i]).reshape(-1)
    return out


def emulate_lin(pb):
    """the row chain: the projection in fp32, rounded to bf16, then the forward above on x and that t"""
    q = SimpleNamespace(**vars(pb))
    q.t = (pb.a.float() @ pb.w.float().t() + pb.b.float()).to(BF16)
    q.t_buf = inbuf(q.t)
    return emulate_forward(q, want=("s_out", "y32", "y16"))


def emulate_backward(pb, form, fault=None, amax=False):
    assert fault is None or fault in FAULTS
    out = bwd_buffers(pb, form)
    rows, n = pb.rows, pb.rows * C
    view = lambda b: b[:n].view(rows, C).float()                                          # noqa: E731
    s, mu, rs = view(pb.s_buf), pb.mean_buf[:rows, None], pb.rstd_buf[:rows, None]
    parts = [(k, view(b)) for k, b in (("gy32", pb.gy32_buf), ("gy16", pb.gy16_buf), ("gy_plus", pb.gyp_buf)) if b is not None]
    g = gp = None
    for key, p in parts:
        if not (fault == "gy16_ignored" and key == "gy16" and len(parts) > 1):
            g = p if g is None else g + p
            if not (fault == "gy_plus_not_in_params" and key == "gy_plus"):
                gp = p if gp is None else gp + p
    xh = (s - mu) * rs
    dg = g * pb.gamma
    inv = torch.tensor(1.0 / 256.0, dtype=F32)
    s1 = torch.zeros(rows, 1) if fault == "no_s1" else dg.sum(1, keepdim=True) * inv
    s2 = torch.zeros(rows, 1) if fault == "no_s2" else (dg * xh).sum(1, keepdim=True) * inv
    inner = dg - s1 - xh * s2
    o = rs * inner
    if out.ds32 is not None:
        out.ds32[:n] = o.reshape(-1)
    if out.ds16 is not None:
        out.ds16[:n] = o.to(BF16).reshape(-1)
    if amax:
        out.ds_amax = float((inner if fault == "amax_before_rstd" else o).abs().max())
    tg, tb = (dg if fault == "dgamma_from_dg" else gp) * xh, gp
    if fault == "short_block_skips_last_row" and rows % pb.rpb:
        tg, tb, rows = tg[:-1], tb[:-1], rows - 1
    fill = pb.blocks * pb.rpb - rows
    block = lambda v: torch.cat([v, torch.zeros(fill, C)]).view(pb.blocks, pb.rpb, C).sum(1)   # noqa: E731
    pg, pbt = block(tg), block(tb)
    if fault == "reduce_skips_last_block" and pb.blocks > 1:
        pg, pbt = pg[:-1], pbt[:-1]
    out.dgamma[:C], out.dbeta[:C] = pg.sum(0), pbt.sum(0)
    return out


@functools.lru_cache(maxsize=8)
def bwd_case(name):
    pb = bwd_problem(name)
    return pb, bwd_reference(pb)


@functools.lru_cache(maxsize=4)
def exact_case(rows):
    pb = exact_problem(rows)
    return pb, bwd_reference(pb)
