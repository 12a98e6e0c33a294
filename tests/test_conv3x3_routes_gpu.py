"""GPU: the 3x3 convolution kernels (csrc/gemm3.hip gemm3_conv_kernel, gemm3_tn2_kernel<128, true(, true)>, gemm3_nt_kernel<conv3x3 ..>,
gemm3_nt2.h) against the fp64 definition of tests/_conv3x3_cases.py, per element, through the C ABI on every route of that file's
tables, and through conv3x3() / autograd.  tests/test_conv3x3_cases_cpu.py holds the definition to F.conv2d, the tables to the
branches they name and the bound to five single faults.

  parity      |got - ref| <= K 2^-24 S per element (S = the same sum over magnitudes): forward and input gradient on every row of
              CONV_RUNS; weight gradient per split (before the reduction), its column sums, and once after mpf_gemm3_nt_reduce
              (bound (K + splits - 1) 2^-24 sum_s S_s: the reduction adds splits - 1 roundings of partial sums that S bounds)
  exact taps  integer operands (|x| <= 8, |w| <= 4, integer bias): every plane split is exact and every sum below 2^24, so all
              results equal the fp64 ones bit for bit; one-hot images with w[tap] = 1 + tap put each tap index at its one place
  isolation   one NaN pixel makes exactly its 3x3 neighbourhood inside its image non-finite (the weight gradient: exactly the taps
              and splits that read it); every other output keeps the bits of the clean run
  out_amax    the slot of the fp16 x 2 entry bounds max |y| within one fp32 rounding
  python      conv3x3() forward + backward per element, with channel-last and NCHW-contiguous upstream gradients, on the
              256 x 256 native, bf16 x 3 native and aten weight-gradient paths
Every comparison prints its worst |err| / (2^-24 S) (`pytest -s`).

Largest |err| / (2^-24 S) per route against the fp64 definition (one MI355X run, every case of the tables, all passing), and the K
derived from it: 4 x the maximum of a form, rounded up to a power of two (the maximum over ~1e5 rounding errors moves with the
seed); the cap is 32.  Nothing is asserted about these figures beyond <= K.
  form and direction        route                                    cases  max     4 x max -> K
  bf16 x 3, fwd / dgrad     gemm3_conv_kernel 128 x 128               16    5.760
                            the same with gemm3_two_pass = 0            2    3.979
                            two-pass gemm3_tn2_kernel<128, true>        4    7.806
                            conv3x3() y, dx (2 shapes)                  8    4.830   31.2 -> 32
  fp16 x 2, fwd / dgrad     gemm3_conv_kernel<h2>                       6    3.968
                            conv3x3() y, dx (2 shapes)                  8    4.615   18.5 -> 32
  bf16 x 3, weight grad     gemm3_nt_kernel<conv3x3>, per split        12    4.586
                            after mpf_gemm3_nt_reduce                  12    4.099
                            conv3x3() dw                                2    4.936   19.7 -> 32
  fp16 x 2, weight grad     gemm3_nt_kernel<conv3x3 h2>, per split     12    4.981
                            <conv3x3 h2 256x256>, per split             4    5.526
                            <conv3x3 h2> with gemm3_nt2 = 0             4    5.526
                            after mpf_gemm3_nt_reduce                  20    2.943
                            conv3x3() dw                                4    3.921   22.1 -> 32
  column sums of dy         per split (bound: rows of the split)       14    1.789
                            reduced (bound: rows + splits - 1)         14    1.544
  aten fallback dw          bound R = 126                               2    1.642
The plane model of the CPU module (products in fp64) sits at 0.5 .. 0.8 on its case, so what is measured here is mostly the fp32
accumulation of the MFMA chain over 9 Cin / 32 steps; the lowest-plane fault sits at 153 (bf16 x 3) and 2837 (fp16 x 2).
On the kernels as they were before the taps were selected instead of multiplied by 0, the six forward / input-gradient isolation
tests fail (NaN pixel (1, 4, 0) of a 3 x 9 x 11 image also poisons (1, 2, 10), (1, 3, 10), (1, 4, 10), the pixels whose dx = +1
neighbour wraps onto it); the three weight-gradient ones pass, as do all 138 other tests: no other fault was found.
"""
import contextlib

import pytest
import torch

import _conv3x3_cases as CC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F64 = torch.float64
NAN = float("nan")


@contextlib.contextmanager
def _options(opts):
    from mp_former_amd import _lib
    try:
        for k, v in opts.items():
            _lib.set_option(k, v)
        yield
    finally:
        for k in opts:
            _lib.set_option(k, CC.OPTION_DEFAULTS[k])


@contextlib.contextmanager
def _one_record(kernel):
    """the launch log around one entry point: exactly one record, under the kernel's name, which is also mpf_last_kernel()"""
    from mp_former_amd import _lib
    _lib.profile_enable(True)
    try:
        yield
        torch.cuda.synchronize()
        assert _lib.last_kernel() == kernel, _lib.last_kernel()
        assert _lib.profile_get("")[0] == 1 and _lib.profile_get(kernel)[0] == 1
        if "<" not in kernel:
            assert _lib.profile_get(kernel + "<")[0] == 0
    finally:
        _lib.profile_enable(False)


def _weight_operand(route, w2):
    """-> (planes, amax slot or None) of W2 [Cout, 9 Cin] on the device"""
    from mp_former_amd.gemm3 import split_weights_grouped, split_weights_grouped_h2
    w2d = w2.to(DEV).contiguous()
    if CC.ROUTES[route]["form"] == "fp16x2":
        return split_weights_grouped_h2([([w2d], False)])[0]
    return split_weights_grouped([([w2d], False)])[0], None


def _conv(route, case, x, wop, bias, tr, x_amax=None, out_amax=None):
    """one launch through the C ABI into a NaN-filled buffer -> y [n, H, W, Cout] on the CPU"""
    from mp_former_amd import _lib
    from mp_former_amd.gemm3 import amax
    n, H, W, Cin, Cout = case
    r = CC.ROUTES[route]
    xd = x.to(DEV).contiguous()
    bd = None if bias is None else bias.to(DEV)
    y = torch.full((n, H, W, Cout), NAN, dtype=torch.float32, device=DEV)
    planes, w_am = wop
    st = _lib.stream_ptr(DEV)
    with _options(r["opts"]):
        if r["form"] == "fp16x2":
            x_am = amax(xd) if x_amax is None else x_amax
            with _one_record(r["kernel"]):
                _lib.call(r["entry"], DEV, xd.data_ptr(), x_am.data_ptr(), planes.data_ptr(), w_am.data_ptr(), _lib.ptr(bd), y.data_ptr(),
                          _lib.ptr(out_amax), n, H, W, Cin, Cout, tr, st)
        else:
            with _one_record(r["kernel"]):
                _lib.call(r["entry"], DEV, xd.data_ptr(), planes.data_ptr(), _lib.ptr(bd), y.data_ptr(), n, H, W, Cin, Cout, tr, st)
    return y.cpu()


def _wgrad(route, case, dy, x, csum, x_amax=None):
    """-> (c_part [ns, Cout, 9 Cin], csum_dy [ns, Cout] or None) on the device, written into NaN-filled buffers"""
    from mp_former_amd import _lib
    from mp_former_amd.gemm3 import amax
    n, H, W, Cin, Cout, rps = case
    r = CC.WGRAD_ROUTES[route]
    ns = CC.cdiv(n * H * W, rps)
    dyd, xd = dy.to(DEV).contiguous(), x.to(DEV).contiguous()
    c = torch.full((ns, Cout, 9 * Cin), NAN, dtype=torch.float32, device=DEV)
    ca = torch.full((ns, Cout), NAN, dtype=torch.float32, device=DEV) if csum else None
    st = _lib.stream_ptr(DEV)
    with _options(r["opts"]):
        if r["form"] == "fp16x2":
            dy_am, x_am = amax(dyd), (amax(xd) if x_amax is None else x_amax)
            with _one_record(r["kernel"]):
                _lib.call(r["entry"], DEV, dyd.data_ptr(), dy_am.data_ptr(), xd.data_ptr(), x_am.data_ptr(), c.data_ptr(), _lib.ptr(ca),
                          n, H, W, Cin, Cout, rps, st)
        else:
            with _one_record(r["kernel"]):
                _lib.call(r["entry"], DEV, dyd.data_ptr(), xd.data_ptr(), c.data_ptr(), _lib.ptr(ca), n, H, W, Cin, Cout, rps, st)
    return c, ca


def _seed(*key):
    return sum((i + 1) * int(v) for i, v in enumerate(key)) % 100003


def _report(tag, name, ratio, k):
    print(f"RATIO {tag:<18} {name:<44} {ratio:8.3f}  (K = {k})")
    assert ratio <= k, f"{name}: |err| / (2^-24 S) = {ratio} > K = {k}"


# ---- forward and input gradient -------------------------------------------------------------------------------------------------
CONV_IDS = [CC.conv_id(*r) for r in CC.CONV_RUNS]


@pytest.mark.parametrize("route,case,tr", CC.CONV_RUNS, ids=CONV_IDS)
def test_conv_parity_per_element(route, case, tr):
    from mp_former_amd.conv3x3 import supported
    n, H, W, Cin, Cout = case
    x, w2, b = CC.conv_inputs(case, seed=_seed(*case, tr))
    bias = None if tr else b
    if not tr:          # what the python gate says about the shape (the C ABI takes all of them)
        admits = dict((CC.conv_id(r, c), s) for r, c, s in CC.CONV_CASES)[CC.conv_id(route, case)]
        xv = x.to(DEV).permute(0, 3, 1, 2)
        assert supported(xv, torch.empty(Cout, Cin, 3, 3, device=DEV)) == admits
    y = _conv(route, case, x, _weight_operand(route, w2), bias, tr)
    form = CC.ROUTES[route]["form"]
    _report(route, CC.conv_id(route, case, tr), CC.worst(y, CC.conv_ref(x, w2, bias, tr), CC.conv_scale(x, w2, bias, tr)), CC.K[form])


@pytest.mark.parametrize("route,case,tr", CC.CONV_RUNS, ids=CONV_IDS)
def test_conv_exact_on_integers(route, case, tr):
    x, w2, b = CC.conv_inputs(case, seed=_seed(*case, tr, 7), integer=True)
    bias = None if tr else b
    ref = CC.conv_ref(x, w2, bias, tr)
    assert float(ref.abs().max()) < 2 ** 24 and float(CC.conv_scale(x, w2, bias, tr).max()) < 2 ** 24
    y = _conv(route, case, x, _weight_operand(route, w2), bias, tr)
    bad = (y.to(F64) != ref).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements differ, first (i, y, x, co) = {bad[0].tolist()}"


PROBE_CASES = [("tile128", (3, 7, 9, 32, 160)), ("two_pass", (3, 9, 15, 32, 256)), ("h2", (3, 9, 7, 32, 256)),
               ("tile128", (1, 1, 16, 32, 32)), ("tile128", (1, 16, 1, 32, 32)), ("tile128", (4, 1, 1, 32, 32)), ("h2", (1, 1, 8, 32, 256))]


@pytest.mark.parametrize("route,case", PROBE_CASES, ids=[CC.conv_id(*c) for c in PROBE_CASES])
def test_one_hot_probes_put_every_tap_in_its_place(route, case):
    n, H, W, Cin, Cout = case
    w2 = (1.0 + torch.arange(9.0)).repeat_interleave(Cin).repeat(Cout, 1)          # w[co][ci][ky][kx] = 1 + ky * 3 + kx
    wop = _weight_operand(route, w2)
    for tr in (0, 1):
        for p in CC.probe_pixels(n, H, W):
            x = torch.zeros(n, H, W, Cin)
            x[p[0], p[1], p[2], Cin // 2] = 1.0
            y = _conv(route, case, x, wop, None, tr)
            e = CC.probe_expected(n, H, W, p, tr)
            assert torch.equal(y.to(F64), e[..., None].expand(n, H, W, Cout)), \
                f"pixel {p} transposed {tr}: got taps\n{y[..., 0]}\nwant\n{e}"


def _pixels(mask):
    return [tuple(v) for v in mask.nonzero().tolist()]


@pytest.mark.parametrize("tr", (0, 1), ids=("F", "T"))
@pytest.mark.parametrize("route,case", CC.ISOLATION, ids=[CC.conv_id(*c) for c in CC.ISOLATION])
def test_a_nan_pixel_reaches_its_neighbourhood_only(route, case, tr):
    from mp_former_amd.gemm3 import amax
    n, H, W, Cin, Cout = case
    x, w2, b = CC.conv_inputs(case, seed=_seed(*case, tr, 3))
    bias = None if tr else b
    wop = _weight_operand(route, w2)
    x_am = amax(x.to(DEV).contiguous()) if CC.ROUTES[route]["form"] == "fp16x2" else None          # from the finite values
    clean = _conv(route, case, x, wop, bias, tr, x_amax=x_am)
    assert torch.isfinite(clean).all()
    for p in CC.poison_pixels(n, H, W):
        xp = x.clone()
        xp[p[0], p[1], p[2], :] = NAN
        got = _conv(route, case, xp, wop, bias, tr, x_amax=x_am)
        nb = CC.neighbourhood(n, H, W, p)
        bad = ~torch.isfinite(got)
        assert bad.all(-1)[nb].all(), f"NaN pixel {p}: finite outputs inside its neighbourhood"
        leaked = bad.any(-1) & ~nb
        assert not leaked.any(), f"NaN pixel {p} (image, y, x) poisons outputs outside its 3x3 neighbourhood: {_pixels(leaked)}"
        assert torch.equal(got.view(torch.int32)[~nb], clean.view(torch.int32)[~nb]), f"NaN pixel {p}: bits changed elsewhere"


H2_CASES = [c for r, c, _ in CC.CONV_CASES if r == "h2"]


@pytest.mark.parametrize("case", H2_CASES, ids=["x".join(map(str, c)) for c in H2_CASES])
def test_out_amax_bounds_the_result(case):
    from mp_former_amd.gemm3 import AMAX_SLOT, amax_value
    for tr in (0, 1):
        x, w2, b = CC.conv_inputs(case, seed=_seed(*case, tr, 5))
        slot = torch.zeros(AMAX_SLOT, dtype=torch.float32, device=DEV)
        y = _conv("h2", case, x, _weight_operand("h2", w2), None if tr else b, tr, out_amax=slot)
        got, true = float(amax_value(slot)), float(y.abs().max())
        assert true <= got <= true * (1.0 + 2.0 ** -23), (got, true)


# ---- weight and bias gradient ---------------------------------------------------------------------------------------------------
WGRAD_IDS = [CC.wgrad_id(*r) for r in CC.WGRAD_RUNS]
_wgrad_refs = {}


def _wgrad_reference(case, integer):
    """(dy, x, per-split dW2, per-split db, their magnitude sums), computed once per case and shared"""
    key = (case, integer)
    if key not in _wgrad_refs:
        dy, x = CC.wgrad_inputs(case, seed=_seed(*case, 9), integer=integer)
        _wgrad_refs[key] = (dy, x) + CC.wgrad_ref(dy, x, case[5]) + CC.wgrad_scale(dy, x, case[5])
    return _wgrad_refs[key]


@pytest.mark.parametrize("route,case,csum", CC.WGRAD_RUNS, ids=WGRAD_IDS)
def test_wgrad_parity_per_split(route, case, csum):
    from mp_former_amd.gemm3 import nt_reduce
    dy, x, c_ref, cs_ref, S, Ss = _wgrad_reference(case, False)
    c, ca = _wgrad(route, case, dy, x, csum)
    k = CC.K[CC.WGRAD_ROUTES[route]["form"] + "_wgrad"]
    name = CC.wgrad_id(route, case, csum)
    _report(route, name, CC.worst(c.cpu(), c_ref, S), k)
    ns = c.shape[0]
    if csum:
        # column sums of the unscaled fp32 values: rows - 1 additions in any order, within (rows) 2^-24 sum |dy|
        rows = min(case[5], case[0] * case[1] * case[2])
        _report(route + " csum", name, CC.worst(ca.cpu(), cs_ref, Ss), rows)
    tot, tot_s = nt_reduce(c, ca)
    _report(route + " reduced", name, CC.worst(tot.cpu(), c_ref.sum(0), S.sum(0)), k + ns - 1)
    if csum:
        _report(route + " csum red.", name, CC.worst(tot_s.cpu(), cs_ref.sum(0), Ss.sum(0)), rows + ns - 1)


@pytest.mark.parametrize("route,case,csum", CC.WGRAD_RUNS, ids=WGRAD_IDS)
def test_wgrad_exact_on_integers(route, case, csum):
    dy, x, c_ref, cs_ref, S, Ss = _wgrad_reference(case, True)
    assert float(S.max()) < 2 ** 24 and float(Ss.max()) < 2 ** 24
    c, ca = _wgrad(route, case, dy, x, csum)
    bad = (c.cpu().to(F64) != c_ref).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements differ, first (split, co, tap * Cin + ci) = {bad[0].tolist()}"
    if csum:
        assert torch.equal(ca.cpu().to(F64), cs_ref)


@pytest.mark.parametrize("route,case", CC.ISOLATION_WGRAD, ids=[CC.wgrad_id(r, c, False) for r, c in CC.ISOLATION_WGRAD])
def test_a_nan_pixel_reaches_only_the_taps_and_splits_that_read_it(route, case):
    from mp_former_amd.gemm3 import amax
    n, H, W, Cin, Cout, rps = case
    dy, x = CC.wgrad_inputs(case, seed=_seed(*case, 13))
    x_am = amax(x.to(DEV).contiguous()) if CC.WGRAD_ROUTES[route]["form"] == "fp16x2" else None
    clean = _wgrad(route, case, dy, x, False, x_amax=x_am)[0].cpu()
    assert torch.isfinite(clean).all()
    for p in CC.poison_pixels(n, H, W):
        xp = x.clone()
        xp[p[0], p[1], p[2], :] = NAN
        got = _wgrad(route, case, dy, xp, False, x_amax=x_am)[0].cpu()
        want = torch.zeros(got.shape, dtype=torch.bool)
        for t, (ty, tx) in enumerate(CC.TAPS):           # row q reads pixel q + TAPS[t]: q = p - TAPS[t], in the split of q
            qy, qx = p[1] - ty, p[2] - tx
            if 0 <= qy < H and 0 <= qx < W:
                want[((p[0] * H + qy) * W + qx) // rps, :, t * Cin:(t + 1) * Cin] = True
        bad = ~torch.isfinite(got)
        assert torch.equal(bad, want), f"NaN pixel {p}: non-finite (split, tap) = " \
            f"{sorted({(s, k // Cin) for s, _, k in (bad != want).nonzero().tolist()})} differ from the ones that read it"
        assert torch.equal(got.view(torch.int32)[~want], clean.view(torch.int32)[~want])


# ---- python level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gy_layout", ("cl", "nchw"))
@pytest.mark.parametrize("N,C,Co,H,W,wpath", CC.PYTHON_CASES + [(1, 256, 256, 6, 8, "gemm3_nt_kernel<conv3x3 h2 256x256>")])
def test_conv3x3_autograd_per_element(N, C, Co, H, W, wpath, gy_layout, monkeypatch):
    from mp_former_amd import _lib, gemm3
    from mp_former_amd.conv3x3 import conv3x3, supported
    from mp_former_amd.groupnorm import is_cl_plane
    case = (N, H, W, C, Co)
    x, w2, b = CC.conv_inputs(case, seed=_seed(*case, 17))
    gy = CC.random_operand((N, H, W, Co), _seed(*case, 19))
    h2 = C % 256 == 0 and Co % 256 == 0
    form = "fp16x2" if h2 else "bf16x3"
    w = w2.view(Co, 3, 3, C).permute(0, 3, 1, 2).contiguous().to(DEV).requires_grad_(True)
    xv = x.to(DEV).permute(0, 3, 1, 2).requires_grad_(True)
    bd = b.to(DEV).requires_grad_(True)
    assert supported(xv, w)
    y = conv3x3(xv, w, bd)
    assert _lib.last_kernel() == ("gemm3_conv_kernel<h2>" if h2 else "gemm3_conv_kernel") and is_cl_plane(y)
    tag = f"python {N}x{C}x{Co}x{H}x{W} {gy_layout}"
    _report("python y", tag, CC.worst(y.detach().permute(0, 2, 3, 1).cpu(), CC.conv_ref(x, w2, b, 0), CC.conv_scale(x, w2, b, 0)), CC.K[form])
    if gy_layout == "cl":
        g = gy.to(DEV).permute(0, 3, 1, 2)
        assert is_cl_plane(g) or N == 1
    else:
        g = gy.permute(0, 3, 1, 2).contiguous().to(DEV)
        assert g.is_contiguous() and (not is_cl_plane(g) or N == 1)
    splits = []
    real_reduce = gemm3.nt_reduce

    def counting_reduce(c_part, s_part=None):
        splits.append(c_part.shape[0])
        return real_reduce(c_part, s_part)
    monkeypatch.setattr(gemm3, "nt_reduce", counting_reduce)
    _lib.profile_enable(True)
    try:
        dx, dw, db = torch.autograd.grad(y, [xv, w, bd], g)
        torch.cuda.synchronize()
        native = _lib.profile_get("gemm3_nt_kernel")[0]
        if wpath == "aten":
            assert native == 0 and not splits
        else:
            assert native == 1 and _lib.profile_get(wpath)[0] == 1 and len(splits) == 1
        assert _lib.profile_get("gemm3_conv_kernel<h2>" if h2 else "gemm3_conv_kernel")[0] == 1
    finally:
        _lib.profile_enable(False)
    w2t = w2.view(Co, 3, 3, C).permute(3, 1, 2, 0).reshape(C, 9 * Co)            # W2t[ci][(ky*3+kx)*Cout + co]
    _report("python dx", tag, CC.worst(dx.permute(0, 2, 3, 1).cpu(), CC.conv_ref(gy, w2t, None, 1), CC.conv_scale(gy, w2t, None, 1)), CC.K[form])
    R = N * H * W
    c_ref, cs_ref = CC.wgrad_ref(gy, x, R)
    S, Ss = CC.wgrad_scale(gy, x, R)
    dw2 = dw.permute(0, 2, 3, 1).reshape(Co, 9 * C).cpu()
    if wpath == "aten":
        # the library's fp32 convolution backward: R products per element summed in fp32 in an unknown order, within R 2^-24 S
        kw = kb = R
    else:
        # the bias gradient is a plain fp32 sum of R values of gy (per split, then over the splits): within R 2^-24 sum |gy|
        kw, kb = CC.K[form + "_wgrad"] + splits[0] - 1, R
    _report("python dw " + ("aten" if wpath == "aten" else form), tag, CC.worst(dw2, c_ref[0], S[0]), kw)
    _report("python db", tag, CC.worst(db.cpu(), cs_ref[0], Ss[0]), kb)
