"""CPU: tests/_conv3x3_cases.py checks itself, and the library refuses 3x3 convolutions its 32-bit offsets cannot address.

  definition   the nine shifted sums equal F.conv2d and its autograd in fp64 (forward, input gradient, weight and bias gradient;
               per-split weight gradients sum to the whole)
  tables       every row reaches the branch it is tagged with, derived from the same cdiv rules as the host layer
  mutants      the per-element bound at the chosen K accepts the plane model of the kernels and rejects five single faults
  size check   mpf_gemm3_conv3x3(_h2) return MPF_E_TOO_LARGE for n*H*W*Cin >= 2^31 or n*H*W*Cout >= 2^31
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _conv3x3_cases as CC

F64 = torch.float64


# ---- definition -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(2, 5, 7, 8, 12), (3, 1, 6, 4, 4), (2, 4, 1, 8, 4)], ids=lambda c: "x".join(map(str, c)))
def test_definition_equals_conv2d_and_autograd(case):
    n, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(n, H, W, Cin, generator=g, dtype=F64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=F64)
    b = torch.randn(Cout, generator=g, dtype=F64)
    gy = torch.randn(n, H, W, Cout, generator=g, dtype=F64)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x.permute(0, 3, 1, 2), w, b))
    yr = F.conv2d(xr, wr, br, 1, 1)
    yr.backward(gy.permute(0, 3, 1, 2))
    w2 = w.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin)              # W2[co][(ky*3+kx)*Cin + ci]
    w2t = w.permute(1, 2, 3, 0).reshape(Cin, 9 * Cout)             # W2t[ci][(ky*3+kx)*Cout + co]

    def close(a, ref):
        assert float((a - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    close(CC.conv_ref(x, w2, b, 0), yr.detach().permute(0, 2, 3, 1))
    close(CC.conv_ref(gy, w2t, None, 1), xr.grad.permute(0, 2, 3, 1))
    for rps in (n * H * W, 4, 7):
        c, cs = CC.wgrad_ref(gy, x, rps)
        assert c.shape[0] == CC.cdiv(n * H * W, rps)
        close(c.sum(0).view(Cout, 3, 3, Cin).permute(0, 3, 1, 2), wr.grad)
        close(cs.sum(0), br.grad)
    # the kernels' formulation (flat row + shift, clamped, validity of the output row's own coordinates) is the same function
    for tr in (0, 1):
        flat = sum(CC._gather(x, -1 if tr else 1, t) @ w2[:, t * Cin:(t + 1) * Cin].T for t in range(9))
        close(flat.view(n, H, W, Cout), CC.conv_ref(x, w2, None, tr))


def test_probe_expected_is_the_definition_on_a_one_hot_image():
    n, H, W, Cin, Cout = 3, 4, 5, 2, 3
    w2 = (1.0 + torch.arange(9, dtype=F64)).repeat_interleave(Cin).repeat(Cout, 1)
    for tr in (0, 1):
        for p in CC.probe_pixels(n, H, W):
            x = torch.zeros(n, H, W, Cin, dtype=F64)
            x[p[0], p[1], p[2], 1] = 1.0
            y = CC.conv_ref(x, w2, None, tr)
            e = CC.probe_expected(n, H, W, p, tr)
            assert torch.equal(y, e[..., None].expand_as(y))
            assert int((e != 0).sum()) == int(CC.neighbourhood(n, H, W, p).sum())
            assert torch.equal(e != 0, CC.neighbourhood(n, H, W, p))


# ---- tables ---------------------------------------------------------------------------------------------------------------------
def test_conv_table_reaches_what_it_claims():
    seen = {CC.conv_id(r, c) for r, c, _ in CC.CONV_CASES}
    assert len(seen) == len(CC.CONV_CASES) == 14
    geo = {CC.conv_id(r, c): CC.conv_geometry(r, c) for r, c, _ in CC.CONV_CASES}
    for route, case, supported in CC.CONV_CASES:
        n, H, W, Cin, Cout = case
        assert Cin % 32 == 0 and Cout % 4 == 0
        assert CC.python_supported_shape(case) == supported, case
        assert CC.expected_two_pass(route, case, 0 if route == "tile128_forced" else 256) == (route in ("two_pass", "h2")), case
        if route in ("two_pass", "h2", "tile128_forced"):
            assert Cout % 256 == 0
    g = geo["tile128-1x5x12x32x96"]
    assert g["M"] == 60 and g["tiles_m"] == 1 and g["tiles_n"] == 1 and 96 % 128 != 0          # one partial tile, column tail
    g = geo["tile128-2x9x7x64x64"]
    assert g["M"] == 126 and g["tiles_m"] == 1 and 0 < 9 * 7 < 126                              # image boundary inside the tile
    g = geo["tile128-3x7x9x32x160"]
    assert g["M"] == 189 and g["tiles_m"] == 2 and g["tiles_n"] == 2 and 160 - 128 == 32
    assert 128 % 9 != 0 and 128 // (7 * 9) == 2                                                 # row 128 is not a row start; it is in image 3
    assert geo["tile128-1x4x4x32x36"]["tiles_n"] == 1 and 36 % 4 == 0 and 36 % 32 != 0
    assert min(c[0] * c[1] * c[2] for _, c, s in CC.CONV_CASES if s) == 12                       # (3, 2, 2) is the smallest admitted
    for c in ((1, 1, 16, 32, 32), (1, 16, 1, 32, 32), (4, 1, 1, 32, 32), (1, 1, 8, 32, 256)):
        assert not CC.python_supported_shape(c)
    assert geo["tile128_forced-1x5x8x32x256"]["tiles_n"] == 2 and geo["two_pass-1x5x8x32x256"]["tiles_n"] == 1
    g = geo["two_pass-2x9x15x64x512"]
    assert g["M"] == 270 and g["tiles_m"] == 3 and g["tiles_n"] == 2 and 128 % 15 != 0 and 256 % 15 != 0
    assert geo["h2-1x6x8x256x256"]["nk"] == 72 and geo["h2-2x9x7x32x256"]["M"] == 126
    # the isolation shapes: a middle image with neighbours on both sides, the tile boundary inside it
    for route, case in CC.ISOLATION:
        n, H, W = case[:3]
        assert n == 3 and H * W < 128 < 2 * H * W and CC.conv_geometry(route, case)["tiles_m"] == 3
        assert all(p[0] == 1 for p in CC.poison_pixels(n, H, W))


def test_wgrad_table_reaches_what_it_claims():
    geo = {}
    for route, case, _ in CC.WGRAD_RUNS:
        n, H, W, Cin, Cout, rps = case
        assert W % 8 == 0 and Cin % 128 == 0 and rps % 32 == 0
        if route in ("nt256_h2", "nt128_h2_forced"):
            assert Cin % 256 == 0 and Cout % 256 == 0
        else:
            assert Cin % 256 != 0 or Cout % 256 != 0            # the h2 entry stays on 128-row tiles
        geo[(route, case)] = CC.wgrad_geometry(route, case)
    assert len(CC.WGRAD_RUNS) == 2 * 6 * 2 + 2 * 2 * 2
    g = geo[("nt128", (1, 8, 8, 128, 64, 32))]
    assert g["ns"] == 2 and 32 % 8 == 0 and g["last_rows"] == 32                 # splits aligned to image rows
    g = geo[("nt128", (2, 5, 8, 128, 96, 32))]
    assert g["R"] == 80 and g["ns"] == 3 and g["last_rows"] == 16 and 32 < 40 < 64 and 32 % 40 != 0
    g = geo[("nt128", (3, 3, 8, 128, 200, 64))]
    assert g["tiles_m"] == 2 and 200 - 128 == 72 and g["R"] == 72 and g["ns"] == 2 and g["last_rows"] == 8 and 64 % 24 != 0
    g = geo[("nt128", (3, 3, 8, 128, 64, 128))]
    assert g["ns"] == 1 and g["last_rows"] == 72 and 72 % 32 != 0                # one split that ends in the tail path
    assert geo[("nt128", (2, 1, 8, 128, 32, 32))]["R"] == 16                     # H = 1: a split shorter than one K step
    assert geo[("nt128", (1, 4, 24, 128, 32, 32))]["ns"] == 3 and 32 % 24 != 0   # split boundary inside an image row
    g = geo[("nt256_h2", (2, 5, 8, 256, 512, 32))]
    assert g["tiles_m"] == 2 and g["tiles_n"] == 9 and g["last_rows"] == 16
    assert geo[("nt128_h2_forced", (2, 5, 8, 256, 512, 32))]["tiles_m"] == 4


# ---- mutants --------------------------------------------------------------------------------------------------------------------
FORMS = ("bf16x3", "fp16x2")
MUT_CASE = (2, 5, 6, 32, 16)


@pytest.fixture(scope="module")
def conv_problem():
    x, w2, b = CC.conv_inputs(MUT_CASE, seed=11)
    out = {}
    for tr in (0, 1):
        bias = None if tr else b
        out[tr] = (bias, CC.conv_ref(x, w2, bias, tr), CC.conv_scale(x, w2, bias, tr))
    return x, w2, out


@pytest.mark.parametrize("form", FORMS)
def test_bound_accepts_the_plane_model(conv_problem, form):
    x, w2, out = conv_problem
    for tr in (0, 1):
        bias, ref, S = out[tr]
        r = CC.worst(CC.model_conv(x, w2, bias, tr, form), ref, S)
        print(form, tr, "model err / (u S)", r)
        assert r <= CC.K[form]
    # the lowest-plane fault sits where the issue places it: near 2^-17 S, above the cap on K
    bias, ref, S = out[0]
    r = CC.worst(CC.model_conv(x, w2, bias, 0, form, kept=CC.KEPT_DROPPED[form]), ref, S)
    print(form, "dropped plane err / (u S)", r)
    assert r > CC.K_CAP


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("fault", ["taps_swapped", "wrong_row", "sign_kept", "plane_dropped"])
def test_bound_rejects_conv_faults(conv_problem, form, fault):
    x, w2, out = conv_problem
    tr = 1 if fault == "sign_kept" else 0
    bias, ref, S = out[tr]
    kw = {"taps_swapped": dict(swap=(1, 7)), "wrong_row": dict(wrong_row=True), "sign_kept": dict(keep_sign=True),
          "plane_dropped": dict(kept=CC.KEPT_DROPPED[form])}[fault]
    got = CC.model_conv(x, w2, bias, tr, form, **kw)
    assert not CC.within(got, ref, S, CC.K[form])
    if fault == "wrong_row":                # the fault is local: only the last column of rows that have a next row is off
        bad = ((got - ref).abs() > CC.K[form] * CC.U * S).any(-1)
        assert bad[:, :, :-1].sum() == 0 and bad[:, :, -1].any()


@pytest.mark.parametrize("form", FORMS)
def test_bound_on_the_weight_gradient_model_and_its_faults(form):
    case = (2, 3, 8, 8, 12, 32)
    dy, x = CC.wgrad_inputs(case, seed=5)
    ref, _ = CC.wgrad_ref(dy, x, 32)
    S, _ = CC.wgrad_scale(dy, x, 32)
    k = CC.K[form + "_wgrad"]
    assert ref.shape[0] == 2 and CC.worst(CC.model_wgrad(dy, x, 32, form), ref, S) <= k
    assert not CC.within(CC.model_wgrad(dy, x, 32, form, late=1), ref, S, k)                     # a split that starts one row late
    assert not CC.within(CC.model_wgrad(dy, x, 32, form, kept=CC.KEPT_DROPPED[form]), ref, S, k)
    # and rows of the wrong split: the per-split check sees what the sum over splits cannot
    m = CC.wgrad_ref(dy, x, 16)[0]                                  # rows [16, 32) counted in the second split
    moved = torch.stack([m[0], m[1] + m[2]])
    assert not CC.within(moved, ref, S, k) and torch.allclose(moved.sum(0), ref.sum(0), rtol=1e-12, atol=1e-12)


def test_split_models_are_exact_on_small_integers():
    """the premise of the exact-tap tests: integer operands survive both splits unchanged"""
    x = CC.int_operand((64,), 3, 8)
    h, m, l = CC.split8(x)
    assert torch.equal(h, x) and not m.any() and not l.any()
    for v in (x, 1.0 + torch.arange(9.0)):
        sc = CC.h2_scale(v.abs().max())
        hh, ll = CC.split8h(v, sc)
        assert 2 ** 14 <= float(v.abs().max()) * sc < 2 ** 15 and torch.equal(hh / sc, v) and not ll.any()
    # and the three pieces of a random value add up to it within 2^-24
    r = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    h, m, l = CC.split8(r)
    assert float(((h.double() + m.double() + l.double()) - r.double()).abs().div(r.abs().double()).max()) <= 2.0 ** -23


# ---- size check -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib


def test_conv3x3_refuses_what_32_bit_offsets_cannot_address(built):
    lib = built.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: argument validation happens first
    E_SHAPE, E_NULL, E_TOO_LARGE = -2, -3, -4

    def conv(n, H, W, Cin, Cout, tr=0):
        return lib.mpf_gemm3_conv3x3(one, one, None, one, n, H, W, Cin, Cout, tr, None)

    def conv_h2(n, H, W, Cin, Cout, tr=0):
        return lib.mpf_gemm3_conv3x3_h2(one, one, one, one, None, one, None, n, H, W, Cin, Cout, tr, None)
    too_large = [(1, 8192, 8192, 32, 32),          # n*H*W*Cin = 2^31 exactly
                 (4, 2048, 2048, 128, 32),         # = 2^31 through the channel count
                 (1, 2048, 2048, 512, 256),        # n*H*W*Cin = 2^31 with n*H*W*Cout = 2^30
                 (1, 4096, 4096, 32, 256),         # n*H*W*Cout = 2^32 with n*H*W*Cin = 2^29
                 (2, 2048, 2048, 32, 256),         # n*H*W*Cout = 2^31 exactly
                 (1, 32768, 32768, 32, 256)]       # n*H*W = 2^30 (what the earlier row-count check caught)
    for n, H, W, Cin, Cout in too_large:
        assert n * H * W * max(Cin, Cout) >= 2 ** 31
        for tr in (0, 1):
            assert conv(n, H, W, Cin, Cout, tr) == E_TOO_LARGE, (n, H, W, Cin, Cout)
            assert b"too large" in lib.mpf_last_error()
            if Cout % 256 == 0:
                assert conv_h2(n, H, W, Cin, Cout, tr) == E_TOO_LARGE, (n, H, W, Cin, Cout)
    # the ordinary shape errors stay, and come first
    assert conv(1, 8192, 8192, 48, 32) == E_SHAPE and conv(1, 8, 8, 32, 30) == E_SHAPE and conv(0, 8, 8, 32, 32) == E_SHAPE
    assert conv_h2(1, 8192, 8192, 32, 128) == E_SHAPE and b"256" in lib.mpf_last_error()
    assert lib.mpf_gemm3_conv3x3(None, one, None, one, 1, 8192, 8192, 32, 32, 0, None) == E_NULL
    assert lib.mpf_gemm3_conv3x3_h2(one, None, one, one, None, one, None, 1, 8192, 8192, 32, 256, 0, None) == E_NULL
