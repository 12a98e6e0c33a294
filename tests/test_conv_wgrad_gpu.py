"""mpf_conv_wgrad_bf16_grouped (csrc/gemm3_conv_wgrad.h) against an fp64 CPU reference computed from the same bf16-valued inputs.

The entry computes out = float(bf16_rn(sum_r dY[r][co] X[r'][ci])) * scale[co] with an fp32 accumulator.  Bound per element, from
those rounding points alone: one bf16 rounding of the sum, 2^-8 |ref|, plus the fp32 accumulation of R products,
4 R 2^-24 (|dY|^T |X|), both times |scale|, plus the one fp32 multiply by the scale, 2^-24 |ref scale|."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GEMM, REDUCE = "gemm3_nt_group_kernel<bf16 conv>", "conv_wgrad_reduce_kernel"


@pytest.fixture(scope="module")
def bb():
    from mp_former_amd import backbone
    return backbone


class Case:
    """one item: bf16 operands on the device, its fp64 reference and bound on the CPU (computed once)"""

    def __init__(self, seed, R, Cout, Cin, kind=0, N=1, H=0, W=0, rps=None, layout="kernel"):
        g = torch.Generator().manual_seed(seed)
        self.R, self.Cout, self.Cin, self.kind, self.H, self.W, self.rps, self.layout = R, Cout, Cin, kind, H, W, rps, layout
        dy = torch.randn(R, Cout, generator=g).bfloat16()
        x = torch.randn(R, Cin, generator=g).bfloat16()
        self.scale = (0.5 + torch.arange(Cout, dtype=torch.float32) / Cout + 0.013 * torch.rand(Cout, generator=g)).contiguous()
        assert self.scale.unique().numel() == Cout
        self.dy, self.x = dy.to(DEV), x.to(DEV)
        d, v = dy.double(), x.double()
        if kind == 0:
            assert N == 1
            ref, mag = d.t() @ v, d.abs().t() @ v.abs()
            self.shape = (Cout, Cin, 1, 1)
        else:
            assert R == N * H * W and bool((x != 0).all()) and bool((dy != 0).all())      # borders and the images' last rows included
            img = lambda t, C: t.view(N, H, W, C).permute(0, 3, 1, 2).contiguous()
            bw = lambda a, b: torch.ops.aten.convolution_backward(a, b, torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64), None, [1, 1], [1, 1],
                                                                  [1, 1], False, [0, 0], 1, [False, True, False])[1]
            ref, mag = bw(img(d, Cout), img(v, Cin)), bw(img(d.abs(), Cout), img(v.abs(), Cin))
            self.shape = (Cout, Cin, 3, 3)
        s = self.scale.double().view(-1, *([1] * (ref.dim() - 1)))
        self.ref = (ref * s).reshape(self.shape)
        self.bound = ((2.0 ** -8 * ref.abs() + 4.0 * R * 2.0 ** -24 * mag) * s + 2.0 ** -24 * (ref * s).abs()).reshape(self.shape)

    def strides(self):
        """(view strides of [Cout, Cin, kh, kw], (co, ci, tap) strides of the entry)"""
        Cin, t = self.Cin, self.shape[2] * self.shape[3]
        if self.layout == "kernel":              # k = tap * Cin + ci contiguous: [Cout, Cin, 1, 1], or channels_last [Cout, Cin, 3, 3]
            return (t * Cin, 1, 3 * Cin if t == 9 else 1, Cin if t == 9 else 1), (t * Cin, 1, Cin)
        if self.layout == "contiguous":
            return (t * Cin, t, 3 if t == 9 else 1, 1), (t * Cin, t, 1)
        assert self.layout == "padded" and t == 1         # rows one element longer: no aligned 16-byte stores
        return (Cin + 1, 1, 1, 1), (Cin + 1, 1, 0)


def run_group(bb, cases):
    """-> [out_i as a [Cout, Cin, kh, kw] view]; items with rps = None take the planner's split, the others their own"""
    from mp_former_amd import _lib
    arr = (bb._CwItem * len(cases))()
    for i, c in enumerate(cases):
        arr[i] = bb.conv_wgrad_item(c.R, c.Cout, getattr(c, "claimed_cin", c.Cin), c.kind, c.H, c.W, c.strides()[1])
    if any(c.rps is None for c in cases):
        bb.conv_wgrad_plan(arr, 0, DEV)
    off, outs = 0, []
    scales = [c.scale.to(DEV) for c in cases]
    for it, c, sc in zip(arr, cases, scales):
        if c.rps is not None:
            it.rows_per_split = c.rps
        taps = 9 if c.kind else 1
        it.ws_offset = off
        off += (-(-c.R // it.rows_per_split) * c.Cout * taps * c.Cin * 4 + 255) & ~255
        vs = c.strides()[0]
        buf = torch.full((c.Cout * vs[0] + 4,), float("nan"), device=DEV)
        outs.append(buf.as_strided(c.shape, vs))
        it.dy, it.x, it.scale, it.out = c.dy.data_ptr(), c.x.data_ptr(), sc.data_ptr(), buf.data_ptr()
    ws = torch.empty(off, dtype=torch.uint8, device=DEV)
    _lib.call("mpf_conv_wgrad_bf16_grouped", DEV, arr, len(cases), ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV))
    torch.cuda.synchronize()
    return outs


def check(cases, outs):
    for c, o in zip(cases, outs):
        err = (o.double().cpu() - c.ref).abs()
        worst = float((err / c.bound.clamp_min(1e-300)).max())
        print(f"R {c.R} {c.Cout} x {c.Cin} kind {c.kind} rps {c.rps} {c.layout}: max |err| / bound = {worst:.3f}")
        assert bool(torch.isfinite(o).all())
        assert bool((err <= c.bound).all()), f"R {c.R} {c.Cout} x {c.Cin} kind {c.kind}: {worst:.3f} x the bound"


@pytest.fixture(scope="module")
def group_1x1():
    """items of different R in one group: a single partial split (R = 96 < 128), a tail row step with a short last split
    (1000 = 416 + 416 + 168), the planner's split at 4096; a half-empty column tile, two row tiles, bounds inside a tile"""
    return [Case(1, 96, 64, 64, rps=128), Case(2, 1000, 256, 64, rps=416), Case(3, 4096, 64, 256), Case(4, 1000, 72, 40, rps=416),
            Case(5, 4096, 64, 64), Case(6, 96, 72, 40, rps=32, layout="padded"), Case(7, 4096, 256, 64, rps=1024)]


def test_group_of_1x1_items_with_different_rows(bb, group_1x1):
    from mp_former_amd import _lib
    _lib.profile_enable(True)
    try:
        outs = run_group(bb, group_1x1)
        assert _lib.profile_get(GEMM)[0] == 1 and _lib.profile_get(REDUCE)[0] == 1
        flops = sum(2.0 * c.R * c.Cout * c.Cin for c in group_1x1)
        assert _lib.profile_get_flops(GEMM) == flops and _lib.profile_get(GEMM)[2] > 0
    finally:
        _lib.profile_enable(False)
    check(group_1x1, outs)
    again = run_group(bb, group_1x1)
    assert all(torch.equal(a, b) for a, b in zip(outs, again)), "not bit-reproducible"


def test_thirteen_items_take_two_launches(bb):
    from mp_former_amd import _lib
    cases = [Case(20 + i, 96 + 32 * i, 64 if i % 2 else 72, 64 if i % 3 else 40) for i in range(13)]
    assert _lib.lib().mpf_conv_wgrad_group_max() < 13
    _lib.profile_enable(True)
    try:
        outs = run_group(bb, cases)
        assert _lib.profile_get(GEMM)[0] == 2 and _lib.profile_get(REDUCE)[0] == 2
    finally:
        _lib.profile_enable(False)
    check(cases, outs)


@pytest.fixture(scope="module")
def group_3x3():
    """two images of 8 x 16 and of 16 x 8 (a tap must not read the neighbouring image); 4 x 24 with 32-row splits, whose
    boundaries fall inside an image row; both destination layouts; 1x1 items in the same launch"""
    return [Case(40, 256, 64, 128, 1, 2, 8, 16, layout="kernel"), Case(41, 256, 128, 128, 1, 2, 8, 16, rps=64, layout="contiguous"),
            Case(42, 256, 64, 128, 1, 2, 16, 8, rps=96, layout="contiguous"), Case(43, 256, 128, 128, 1, 2, 16, 8, layout="kernel"),
            Case(44, 96, 64, 128, 1, 1, 4, 24, rps=32, layout="kernel"), Case(45, 1000, 72, 40, rps=416),
            Case(46, 192, 128, 256, 1, 2, 4, 24, rps=32, layout="contiguous")]


def test_group_with_3x3_items(bb, group_3x3):
    outs = run_group(bb, group_3x3)
    check(group_3x3, outs)
    again = run_group(bb, group_3x3)
    assert all(torch.equal(a, b) for a, b in zip(outs, again)), "not bit-reproducible"


def test_split_choice_does_not_move_the_result_beyond_the_bound(bb):
    """one split against many: the same sums in another order"""
    a, b = Case(50, 4096, 64, 128, rps=4096), Case(50, 4096, 64, 128, rps=32)
    outs = run_group(bb, [a, b])
    check([a, b], outs)


def test_ineligible_items_return_the_shape_error(bb):
    from mp_former_amd import _lib
    ok = Case(60, 96, 64, 64, rps=96)
    _lib.profile_enable(True)
    try:
        for bad in (Case(61, 96, 64, 64, rps=48), Case(62, 256, 64, 128, 1, 2, 8, 16, rps=64)):
            if bad.kind:
                bad.claimed_cin = 64    # a 3x3 item whose Cin is no multiple of 128 (checked before anything is read)
            with pytest.raises(RuntimeError, match="mpf_conv_wgrad_bf16_grouped failed with code"):
                run_group(bb, [ok, bad])
        assert _lib.profile_get(GEMM)[0] == 0, "launched in spite of a bad item"
    finally:
        _lib.profile_enable(False)
    arr = (bb._CwItem * 1)(bb.conv_wgrad_item(256, 64, 128, 1, 8, 12))
    plans, ws = (bb._CwPlan * 1)(), ctypes.c_size_t(0)
    assert _lib.lib().mpf_conv_wgrad_plan(arr, 1, 0, plans, ctypes.byref(ws)) != 0
    assert b"W % 8" in _lib.lib().mpf_last_error()
