"""GPU: the GroupNorm kernels (csrc/groupnorm_cl.hip, mpf_group_stats of csrc/elementwise.hip) against the per-element fp64
references of tests/_groupnorm_cases.py on every route that reaches them.  The problems, bounds, mirrors and check functions are that
file's; tests/test_groupnorm_cases_cpu.py holds every table row to the branch it is tagged with, the mirrors to the built library,
aten's own fp32 GroupNorm to the bounds at K = 4, and shows that each of 14 single faults of a torch emulation fails these checks.

  channel-last  every (row, mode) of CL_CASES through the C ABI (mpf_gn_cl_forward / _backward, mpf_upsample2x_cl_backward) into
                sentinel-filled strided buffers with NaN input gaps and a 0xFF workspace of exactly the mirrored size: y, mean, rstd,
                dx, dgamma, dbeta, dtop per element, gaps bit-intact; then through GroupNorm.forward_cl / autograd with the
                upstream gradient as a strided channel-last view and as an NCHW-contiguous tensor (N = 1 among them)
  flatten       group_norm_flatten on 8x16, 43x3, 82x100 (C = 32, G = 8) against the fp64 per-level reference, values and gradients
  NCHW          mpf_group_stats mean / rstd on the NCHW rows (4 .. 3 * 8192 + 12 elements, both large-mean distributions) and
                _GroupNormFn forward + gradients at two of them
  fallback      GroupNorm.forward on C / G = 3, 64, 2 with channels-last and contiguous input: fp64 parity, no gn_cl_ kernel
  determinism   two runs of the 65-chunk production case give the same bits
Every comparison prints its worst err / bound (`pytest -s`).  Bounds (K = 8, u = 2^-24): see tests/_groupnorm_cases.py; the rstd
form kept is K u rstd (1 + |mu| / sigma).  The large-mean rows also hold max|dx - ref| <= 4 x aten's fp32 backward on this device.

Worst err / bound seen per quantity (one MI355X run, all cases passing; nothing is asserted about these beyond <= 1):
  route                              y      mean   rstd   dx     dgamma dbeta  dtop   dx err / aten's (bar 4)
  channel-last, ABI and autograd     0.780  0.308  0.215  0.363  0.355  0.284  0.306  1.17
  group_norm_flatten                 0.516                0.177  0.031  0.047
  mpf_group_stats / _GroupNormFn     0.531  0.307  0.115  0.126  0.016  0.018
  fallback chain                     0.402                0.202  0.099  0.119
At |mu| / sigma = 133 and 6000 rstd is at 0.003 .. 0.008 of its bound and dx at 0.43 .. 1.17 of aten's fp32 backward: the uncentred
fp32 chunk sums of gy * x cost nothing against aten there, so the kernels stay as they are.  K did not move.
No bug was found in csrc/groupnorm_cl.hip, mpf_group_stats or groupnorm.py: all 71 tests passed on the kernels as they were.
"""
import pytest
import torch

import _groupnorm_cases as GC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = torch.float32


def _poison_bytes(n):
    return torch.full((max(int(n), 1),), 0xFF, dtype=torch.uint8, device=DEV)           # NaN as fp32


def _upload(pb):
    d = {"x": pb.x_buf.to(DEV), "gy": pb.gy_buf.to(DEV), "gamma": pb.gamma.to(DEV), "beta": pb.beta.to(DEV)}
    d["top"] = pb.top_buf.to(DEV) if pb.has_top else None
    return d


def _run_abi(pb, d):
    """forward, backward and the top map's adjoint through the C ABI -> the output buffers on the CPU"""
    from mp_former_amd import _lib
    P = GC.make_plane(pb.HW, pb.C, pb.G)
    out = {k: v.to(DEV) for k, v in GC.new_buffers(pb).items()}
    st = _lib.stream_ptr(DEV)
    assert _lib.lib().mpf_gn_cl_workspace_bytes(pb.N, pb.HW, pb.C, pb.G) == max(GC.fwd_ws(pb.N, P), GC.bwd_ws(pb.N, P))
    ws = _poison_bytes(GC.fwd_ws(pb.N, P))
    _lib.call("mpf_gn_cl_forward", DEV, d["x"].data_ptr(), pb.bs["x"], d["gamma"].data_ptr(), d["beta"].data_ptr(), pb.N, pb.HW, pb.C, pb.G,
              pb.eps, int(pb.relu), _lib.ptr(d["top"]), pb.bs["top"] if pb.has_top else 0, pb.W, out["y"].data_ptr(), pb.bs["y"],
              out["mean"].data_ptr(), out["rstd"].data_ptr(), ws.data_ptr(), ws.numel(), st)
    assert _lib.last_kernel() == "gn_cl_apply_kernel", _lib.last_kernel()
    ws = _poison_bytes(GC.bwd_ws(pb.N, P))
    _lib.call("mpf_gn_cl_backward", DEV, d["gy"].data_ptr(), pb.bs["gy"], d["x"].data_ptr(), pb.bs["x"], d["gamma"].data_ptr(), d["beta"].data_ptr(),
              out["mean"].data_ptr(), out["rstd"].data_ptr(), pb.N, pb.HW, pb.C, pb.G, int(pb.relu), out["dx"].data_ptr(), pb.bs["dx"],
              out["dgamma"].data_ptr(), out["dbeta"].data_ptr(), ws.data_ptr(), ws.numel(), st)
    assert _lib.last_kernel() == "gn_cl_bwd_apply_kernel", _lib.last_kernel()
    if pb.has_top:
        _lib.call("mpf_upsample2x_cl_backward", DEV, d["gy"].data_ptr(), pb.bs["gy"], pb.N, pb.Ht, pb.Wt, pb.C, out["dtop"].data_ptr(),
                  pb.bs["dtop"], st)
        assert _lib.last_kernel() == "upsample2x_cl_bwd_kernel", _lib.last_kernel()
    return {k: v.cpu() for k, v in out.items()}


def _view(buf, pb, H, W, bs):
    return buf.as_strided((pb.N, pb.C, H, W), (bs, 1, W * pb.C, pb.C))


def _module(pb):
    from mp_former_amd.groupnorm import GroupNorm
    gn = GroupNorm(pb.G, pb.C, eps=pb.eps).to(DEV)
    with torch.no_grad():
        gn.weight.copy_(pb.gamma); gn.bias.copy_(pb.beta)
    return gn


def _run_autograd(pb, d, gy_layout):
    """GroupNorm.forward_cl and its backward -> result namespace (mean and rstd stay inside the wrapper)"""
    from mp_former_amd import _lib
    from mp_former_amd.groupnorm import is_cl_plane
    gn = _module(pb)
    x = _view(d["x"], pb, pb.H, pb.W, pb.bs["x"]).requires_grad_(True)
    top = _view(d["top"], pb, pb.Ht, pb.Wt, pb.bs["top"]).requires_grad_(True) if pb.has_top else None
    assert gn.cl_ok(x, top)
    y = gn.forward_cl(x, relu=pb.relu, top=top)
    assert _lib.last_kernel() == "gn_cl_apply_kernel" and is_cl_plane(y)
    if gy_layout == "strided":
        gy = _view(d["gy"], pb, pb.H, pb.W, pb.bs["gy"])
        assert is_cl_plane(gy) and gy.stride(0) == pb.bs["gy"]
    else:
        gy = GC._nchw(pb.gy, pb).contiguous().to(DEV)
        assert gy.is_contiguous() and not is_cl_plane(gy)
    grads = torch.autograd.grad(y, [x, gn.weight, gn.bias] + ([top] if pb.has_top else []), gy)
    assert _lib.last_kernel() == ("upsample2x_cl_bwd_kernel" if pb.has_top else "gn_cl_bwd_apply_kernel"), _lib.last_kernel()
    return GC.SimpleNamespace(y=GC._cl(y.detach()), dx=GC._cl(grads[0]), dgamma=grads[1], dbeta=grads[2],
                              dtop=GC._cl(grads[3]) if pb.has_top else None)


NCHW_GY = {"c64g2_8x16", "c256g8_9x5", "c128g8_6x10_gaps", "c256g32_top_2x6"}          # rows that also get an NCHW-contiguous gy
assert GC.CL_CASES["c64g2_8x16"]["N"] == 1                                              # (the memory-format query is ambiguous at N = 1)


@pytest.mark.parametrize("name,mode", GC.CL_RUNS)
def test_channel_last_against_fp64(name, mode):
    pb, ref = GC.cl_case(name, mode)
    d = _upload(pb)
    res = GC.take_all(pb, _run_abi(pb, d))
    GC.check_all(pb, ref, res, route="abi")
    aten = GC.aten_results(pb, DEV) if pb.dist != "std" else None
    if aten is not None:
        GC.check_vs_aten(pb, ref, res.dx, aten.dx, route="abi")
    for layout in ("strided", "nchw") if name in NCHW_GY else ("strided",):
        auto = _run_autograd(pb, d, layout)
        GC.check_all(pb, ref, auto, route=f"autograd gy {layout}")
        if aten is not None:
            GC.check_vs_aten(pb, ref, auto.dx, aten.dx, route="autograd")


def test_production_case_is_bit_identical_on_a_second_run():
    pb, _ = GC.cl_case("c256g32_82x100", "plain")
    assert GC.make_plane(pb.HW, pb.C, pb.G).chunks == 65
    d = _upload(pb)
    a, b = _run_abi(pb, d), _run_abi(pb, d)
    for k in ("y", "mean", "rstd", "dx", "dgamma", "dbeta"):
        assert torch.equal(GC._bits(a[k]), GC._bits(b[k])), f"{k} differs between two runs"


def test_group_norm_flatten_against_fp64_per_level():
    from mp_former_amd.groupnorm import group_norm_flatten
    N, C, G = 2, 32, 8
    pbs = [GC.cl_problem(f"flatten_level{i}", "plain", hw=hw, C=C, G=G, N=N, gaps=i != 1) for i, hw in enumerate(GC.FLATTEN_LEVELS)]
    assert [GC.make_plane(p.HW, C, G).chunks for p in pbs] == [1, 2, 65] and [p.HW % 128 for p in pbs] == [0, 1, 8]
    norms = [_module(p) for p in pbs]
    xs = [_view(p.x_buf.to(DEV), p, p.H, p.W, p.bs["x"]).requires_grad_(True) for p in pbs]
    out = group_norm_flatten(norms, xs)
    S = sum(p.HW for p in pbs)
    assert out is not None and out.shape == (N, S, C) and out.is_contiguous()
    g = torch.cat([p.gy for p in pbs], 1).to(DEV)
    leaves = xs + [n.weight for n in norms] + [n.bias for n in norms]
    grads = torch.autograd.grad(out, leaves, g)
    off = 0
    for i, p in enumerate(pbs):
        res = GC.SimpleNamespace(y=out.detach()[:, off:off + p.HW], dx=GC._cl(grads[i]), dgamma=grads[3 + i], dbeta=grads[6 + i])
        GC.check_all(p, GC.cl_reference(p), res, route="group_norm_flatten")
        off += p.HW


# ---- NCHW route --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GC.NCHW_CASES))
def test_group_stats_against_fp64(name):
    from mp_former_amd import _lib
    np_ = GC.nchw_problem(name)
    buf = np_.buf.to(DEV)
    mean, rstd = GC.sentinel(np_.rows + GC.GUARD).to(DEV), GC.sentinel(np_.rows + GC.GUARD).to(DEV)
    need = _lib.lib().mpf_group_stats_workspace_bytes(np_.rows, np_.row_len)
    assert need == GC.group_stats_workspace_bytes(np_.rows, np_.row_len)
    ws = _poison_bytes(need)
    _lib.call("mpf_group_stats", DEV, buf.data_ptr() + 4 * GC.NCHW_PAD, np_.rows, np_.row_len, np_.eps, mean.data_ptr(), rstd.data_ptr(),
              ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV))
    assert _lib.last_kernel() == "gn_chunk_stats_kernel", _lib.last_kernel()
    GC.check_stats(np_, mean, rstd)


@pytest.mark.parametrize("name", list(GC.NCHW_MODULE_CASES))
def test_nchw_function_against_fp64(name):
    from mp_former_amd import _lib
    from mp_former_amd.groupnorm import _GroupNormFn
    shape, G = GC.NCHW_MODULE_CASES[name]
    pb = GC.module_problem(shape, G, f"nchw_fn_{name}")
    x = GC._nchw(pb.x, pb).contiguous().to(DEV).requires_grad_(True)
    w, b = pb.gamma.to(DEV).requires_grad_(True), pb.beta.to(DEV).requires_grad_(True)
    y = _GroupNormFn.apply(x, w, b, G, pb.eps)
    assert _lib.last_kernel() == "gn_chunk_stats_kernel", _lib.last_kernel()
    grads = torch.autograd.grad(y, [x, w, b], GC._nchw(pb.gy, pb).contiguous().to(DEV))
    res = GC.SimpleNamespace(y=GC._cl(y.detach()), dx=GC._cl(grads[0]), dgamma=grads[1], dbeta=grads[2])
    GC.check_all(pb, GC.cl_reference(pb), res, route="_GroupNormFn")


# ---- fallback chain ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["channels_last", "contiguous"])
@pytest.mark.parametrize("shape,G,kernel", GC.FALLBACK_CASES)
def test_fallback_chain_against_fp64(shape, G, kernel, layout):
    from mp_former_amd import _lib
    pb = GC.module_problem(shape, G, f"fallback_{shape[1]}_{G}")
    gn = _module(pb)
    x = GC._nchw(pb.x, pb).to(DEV)
    x = (x.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else x.contiguous()).requires_grad_(True)
    assert not gn.cl_ok(x)
    # a native call of another family first: last_kernel() then cannot be a stale gn_cl_ name, and the profile counts what runs
    one = torch.ones(4, device=DEV)
    _lib.call("mpf_amax_f32", DEV, one.data_ptr(), 4, torch.zeros(1, device=DEV).data_ptr(), _lib.stream_ptr(DEV))
    assert "gn_" not in _lib.last_kernel()
    _lib.profile_enable(True)
    try:
        y = gn(x)
        assert _lib.profile_get("gn_cl_")[0] == 0 and _lib.profile_get("gn_chunk_stats_kernel")[0] == (0 if kernel is None else 1)
    finally:
        _lib.profile_enable(False)
    assert "gn_cl_" not in _lib.last_kernel()
    if kernel is not None:
        assert _lib.last_kernel() == kernel, _lib.last_kernel()
    grads = torch.autograd.grad(y, [x, gn.weight, gn.bias], GC._nchw(pb.gy, pb).to(DEV))
    assert "gn_cl_" not in _lib.last_kernel()
    res = GC.SimpleNamespace(y=GC._cl(y.detach()), dx=GC._cl(grads[0]), dgamma=grads[1], dbeta=grads[2])
    GC.check_all(pb, GC.cl_reference(pb), res, route=f"GroupNorm.forward {layout}")
