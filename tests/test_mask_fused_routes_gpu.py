"""GPU: the three entry points of csrc/mask_fused.hip through the C ABI (_lib.call) against the per-element fp64 references of
tests/_mask_fused_cases.py, at every tile boundary, tail and edge of the six kernels.  The problems, bounds, geometry and the
check functions are that file's; tests/test_mask_fused_cases_cpu.py holds them to einsum, autograd, the oracle and the built
library, shows that every table row reaches the branch it names, and that a single fault of each listed kind fails these checks.

  forward      h x w in {2x2, 10x10, 11x12, 8x16, 13x20} x counts {(1), (15, 16), (17, 31), (32, 33), (48, 49, 0)}: HW % 128 != 0
               (tail workgroup, partially written wave), slot counts on both sides of the 16- and 32-slot steps, shuffled pairs,
               two unaddressed slots before, between and behind the images' ranges
  backward     P1 .. P9: KP 64 .. 320, 1 .. 3 row groups, KS 1 .. 64 with 1 .. 67 steps per chunk, counts 1 / 63 / 64 / 65 / 128 /
               129 / 257, an image without pairs, padded slot ranges, 300 images; d_embed bf16 and fp32, d_features or d_embed NULL
  cost         C1 .. C10: all seven TCH instantiations with targets at TCH and TCH + 1, Q 127 / 128 / 129 / 200, P 1 .. 4128
               (P % 4 != 0 row sums, a last tile of one point), 1 .. 3 tiles per workgroup, groups without targets, NaN rows
               around every group's target samples
Every case asserts the kernel that ran, prints its worst err / bound (`pytest -s`), asserts that sentinels outside the addressed
results are intact and that a second run gives the same bits.

Bounds: planes and gradients |got - ref| <= 2^-8 |ref| [bf16 output] + (K + 8) 2^-22 S + 1e-30 for every element; cost
|got - ref| <= 2e-4 + 2e-4 |ref| for every entry t < t_count[g].  Nothing is asserted about the figures below beyond <= 1.

Worst error seen per kernel (one MI355X run, all cases passing):
  kernel                                   what        max abs err   worst err / bound
  pair_planes_fwd_kernel                   planes      2.5e-01       0.927
  pair_planes_dfeat_kernel                 d F         2.3e-01       0.992
  pair_planes_dembed_kernel + reduce<bf16> d E         9.9e-01       0.970
  pair_planes_dembed_kernel + reduce<float> d E        1.5e-04       0.002
  match_cost_fused_kernel                  cost        2.5e-05       0.009
The bf16 figures near 1 are the rounding of the stored value, not the arithmetic: a correctly rounded bf16 value just above a power
of two is off by up to 2^-8 relative, so the bound has only its fp32 term as slack (the fp32 d E of the same cases: 0.002).
No bug was found in csrc/mask_fused.hip or mask_fused.py: all 54 cases passed on the kernels as they were.
"""
import functools

import numpy as np
import pytest
import torch

import _mask_fused_cases as MC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32


def _i32(a):
    return torch.from_numpy(np.asarray(a).astype(np.int32)).to(DEV)


def _poison_bytes(n):
    return torch.full((max(int(n), 1),), 0xFF, dtype=torch.uint8, device=DEV)          # NaN as bf16 and as fp32


# ---- pair planes ----------------------------------------------------------------------------------------------------------------------
def _upload_pairs(pb):
    d = {"embed": pb.embed.to(DEV), "feat": pb.feat.to(DEV), "first": _i32(pb.first), "count": _i32(pb.counts),
         "G": None if pb.G is None else pb.G.to(DEV)}
    _upload_order(pb, d)
    return d


def _upload_order(pb, d):
    d["row_off"], d["pos"] = pb.row_off.to(DEV), pb.pair_of_slot.to(DEV)


def _forward(pb, d):
    from mp_former_amd import _lib
    out = torch.full((pb.total, pb.HW), MC.SENT_OUT, dtype=BF16, device=DEV)
    _lib.call("mpf_pair_planes_forward", DEV, d["embed"].data_ptr(), d["row_off"].data_ptr(), d["pos"].data_ptr(), d["first"].data_ptr(),
              d["count"].data_ptr(), d["feat"].data_ptr(), pb.feat_stride, out.data_ptr(), pb.N, pb.HW, MC.C, _lib.stream_ptr(DEV))
    assert _lib.last_kernel() == "pair_planes_fwd_kernel", _lib.last_kernel()
    return out


def _backward(pb, d, dtype, want_dF=True, want_dE=True, profile=False):
    """-> (d_features [N, HW, C] that started as SENT_GRAD, d_embed [R, N, C] that started as SENT_GRAD); the workspace has exactly
    the queried size and starts as NaN"""
    from mp_former_amd import _lib
    dF = torch.full((pb.N, pb.HW, MC.C), MC.SENT_GRAD, dtype=BF16, device=DEV) if want_dF else None
    dE = torch.full((pb.R, pb.N, MC.C), MC.SENT_GRAD, dtype=dtype, device=DEV) if want_dE else None
    ws = _poison_bytes(_lib.lib().mpf_pair_planes_backward_workspace_bytes(pb.N, pb.HW, pb.total, pb.max_count))
    if profile:
        _lib.profile_enable(True)
    try:
        _lib.call("mpf_pair_planes_backward", DEV, d["G"].data_ptr(), d["embed"].data_ptr(), d["row_off"].data_ptr(), d["pos"].data_ptr(),
                  d["first"].data_ptr(), d["count"].data_ptr(), d["feat"].data_ptr(), pb.feat_stride, _lib.ptr(dF), pb.HW * MC.C, _lib.ptr(dE),
                  _lib.DTYPE[dtype], pb.N, pb.HW, MC.C, pb.total, pb.max_count, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV))
        assert _lib.last_kernel() == ("pair_planes_dembed_kernel" if want_dE else "pair_planes_dfeat_kernel"), _lib.last_kernel()
        if profile:
            assert _lib.profile_get("pair_planes_dfeat_kernel")[0] == int(want_dF)
            assert _lib.profile_get("pair_planes_dembed_kernel")[0] == int(want_dE)
    finally:
        if profile:
            _lib.profile_enable(False)
    return dF, dE


@pytest.mark.parametrize("counts", MC.FWD_COUNTS)
@pytest.mark.parametrize("hw", MC.FWD_HW)
def test_forward_planes_against_fp64(hw, counts):
    pb = MC.fwd_problem(hw, counts)
    d = _upload_pairs(pb)
    out = _forward(pb, d)
    MC.check_planes(pb, out, f"{hw[0]}x{hw[1]} counts {counts}")
    assert torch.equal(_forward(pb, d), out), "two runs differ"
    order = pb.pair_of_slot.clone()
    MC.set_pair_order(pb, np.random.default_rng(5).permutation(len(pb.vslots)))
    assert len(pb.vslots) < 3 or not torch.equal(order, pb.pair_of_slot)
    _upload_order(pb, d)
    assert torch.equal(_forward(pb, d), out), "another order of the pair list with the same slots changes the planes"


@functools.lru_cache(maxsize=2)
def _pair_case(name):
    pb = MC.pair_case(name)
    return pb, MC.grads_ref(pb), _upload_pairs(pb)


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("name", list(MC.PAIR_CASES))
def test_forward_and_backward_against_fp64(name, dtype):
    pb, refs, d = _pair_case(name)
    from mp_former_amd import _lib
    g = _lib.lib().mpf_pair_planes_backward_workspace_bytes(pb.N, pb.HW, pb.total, pb.max_count)
    assert g == MC.pb_workspace_bytes(pb.N, pb.HW, pb.total, pb.max_count), "the library's geometry is not the table's"
    if dtype == BF16:
        MC.check_planes(pb, _forward(pb, d), name)
    dF, dE = _backward(pb, d, dtype, profile=True)
    MC.check_dfeat(pb, dF, refs, name)
    MC.check_dembed(pb, dE, refs, name)
    dF2, dE2 = _backward(pb, d, dtype)
    assert torch.equal(dF2, dF), "d_features differs between two runs"
    assert torch.equal(dE2, dE), "d_embed differs between two runs"
    only_dE = _backward(pb, d, dtype, want_dF=False, profile=True)[1]
    assert torch.equal(only_dE, dE), "d_embed with d_features = NULL differs from the full call"
    only_dF = _backward(pb, d, dtype, want_dE=False, profile=True)[0]
    assert torch.equal(only_dF, dF), "d_features with d_embed = NULL differs from the full call"


# ---- matching cost --------------------------------------------------------------------------------------------------------------------
def _upload_cost(cp):
    return {"embed": cp.embed.to(DEV), "ef": torch.from_numpy(cp.embed_first).to(DEV), "feat": cp.feat.to(DEV), "gi": _i32(cp.group_image),
            "coords": cp.coords.to(DEV), "tsamp": cp.tsamp.to(DEV), "tf": _i32(cp.t_first), "tc": _i32(cp.t_count)}


def _cost_args(cp, d, cost, ws, Tmax):
    from mp_former_amd import _lib
    return (d["embed"].data_ptr(), d["ef"].data_ptr(), cp.row_stride, d["feat"].data_ptr(), cp.feat_stride, d["gi"].data_ptr(), cp.h, cp.w, MC.C,
            d["coords"].data_ptr(), d["tsamp"].data_ptr(), cp.tsamp.shape[0], d["tf"].data_ptr(), d["tc"].data_ptr(), cost.data_ptr(), cp.G,
            cp.Q, Tmax, cp.P, MC.W_MASK, MC.W_DICE, ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV))


def _cost(cp, d):
    from mp_former_amd import _lib
    cost = torch.full((cp.G, cp.Q, cp.Tmax), MC.SENT_GRAD, dtype=F32, device=DEV)
    ws = _poison_bytes(_lib.lib().mpf_match_cost_fused_workspace_bytes(cp.G, cp.Q, cp.Tmax, cp.P, cp.tsamp.shape[0]))
    _lib.profile_enable(True)
    try:
        _lib.call("mpf_match_cost_fused", DEV, *_cost_args(cp, d, cost, ws, cp.Tmax))
        assert _lib.last_kernel() == "match_cost_fused_kernel", _lib.last_kernel()
        assert _lib.profile_get("match_cost_fused_kernel")[0] == 1
    finally:
        _lib.profile_enable(False)
    return cost


@pytest.mark.parametrize("name", list(MC.COST_CASES))
def test_match_cost_against_fp64(name):
    cp = MC.cost_case(name)
    d = _upload_cost(cp)
    cost = _cost(cp, d)
    ref = MC.cost_ref(cp)
    MC.check_cost(cp, cost, ref, f"{name} TCH={MC.tch_of(cp.Tmax)} Q={cp.Q} P={cp.P}")
    if cp.outside_group is not None:                # logits exactly 0: the closed form (tests/test_mask_fused_cases_cpu.py) to the bound
        gi, n = cp.outside_group, int(cp.t_count[cp.outside_group])
        assert bool((cost[gi, 1:, :n] == cost[gi, :1, :n]).all()), "all-zero logits: every query must get the same cost"
    assert torch.equal(_cost(cp, d), cost), "two runs differ"


def test_129_targets_are_rejected_before_any_launch():
    from mp_former_amd import _lib
    cp = MC.cost_case("C8")
    d = _upload_cost(cp)
    cost = torch.full((cp.G, cp.Q, 129), MC.SENT_GRAD, dtype=F32, device=DEV)
    ws = _poison_bytes(2 * _lib.lib().mpf_match_cost_fused_workspace_bytes(cp.G, cp.Q, 128, cp.P, cp.tsamp.shape[0]))
    before = _lib.last_kernel()
    code = _lib.lib().mpf_match_cost_fused(*_cost_args(cp, d, cost, ws, 129))
    assert code == -2 and b"128" in _lib.lib().mpf_last_error()              # MPF_E_SHAPE
    assert _lib.last_kernel() == before
    torch.cuda.synchronize()
    assert bool((cost == MC.SENT_GRAD).all()), "a rejected call wrote to the cost buffer"
    with pytest.raises(RuntimeError, match="mpf_match_cost_fused failed with code -2"):
        _lib.call("mpf_match_cost_fused", DEV, *_cost_args(cp, d, cost, ws, 129))
