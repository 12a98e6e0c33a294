"""GPU: mpf_match_cost_fused_clip through the C ABI on the problems of tests/_mask_fused_clip_cases.py (NaN poison behind every
frame, around every group's target rows and in every embedding row that no group addresses), held to the fp64 reference with
|got - ref| <= 2e-4 + 2e-4 |ref| at w_mask = w_dice = 5 for every entry t < t_count[g]; entries t >= t_count[g] and groups without
tubes keep the sentinel; two runs are bit-equal; with F = 1 the cost is mpf_match_cost_fused's bit for bit; argument errors return
before any launch."""
import numpy as np
import pytest
import torch

import _mask_fused_cases as MC
import _mask_fused_clip_cases as KC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F32 = torch.float32


def _i32(a):
    return torch.from_numpy(np.asarray(a).astype(np.int32)).to(DEV)


def _poison_bytes(n):
    return torch.full((max(int(n), 1),), 0xFF, dtype=torch.uint8, device=DEV)          # NaN as bf16 and as fp32


def _upload(cp):
    return {"embed": cp.embed.to(DEV), "ef": torch.from_numpy(cp.embed_first).to(DEV), "feat": cp.feat.to(DEV), "gc": _i32(cp.group_clip),
            "coords": cp.coords.to(DEV), "tsamp": cp.tsamp.to(DEV), "tf": _i32(cp.t_first), "tc": _i32(cp.t_count)}


def _args(cp, d, cost, ws, **kw):
    from mp_former_amd import _lib
    a = dict(embed=d["embed"].data_ptr(), ef=d["ef"].data_ptr(), ers=cp.row_stride, feat=d["feat"].data_ptr(), cs=cp.clip_stride,
             fs=cp.frame_stride, gc=d["gc"].data_ptr(), h=cp.h, w=cp.w, ch=MC.C, coords=d["coords"].data_ptr(), tsamp=d["tsamp"].data_ptr(),
             rows=cp.tsamp.shape[0], tf=d["tf"].data_ptr(), tc=d["tc"].data_ptr(), cost=cost.data_ptr(), G=cp.G, Q=cp.Q, Tmax=cp.Tmax, P=cp.P,
             F=cp.F, wm=MC.W_MASK, wd=MC.W_DICE, ws=ws.data_ptr(), wsb=ws.numel(), st=_lib.stream_ptr(DEV))
    a.update(kw)
    return tuple(a.values())


def _cost(cp, d):
    from mp_former_amd import _lib
    cost = torch.full((cp.G, cp.Q, cp.Tmax), MC.SENT_GRAD, dtype=F32, device=DEV)
    ws = _poison_bytes(_lib.lib().mpf_match_cost_fused_clip_workspace_bytes(cp.G, cp.Q, cp.Tmax, cp.P, cp.F, cp.tsamp.shape[0]))
    _lib.profile_enable(True)
    try:
        _lib.call("mpf_match_cost_fused_clip", DEV, *_args(cp, d, cost, ws))
        assert _lib.last_kernel() == "match_cost_fused_kernel", _lib.last_kernel()
        assert _lib.profile_get("match_cost_fused_kernel")[0] == 1
    finally:
        _lib.profile_enable(False)
    return cost


@pytest.mark.parametrize("name", list(KC.CLIP_CASES))
def test_clip_cost_against_fp64(name):
    from mp_former_amd import _lib
    cp = KC.clip_case(name)
    d = _upload(cp)
    cost = _cost(cp, d)
    KC.check_cost(cp, cost, KC.cost_ref(cp), f"{name} F={cp.F} TCH={MC.tch_of(cp.Tmax)} Q={cp.Q} P={cp.P}")
    if cp.outside_group is not None:
        gi, n = cp.outside_group, int(cp.t_count[cp.outside_group])
        assert bool((cost[gi, 1:, :n] == cost[gi, :1, :n]).all()), "all-zero logits: every query must get the same cost"
    assert torch.equal(_cost(cp, d), cost), "two runs differ"
    if cp.F == 1:                                   # the image entry on the same buffers: the same bits
        img = torch.full_like(cost, MC.SENT_GRAD)
        ws = _poison_bytes(_lib.lib().mpf_match_cost_fused_workspace_bytes(cp.G, cp.Q, cp.Tmax, cp.P, cp.tsamp.shape[0]))
        _lib.call("mpf_match_cost_fused", DEV, d["embed"].data_ptr(), d["ef"].data_ptr(), cp.row_stride, d["feat"].data_ptr(), cp.clip_stride,
                  d["gc"].data_ptr(), cp.h, cp.w, MC.C, d["coords"].data_ptr(), d["tsamp"].data_ptr(), cp.tsamp.shape[0], d["tf"].data_ptr(),
                  d["tc"].data_ptr(), img.data_ptr(), cp.G, cp.Q, cp.Tmax, cp.P, MC.W_MASK, MC.W_DICE, ws.data_ptr(), ws.numel(),
                  _lib.stream_ptr(DEV))
        assert torch.equal(img, cost), "F = 1 differs from mpf_match_cost_fused"


def test_argument_errors_return_before_any_launch():
    from mp_former_amd import _lib
    lib = _lib.lib()
    cp = KC.clip_case("K3")
    d = _upload(cp)
    cost = torch.full((cp.G, cp.Q, 129), MC.SENT_GRAD, dtype=F32, device=DEV)
    need = lib.mpf_match_cost_fused_clip_workspace_bytes(cp.G, cp.Q, 129, cp.P, cp.F, cp.tsamp.shape[0])
    ws = _poison_bytes(2 * need)
    before = _lib.last_kernel()
    SH, NUL = -2, -3
    bad = dict(null=dict(embed=None), channels=dict(ch=255), clip_stride=dict(cs=cp.clip_stride + 4), frame_stride=dict(fs=cp.frame_stride + 4),
               row_stride=dict(ers=cp.row_stride + 2), frames_overlap=dict(fs=cp.h * cp.w * MC.C - 8), tmax=dict(Tmax=129),
               workspace=dict(wsb=lib.mpf_match_cost_fused_clip_workspace_bytes(cp.G, cp.Q, cp.Tmax, cp.P, cp.F, cp.tsamp.shape[0]) - 1))
    got = {}
    _lib.profile_enable(True)                       # a launch of the cost kernel would be logged
    try:
        for name, kw in bad.items():
            got[name] = (lib.mpf_match_cost_fused_clip(*_args(cp, d, cost, ws, **kw)), lib.mpf_last_error())
        n_logged = _lib.profile_get("match_cost_fused_kernel")[0]
    finally:
        _lib.profile_enable(False)
    assert {k: v[0] for k, v in got.items()} == {k: (NUL if k == "null" else SH) for k in bad}
    assert b"128" in got["tmax"][1] and b"workspace" in got["workspace"][1] and b"overlap" in got["frames_overlap"][1]
    assert n_logged == 0 and _lib.last_kernel() == before
    torch.cuda.synchronize()
    assert bool((cost == MC.SENT_GRAD).all()), "a rejected call wrote to the cost buffer"
    with pytest.raises(RuntimeError, match="mpf_match_cost_fused_clip failed with code -2"):
        _lib.call("mpf_match_cost_fused_clip", DEV, *_args(cp, d, cost, ws, Tmax=129))
