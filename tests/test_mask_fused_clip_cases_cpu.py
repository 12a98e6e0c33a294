"""CPU: tests/_mask_fused_clip_cases.py held to the image reference, the built library and its own emulation, so that the GPU test
(tests/test_mask_fused_clip_gpu.py) can rely on it: the fp64 reference against the cost of the materialised tall map with zero
padding per frame, the input conditions and named geometry of every case, the workspace mirror against the library's query, the
argument checks of mpf_match_cost_fused_clip (no launch), and the emulation: without a fault it passes the check function the GPU
test uses, with each single fault it fails it on a named case."""
import ctypes

import pytest
import torch

import _loss_restate as LR
import _mask_fused_cases as MC
import _mask_fused_clip_cases as KC

F64 = torch.float64
SH, NUL, BIG = -2, -3, -4                        # MPF_E_SHAPE, MPF_E_NULL, MPF_E_TOO_LARGE


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", ["K3", "K4", "K5"])
def test_reference_equals_the_cost_of_the_materialised_frames(name):
    """every frame's map is sampled on its own (zero padding per frame) and the samples are laid frame-major"""
    cp = KC.clip_case(name)
    ref = KC.cost_ref(cp)
    for gi in range(cp.G):
        Tn = int(cp.t_count[gi])
        if Tn == 0:
            assert ref[gi] is None
            continue
        E, c = KC.group_embed(cp, gi).to(F64), cp.coords[gi].to(F64)
        maps = torch.stack([torch.einsum("qc,xc->qx", E, KC.frame_feat(cp, gi, f).to(F64)).view(cp.Q, cp.h, cp.w) for f in range(cp.F)], 1)
        x = LR.point_sample(maps.reshape(cp.Q * cp.F, cp.h, cp.w), c[None]).reshape(cp.Q, cp.F * cp.P)
        m = cp.masks[cp.group_clip[gi]]
        t = LR.point_sample(m.reshape(Tn * cp.F, *MC.GT_HW), c[None]).reshape(Tn, cp.F * cp.P)
        torch.testing.assert_close(ref[gi], LR.match_cost_samples(x, t.float(), MC.W_MASK, MC.W_DICE), rtol=1e-9, atol=1e-9)
        if gi == cp.outside_group:
            assert bool((x == 0).all())


def test_one_frame_is_the_image_reference():
    cp = KC.clip_case("K1")
    ref = KC.cost_ref(cp)
    img = MC.SimpleNamespace(**{**vars(cp), "group_image": cp.group_clip, "feat_stride": cp.clip_stride})
    for a, b in zip(ref, MC.cost_ref(img)):
        assert (a is None and b is None) or torch.equal(a, b)
    assert KC.CLIP_CASES["K1"]["Q"] == MC.COST_CASES["C2"]["Q"] and KC.CLIP_CASES["K1"]["P"] == MC.COST_CASES["C2"]["P"]
    assert KC.CLIP_CASES["K1"]["counts"] == MC.COST_CASES["C2"]["counts"] and KC.CLIP_CASES["K2"]["counts"] == MC.COST_CASES["C4"]["counts"]
    assert KC.CLIP_CASES["K2"]["Q"] == MC.COST_CASES["C4"]["Q"] and KC.CLIP_CASES["K2"]["P"] == MC.COST_CASES["C4"]["P"]


@pytest.mark.parametrize("name", list(KC.CLIP_CASES))
def test_cases_reach_the_geometry_they_name_and_meet_their_input_conditions(name):
    cp = KC.clip_case(name)
    m = KC.mc_geom_clip(cp.G, cp.Q, cp.P, cp.F)
    assert (MC.tch_of(cp.Tmax), m.qgroups, m.per_frame, m.tiles_per_wg, m.nwg, m.crossing) == KC.CLIP_CASES[name]["geom"]
    if cp.F == 1:
        i = MC.mc_geom(cp.G, cp.Q, cp.P)
        assert (i.ntiles, i.tiles_per_wg, i.nwg) == (m.ntiles, m.tiles_per_wg, m.nwg)
    assert cp.row_stride % 8 == 0 and cp.clip_stride % 8 == 0 and cp.frame_stride % 8 == 0 and bool((cp.embed_first % 8 == 0).all())
    assert cp.frame_stride == cp.h * cp.w * MC.C + 64 and cp.tsamp.shape[1] == cp.F * cp.P
    fv = cp.feat.float().view(cp.N, cp.F, cp.frame_stride)
    assert bool(torch.isnan(fv[:, :, cp.h * cp.w * MC.C:]).all()), "the 64 elements behind a frame are not poison"
    for b in range(cp.N):
        assert bool(torch.isfinite(fv[b, :, :cp.h * cp.w * MC.C]).all()) == (cp.counts[b] > 0)
    addressed = torch.zeros(cp.tsamp.shape[0], dtype=torch.bool)
    for gi in range(cp.G):
        T0, Tn = int(cp.t_first[gi]), int(cp.t_count[gi])
        assert not bool(addressed[T0:T0 + Tn].any())
        addressed[T0:T0 + Tn] = True
    assert bool(torch.isnan(cp.tsamp[~addressed]).all()) and bool(torch.isfinite(cp.tsamp[addressed]).all())
    assert not bool(addressed[0]) and not bool(addressed[-1]) and int((~addressed).sum()) == cp.G + 2
    e = cp.embed.float().view(cp.L, cp.Qt, cp.N, MC.C)
    assert bool(torch.isnan(e[:, :3]).all())
    for gi in range(cp.G):
        l, b = divmod(gi, cp.N)
        assert bool(torch.isnan(e[l, 3:, b]).all()) == (cp.t_count[gi] == 0)
    # planted points: y = 0, y = 1, a footprint with its lower corners in row h, one with its upper corners in row -1, outside
    _, y0, _, ly = LR.corners(cp.coords[0], cp.h, cp.w)
    n = min(cp.P, 8)
    if n == 8:
        assert y0[:8].tolist() == [-1, cp.h - 1, cp.h - 1, -1, -cp.h - 1, 2 * cp.h - 1, cp.h - 1, cp.h - 1]
        assert float(ly[2]) == 0.25 and float(ly[6]) == 0.375 and float(ly[7]) == 0.125


def test_the_long_case_lets_a_workgroup_cross_the_frame_boundary():
    c = KC.CLIP_CASES["K6"]
    m = KC.mc_geom_clip(c["L"] * c["N"], c["Q"], c["P"], c["F"])
    assert m.per_frame == 129 and m.tiles_per_wg == 5 and 129 % 5 and m.crossing == 1
    assert MC.mc_geom(c["L"] * c["N"], c["Q"], c["P"]).tiles_per_wg == 3          # (the image geometry of one frame alone)


def test_workspace_mirror_equals_the_library(lib):
    for name in KC.CLIP_CASES:
        cp = KC.clip_case(name)
        args = (cp.G, cp.Q, cp.Tmax, cp.P, cp.F, cp.tsamp.shape[0])
        assert lib.mpf_match_cost_fused_clip_workspace_bytes(*args) == KC.clip_workspace_bytes(*args) > 0, name
    for G, Q, T, P, F, rows in [(20, 100, 14, 12544, 2, 190), (513, 1, 1, 1, 7, 0), (3, 300, 128, 33, 36, 1000), (4, 100, 9, 12544, 1, 40)]:
        assert lib.mpf_match_cost_fused_clip_workspace_bytes(G, Q, T, P, F, rows) == KC.clip_workspace_bytes(G, Q, T, P, F, rows) > 0
        if F == 1:
            assert lib.mpf_match_cost_fused_workspace_bytes(G, Q, T, P, rows) == KC.clip_workspace_bytes(G, Q, T, P, F, rows)
    for bad in [(0, 1, 1, 1, 1, 1), (1, 0, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1), (1, 1, 1, 0, 1, 1), (1, 1, 1, 1, 0, 1), (1, 1, 1, 1, 1, -1),
                (1, 1, 1, 1 << 20, 1 << 11, 1)]:
        assert lib.mpf_match_cost_fused_clip_workspace_bytes(*bad) == 0 == KC.clip_workspace_bytes(*bad)


def test_argument_errors(lib):
    one = ctypes.c_void_p(16)
    need = lib.mpf_match_cost_fused_clip_workspace_bytes(4, 10, 32, 112, 3, 130)
    ok = dict(embed=one, ef=one, ers=512, feat=one, cs=3 * (96 * 256 + 64), fs=96 * 256 + 64, gc=one, h=8, w=12, ch=256, coords=one,
              tsamp=one, rows=130, tf=one, tc=one, cost=one, G=4, Q=10, Tmax=32, P=112, F=3, wm=5.0, wd=5.0, ws=one, wsb=need - 1, st=None)
    mc = lambda **kw: lib.mpf_match_cost_fused_clip(*{**ok, **kw}.values())
    assert mc() == SH and b"workspace" in lib.mpf_last_error()                       # one byte short, everything else valid
    for k in ("embed", "ef", "feat", "gc", "coords", "tsamp", "tf", "tc", "cost", "ws"):
        assert mc(**{k: None}) == NUL, k
    assert mc(ch=255) == SH and mc(ers=508) == SH and mc(cs=3 * (96 * 256 + 64) + 4) == SH and mc(fs=96 * 256 + 4) == SH
    assert mc(fs=96 * 256 - 8) == SH and b"overlap" in lib.mpf_last_error()
    assert mc(P=0) == SH and mc(h=0) == SH and mc(F=0) == SH
    assert mc(Tmax=129, wsb=1 << 40) == SH and b"128" in lib.mpf_last_error()
    assert mc(F=65536, wsb=1 << 40) == BIG and mc(G=65536, wsb=1 << 40) == BIG and mc(F=65535, P=1 << 16, wsb=1 << 40) == BIG


@pytest.mark.parametrize("name", list(KC.CLIP_CASES))
def test_emulation_passes_and_each_fault_fails(name):
    cp = KC.clip_case(name)
    ref = KC.cost_ref(cp)
    KC.check_cost(cp, KC.emu_cost(cp), ref, f"emulation {name}")
    for fault, case in KC.CLIP_FAULT_CASE.items():
        if case == name:
            with pytest.raises(AssertionError):
                KC.check_cost(cp, KC.emu_cost(cp, fault), ref, f"fault {fault} {name}")


def test_every_fault_has_a_case():
    assert set(KC.CLIP_FAULT_CASE) == set(KC.CLIP_FAULTS) and all(c in KC.CLIP_CASES for c in KC.CLIP_FAULT_CASE.values())
    assert all(KC.CLIP_CASES[c]["F"] > 1 for c in KC.CLIP_FAULT_CASE.values())
