"""CPU: tests/_mask_fused_cases.py held to einsum, autograd, the oracle and the built library, so that the GPU test
(tests/test_mask_fused_routes_gpu.py) can rely on it: the fp64 references, the input conditions and the named geometry of every
GPU case, the geometry mirrors against the library's workspace queries, the argument checks of the three entry points (no launch),
and the emulation: without a fault it passes the check functions the GPU test uses, with each single fault it fails them."""
import ctypes

import numpy as np
import pytest
import torch

import _loss_restate as LR
import _mask_fused_cases as MC

F64 = torch.float64


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib.lib()


def _all_pair_problems():
    for hw in MC.FWD_HW:
        for counts in MC.FWD_COUNTS:
            yield f"fwd {hw} {counts}", MC.fwd_problem(hw, counts)
    for name in MC.PAIR_CASES:
        yield name, MC.pair_case(name)


# ---- references -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P3", "P8", "P6"])
def test_pair_references_equal_einsum_and_autograd(name):
    pb = MC.pair_case(name)
    E = torch.nan_to_num(pb.embed.to(F64)).transpose(0, 1).contiguous().requires_grad_(True)                  # [N, R, C]
    F = torch.nan_to_num(pb.feat.to(F64)).view(pb.N, -1)[:, :pb.HW * MC.C].reshape(pb.N, pb.h, pb.w, MC.C).permute(0, 3, 1, 2)
    F = F.contiguous().requires_grad_(True)
    maps = torch.einsum("bqc,bchw->bqhw", E, F).flatten(2)                                                      # [N, R, HW]
    b, r = pb.slot_img[pb.vslots], pb.slot_row[pb.vslots]
    ref, _ = MC.planes_ref(pb)
    torch.testing.assert_close(ref, maps[b, r].detach(), rtol=1e-12, atol=1e-12)
    up = torch.zeros_like(maps)
    up[b, r] = pb.G[pb.vslots].to(F64)
    gE, gF = torch.autograd.grad(maps, [E, F], up)
    refs = MC.grads_ref(pb)
    torch.testing.assert_close(refs.dE, gE[b, r], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(refs.dF, gF.permute(0, 2, 3, 1).reshape(pb.N, pb.HW, MC.C), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", ["C1", "C2", "C5", "C9"])
def test_cost_reference_equals_the_oracle_on_materialised_maps(name):
    from oracle import head_ref as O
    cp = MC.cost_case(name)
    for gi in range(cp.G):
        Tn = int(cp.t_count[gi])
        if Tn == 0:
            continue
        E, Fm, c = MC.group_embed(cp, gi).to(F64), MC.group_feat(cp, gi).to(F64), cp.coords[gi].to(F64)
        masks = cp.masks[cp.group_image[gi]]
        mine = LR.match_cost_samples(MC.logits_ref(E, Fm, c, cp.h, cp.w), LR.point_sample(masks, c[None]), MC.W_MASK, MC.W_DICE)
        maps = torch.einsum("qc,xc->qx", E, Fm).view(cp.Q, cp.h, cp.w)
        want = O.matcher_cost(torch.zeros(cp.Q, 2, dtype=F64), maps, torch.zeros(Tn, dtype=torch.long), masks, c[None], w_class=0.0,
                              w_mask=MC.W_MASK, w_dice=MC.W_DICE)
        assert want.dtype == F64
        torch.testing.assert_close(mine, want, rtol=1e-9, atol=1e-9)
        torch.testing.assert_close(mine, LR.match_cost(maps, masks, c[None], MC.W_MASK, MC.W_DICE), rtol=1e-9, atol=1e-9)
        # the reference the GPU test uses differs only by the fp32 rounding of the target samples it hands the kernel
        T0 = int(cp.t_first[gi])
        torch.testing.assert_close(cp.tsamp[T0:T0 + Tn].to(F64), LR.point_sample(masks, c[None]), rtol=2.0 ** -24, atol=0)
        if gi == cp.outside_group:
            x = MC.logits_ref(E, Fm, c, cp.h, cp.w)
            assert bool((x == 0).all())
            t = cp.tsamp[T0:T0 + Tn].to(F64)
            closed = MC.W_MASK * np.log(2.0) + MC.W_DICE * (1 - (t.sum(1) + 1) / (cp.P / 2 + t.sum(1) + 1))
            torch.testing.assert_close(MC.cost_ref(cp)[gi], closed[None].expand(cp.Q, -1), rtol=1e-12, atol=1e-12)


# ---- input conditions and named geometry of every GPU case -----------------------------------------------------------------------------
def test_pair_problems_meet_their_input_conditions():
    n = 0
    for name, pb in _all_pair_problems():
        n += 1
        assert pb.max_count >= int(pb.counts.max()) and pb.total >= int((pb.first + pb.counts).max()), name
        b, r = pb.slot_img[pb.vslots], pb.slot_row[pb.vslots]
        assert len(set(zip(b.tolist(), r.tolist()))) == len(pb.vslots) == int(pb.counts.sum()), f"{name}: rows of valid slots repeat"
        assert bool(torch.isfinite(pb.embed[r, b].float()).all()), name
        assert int(torch.isnan(pb.embed.float()).all(2).sum()) == pb.R * pb.N - len(pb.vslots), f"{name}: an unaddressed row is not NaN"
        assert bool(torch.isnan(pb.embed.view(-1)[pb.poison_row:pb.poison_row + MC.C].float()).all())
        fv = pb.feat.view(pb.N, -1).float()
        assert bool(torch.isnan(fv[:, pb.HW * MC.C:]).all()) and pb.feat_stride % 8 == 0, name
        for i in range(pb.N):
            assert bool(torch.isfinite(fv[i, :pb.HW * MC.C]).all()) == (pb.counts[i] > 0), name
        # the pair list addresses exactly the valid slots' rows, in an order that is not the slot order
        n_pairs = len(pb.vslots)
        pos = pb.pair_of_slot.numpy()
        assert sorted(pos[pb.vslots].tolist()) == list(range(n_pairs)) and bool((pos[~pb.valid.numpy()] == n_pairs).all()), name
        assert bool((pb.row_off[:n_pairs][pos[pb.vslots]].numpy() == r * pb.N * MC.C + b * MC.C).all()), name
        if n_pairs > 3:
            assert pos[pb.vslots].tolist() != list(range(n_pairs)), name
        if pb.G is not None:
            assert bool(torch.isfinite(pb.G[pb.vslots].float()).all()) and bool(torch.isnan(pb.G[~pb.valid].float()).all()), name
            assert pb.HW % 128 == 0
            nz = pb.G[pb.sparse_slots].float() != 0
            want = torch.zeros(pb.HW, dtype=torch.bool)
            want[pb.sparse_px] = True
            assert bool((nz == want[None]).all()), f"{name}: the sparse planes' non-zeros are not exactly the boundary pixels"
            assert pb.sparse == (len(pb.sparse_slots) > 0) and (not pb.sparse or len(pb.sparse_slots) < len(pb.vslots))
            assert pb.sparse == (pb.HW > 1024), name
        else:
            assert pb.HW % 4 == 0
    assert n == 25 + 9


@pytest.mark.parametrize("name", list(MC.PAIR_CASES))
def test_pair_cases_reach_the_geometry_they_name(name):
    pb = MC.pair_case(name)
    g = pb.geom
    assert (g.KP, g.mgroups, g.KS, g.px_per_chunk // 64) == MC.PAIR_CASES[name]["geom"]
    assert g.px_per_chunk % 64 == 0 and g.KS * g.px_per_chunk == pb.HW
    if pb.sparse:
        px = set(pb.sparse_px)
        assert {0, 63, 64, g.px_per_chunk - 1, g.px_per_chunk, pb.HW - 65, pb.HW - 64, pb.HW - 1} <= px
        assert len(px) <= 6 + 2 * (g.KS - 1)


@pytest.mark.parametrize("name", list(MC.COST_CASES))
def test_cost_cases_reach_the_geometry_they_name(name):
    cp = MC.cost_case(name)
    m = MC.mc_geom(cp.G, cp.Q, cp.P)
    assert (MC.tch_of(cp.Tmax), m.qgroups, m.tiles_per_wg, m.nwg, m.last_tiles) == MC.COST_CASES[name]["geom"]
    assert cp.Tmax <= 128 and cp.Tmax >= int(cp.t_count.max())
    assert cp.L == 1 or cp.group_image.tolist() != list(range(cp.G))
    assert cp.row_stride % 8 == 0 and cp.feat_stride % 8 == 0 and bool((cp.embed_first % 8 == 0).all())
    addressed = torch.zeros(cp.tsamp.shape[0], dtype=torch.bool)
    for gi in range(cp.G):
        T0, Tn = int(cp.t_first[gi]), int(cp.t_count[gi])
        assert not bool(addressed[T0:T0 + Tn].any())
        addressed[T0:T0 + Tn] = True
        if Tn:
            assert bool(torch.isfinite(MC.group_embed(cp, gi).float()).all()) and bool(torch.isfinite(MC.group_feat(cp, gi).float()).all())
            t = cp.tsamp[T0:T0 + Tn]
            assert bool(((t >= 0) & (t <= 1)).all())
    assert bool(torch.isnan(cp.tsamp[~addressed]).all()) and bool(torch.isfinite(cp.tsamp[addressed]).all())
    assert not bool(addressed[0]) and not bool(addressed[-1]) and int((~addressed).sum()) == cp.G + 2
    lo, hi = float(cp.coords[:, 6:].min()) if cp.P > 6 else -0.1, float(cp.coords[:, 6:].max()) if cp.P > 6 else 1.1
    assert lo >= -0.1 and (hi <= 1.1 or cp.outside_group is not None)
    # the first three rows of every output's block and the rows of groups without targets are NaN
    e = cp.embed.float().view(cp.L, cp.Qt, cp.N, MC.C)
    assert bool(torch.isnan(e[:, :3]).all())
    for gi in range(cp.G):
        l, b = divmod(gi, cp.N)
        assert bool(torch.isnan(e[l, 3:, b]).all()) == (cp.t_count[gi] == 0)


def test_every_tch_instantiation_and_its_boundary_is_in_the_table():
    seen = {MC.tch_of(max(c["counts"])) for c in MC.COST_CASES.values()}
    assert seen == {4, 8, 12, 16, 24, 32, 64}
    assert [MC.tch_of(t) for t in (1, 8, 9, 16, 17, 24, 25, 32, 33, 48, 49, 64, 65, 128)] == [4, 4, 8, 8, 12, 12, 16, 16, 24, 24, 32, 32, 64, 64]
    counts = {c for case in MC.COST_CASES.values() for c in case["counts"]}
    assert {1, 8, 9, 16, 17, 24, 25, 32, 33, 48, 49, 64, 65, 127, 128, 0} <= counts


# ---- mirrors against the built library ---------------------------------------------------------------------------------------------------
def test_workspace_mirrors_equal_the_library(lib):
    for name, pb in _all_pair_problems():
        if pb.G is None:
            continue
        assert lib.mpf_pair_planes_backward_workspace_bytes(pb.N, pb.HW, pb.total, pb.max_count) == \
            MC.pb_workspace_bytes(pb.N, pb.HW, pb.total, pb.max_count) > 0, name
    for name in MC.COST_CASES:
        cp = MC.cost_case(name)
        args = (cp.G, cp.Q, cp.Tmax, cp.P, cp.tsamp.shape[0])
        assert lib.mpf_match_cost_fused_workspace_bytes(*args) == MC.mc_workspace_bytes(*args) > 0, name
    for N, HW, total, mc in [(1, 128, 1, 1), (7, 8576, 900, 300), (64, 65536, 500, 250), (513, 256, 513, 1), (2, 12288, 133, 130)]:
        assert lib.mpf_pair_planes_backward_workspace_bytes(N, HW, total, mc) == MC.pb_workspace_bytes(N, HW, total, mc)
    for bad in [(0, 128, 1, 1), (1, 0, 1, 1), (1, 128, 0, 1), (1, 128, 1, 0), (-1, 128, 1, 1)]:
        assert lib.mpf_pair_planes_backward_workspace_bytes(*bad) == 0 == MC.pb_workspace_bytes(*bad)
    for G, Q, T, P, rows in [(20, 100, 14, 12544, 190), (513, 1, 1, 1, 0), (3, 300, 128, 33, 1000)]:
        assert lib.mpf_match_cost_fused_workspace_bytes(G, Q, T, P, rows) == MC.mc_workspace_bytes(G, Q, T, P, rows)
    for bad in [(0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 1), (1, 1, 1, 0, 1), (1, 1, 1, 1, -1)]:
        assert lib.mpf_match_cost_fused_workspace_bytes(*bad) == 0 == MC.mc_workspace_bytes(*bad)


# ---- argument checks: every call fails a check before any launch ---------------------------------------------------------------------------
DT, SH, NUL = -1, -2, -3                        # MPF_E_DTYPE, MPF_E_SHAPE, MPF_E_NULL


def _caller(fn, ok):
    return lambda **kw: fn(*{**ok, **kw}.values())


def test_forward_argument_errors(lib):
    one = ctypes.c_void_p(16)
    fw = _caller(lib.mpf_pair_planes_forward, dict(embed=one, row_off=one, pos=one, first=one, count=one, feat=one, fs=132 * 256, out=one,
                                                   N=2, HW=132, ch=256, st=None))
    for k in ("embed", "row_off", "first", "count", "feat", "out"):
        assert fw(**{k: None}) == NUL, k
    assert fw(ch=128) == SH and fw(HW=130) == SH and fw(HW=0) == SH and fw(N=0) == SH and fw(fs=132 * 256 + 4) == SH


def test_backward_argument_errors(lib):
    from mp_former_amd import _lib
    one = ctypes.c_void_p(16)
    need = lib.mpf_pair_planes_backward_workspace_bytes(2, 384, 10, 7)
    bw = _caller(lib.mpf_pair_planes_backward, dict(g=one, embed=one, row_off=one, pos=one, first=one, count=one, feat=one, fs=384 * 256,
                                                    dF=one, dfs=384 * 256, dE=one, dt=_lib.MPF_BF16, N=2, HW=384, ch=256, total=10, mc=7,
                                                    ws=one, wsb=need - 1, st=None))
    assert bw() == SH and b"workspace" in lib.mpf_last_error()                       # one byte short, everything else valid
    for k in ("g", "embed", "row_off", "first", "count", "feat", "ws"):
        assert bw(**{k: None}) == NUL, k
    assert bw(ch=255) == SH and bw(HW=388) == SH and b"128" in lib.mpf_last_error()
    assert bw(HW=64) == SH and bw(fs=384 * 256 + 4) == SH and bw(dfs=384 * 256 + 2) == SH and bw(total=0) == SH and bw(mc=0) == SH
    assert bw(dt=_lib.MPF_F64) == DT and bw(dt=_lib.MPF_U8) == DT and bw(dt=99) == DT
    assert bw(dt=99, dE=None) == SH                                                   # no d_embed: its dtype is not looked at


def test_match_cost_argument_errors(lib):
    one = ctypes.c_void_p(16)
    need = lib.mpf_match_cost_fused_workspace_bytes(4, 10, 32, 112, 130)
    mc = _caller(lib.mpf_match_cost_fused, dict(embed=one, ef=one, ers=512, feat=one, fs=96 * 256, gi=one, h=8, w=12, ch=256, coords=one,
                                                tsamp=one, rows=130, tf=one, tc=one, cost=one, G=4, Q=10, Tmax=32, P=112, wm=5.0, wd=5.0,
                                                ws=one, wsb=need - 1, st=None))
    assert mc() == SH and b"workspace" in lib.mpf_last_error()
    for k in ("embed", "ef", "feat", "gi", "coords", "tsamp", "tf", "tc", "cost", "ws"):
        assert mc(**{k: None}) == NUL, k
    assert mc(ch=64) == SH and mc(ers=508) == SH and mc(fs=96 * 256 + 4) == SH and mc(P=0) == SH and mc(h=0) == SH
    assert mc(Tmax=129, wsb=1 << 40) == SH and b"128" in lib.mpf_last_error()


# ---- the emulation passes every check; every single fault fails its named case ------------------------------------------------------------
def test_forward_emulation_passes_and_each_fault_fails():
    for hw in MC.FWD_HW:
        for counts in MC.FWD_COUNTS:
            pb = MC.fwd_problem(hw, counts)
            _, frac = MC.check_planes(pb, MC.emu_planes(pb), f"emulation {hw} {counts}")
            assert frac <= 1.0
    for fault, (hw, counts) in MC.FWD_FAULT_CASE.items():
        pb = MC.fwd_problem(hw, counts)
        with pytest.raises(AssertionError):
            MC.check_planes(pb, MC.emu_planes(pb, fault), f"fault {fault}")
    assert set(MC.FWD_FAULT_CASE) == set(MC.PLANES_FAULTS)


@pytest.mark.parametrize("name", list(MC.PAIR_CASES))
def test_backward_emulation_passes_and_each_fault_fails(name):
    pb = MC.pair_case(name)
    refs = MC.grads_ref(pb)
    MC.check_planes(pb, MC.emu_planes(pb), f"emulation {name}")
    MC.check_dfeat(pb, MC.emu_dfeat(pb), refs, f"emulation {name}")
    for dt in (torch.bfloat16, torch.float32):
        MC.check_dembed(pb, MC.emu_dembed(pb, dt), refs, f"emulation {name}")
    for fault, case in MC.DFEAT_FAULT_CASE.items():
        if case == name:
            with pytest.raises(AssertionError):
                MC.check_dfeat(pb, MC.emu_dfeat(pb, fault), refs, f"fault {fault} {name}")
    for fault, cases in MC.DEMBED_FAULT_CASE.items():
        if name in cases:
            for dt in (torch.bfloat16, torch.float32):
                with pytest.raises(AssertionError):
                    MC.check_dembed(pb, MC.emu_dembed(pb, dt, fault), refs, f"fault {fault} {name}")


def test_every_backward_fault_has_a_case():
    assert set(MC.DFEAT_FAULT_CASE) == set(MC.DFEAT_FAULTS) and set(MC.DEMBED_FAULT_CASE) == set(MC.DEMBED_FAULTS)
    assert set(MC.COST_FAULT_CASE) == set(MC.COST_FAULTS)
    assert all(c in MC.PAIR_CASES for c in MC.DFEAT_FAULT_CASE.values()) and all(c in MC.PAIR_CASES for cs in MC.DEMBED_FAULT_CASE.values() for c in cs)
    dense, sparse = MC.DEMBED_FAULT_CASE["chunk_tail"]
    assert not MC.PAIR_CASES[dense]["sparse"] and MC.PAIR_CASES[sparse]["sparse"]


@pytest.mark.parametrize("name", list(MC.COST_CASES))
def test_cost_emulation_passes_and_each_fault_fails(name):
    cp = MC.cost_case(name)
    ref = MC.cost_ref(cp)
    MC.check_cost(cp, MC.emu_cost(cp), ref, f"emulation {name}")
    for fault, case in MC.COST_FAULT_CASE.items():
        if case == name:
            with pytest.raises(AssertionError):
                MC.check_cost(cp, MC.emu_cost(cp, fault), ref, f"fault {fault} {name}")
