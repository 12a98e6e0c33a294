"""GPU: every kernel route of csrc/loss.hip against the fp64 restatement tests/_loss_restate.py (held to F.grid_sample, the oracle
and autograd by tests/test_loss_restate_cpu.py), at the tails, thresholds and edges of each route; every case asserts the kernel
that ran (_lib.last_kernel()).

Bounds (ceilings the project already holds these kernels to): sums rtol 2e-4 / atol 2e-3, costs 2e-4 / 2e-4, fp32 gradients
1e-4 / 1e-4, bf16 gradients |got - ref| <= 2^-8 |ref| + the fp32 bound (one bf16 rounding is 2^-9 relative; the factor of two
covers the fp32 value it rounds).  Selection: a candidate whose fp64 |logit| is within 1e-5 of the fp64 k-th value may go either
way, every other candidate and the output order must match.

Worst error seen per route (one MI355X run, all 95 cases passing; `pytest -s` prints the figure of every comparison):
  route                               what               max abs err   worst err / bound
  match_cost_lds_kernel<bf16>         cost               2.4e-06       0.001
  match_cost_kernel<bf16>             cost               1.7e-06       0.001
  match_cost_kernel<float>            cost               3.4e-06       0.002
  mask_loss_fwd_lds_kernel            sums               2.1e-04       0.001
  mask_loss_fwd_kernel<bf16>          sums               2.9e-04       0.003
  mask_loss_fwd_kernel<float>         sums               4.3e-04       0.003
  mask_loss_bwd_band_kernel<float>    gradient           4.9e-05       0.312   (400x176, P = 2500)
  mask_loss_bwd_band_kernel<bf16>     gradient           2.4e-01       0.954   (400x176, P = 2500)
  mask_loss_bwd_band_kernel<float>    240 coincident     2.1e-05       0.001
  mask_loss_bwd_band_kernel<bf16>     240 coincident     1.5e-03       0.002
  mask_loss_bwd_kernel<float>         buffer + gradient  1.6e-05       0.127
  mask_loss_bwd_kernel<bf16>          buffer + gradient  1.9e-05       0.109
  point_sample_kernel<bf16>           logits             1.6e-05       0.244
  point_sample_bits_kernel            samples            3.8e-06       0.364
The bf16 gradient's 0.95 is rounding, not arithmetic: bf16 keeps 8 significant bits, so a correctly rounded value just above a power
of two is off by up to 2^-8 relative; its bound has only the fp32 allowance as slack (the fp32 route of the same case: 0.31).
sample_select_kernel<bf16> (M = 700 ... 40960, all three instantiations), select_uncertain_kernel and pack_mask_bits_kernel are
compared exactly (membership, order, bits): every case matched.
"""
import ctypes

import numpy as np
import pytest
import torch

import _loss_restate as LR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENT = -7.0                        # exact in bf16
GT_HW = (40, 56)                   # 2240 pixels = 70 words: rows of 56 straddle the words of the bit-packed form
BF16, F32 = torch.bfloat16, torch.float32
NAME = {BF16: "bf16", F32: "float"}


def _hold(route, what, got, ref, rtol, atol, rel_extra=0.0):
    """print the worst error of this comparison, then assert |got - ref| <= atol + (rtol + rel_extra) |ref| element-wise"""
    got, ref = got.detach().double().cpu(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    frac = err / (atol + (rtol + rel_extra) * ref.abs())
    print(f"[loss-routes] {route} | {what} | max abs err {float(err.max()):.3e} | worst err/bound {float(frac.max()):.3e}")
    assert bool(torch.isfinite(got).all()) and float(frac.max()) <= 1.0, (route, what, float(err.max()), float(frac.max()))


def _sample_atol(h, w, lo, hi):
    """bound of one fp32 bilinear sample of a plane with values in [lo, hi]: the pixel coordinate c * size - 0.5 carries two fp32
    roundings of a number below size (2 * 2^-24 * size pixels) and the value moves by at most hi - lo per pixel, plus a few
    roundings (2^-21 relative) of the blend itself"""
    return 2.0 ** -23 * max(h, w) * (hi - lo) + 2.0 ** -21 * max(abs(lo), abs(hi))


def _i32(a):
    return torch.from_numpy(np.asarray(a).astype(np.int32)).to(DEV)


# ---- matching cost, image form ----------------------------------------------------------------------------------------------------
MC_COUNTS = (5, 0, 1, 4, 8, 9, 16)        # targets per image: the LDS kernel takes 4 per pass, the generic one 8; one image without any
LDS, GEN = "match_cost_lds_kernel<bf16>", "match_cost_kernel<bf16>"
MATCH_CASES = [                            # (h, w), Q, counts, P, grouped, route of the bf16 maps (fp32 maps: always the generic kernel)
    ((16, 24), 6, MC_COUNTS, 500, True, LDS),         # slot j = 0 of the 25 points per thread only
    ((16, 24), 6, MC_COUNTS, 513, True, LDS),         # one point in slot 1
    ((16, 24), 6, MC_COUNTS, 1031, True, LDS),
    ((16, 24), 6, MC_COUNTS, 12800, True, LDS),       # the LDS kernel's limit: all 25 slots of all 512 threads
    ((16, 24), 6, MC_COUNTS, 12801, True, GEN),       # one above it; 51204 bytes of dynamic LDS
    ((5, 7), 6, (3, 0, 9), 500, True, GEN),           # 70-byte planes: not a multiple of 16
    ((264, 256), 2, (5,), 1031, True, LDS),           # 132 KiB planes
    ((280, 256), 2, (5,), 1031, True, GEN),           # 140 KiB planes: above the LDS kernel's 136 KiB
    ((16, 24), 7, (3, 0, 9), 500, True, GEN),         # odd row group
    ((16, 24), 6, (3, 0, 9), 500, False, GEN),        # no row-group guarantee
    ((16, 24), 6, MC_COUNTS, 9000, False, GEN),       # dynamic LDS above 32 KiB ...
    ((16, 24), 6, MC_COUNTS, 20000, False, GEN)]      # ... and above 64 KiB


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("hw,Q,counts,P,grouped,route", MATCH_CASES)
def test_match_cost_against_fp64(hw, Q, counts, P, grouped, route, dtype):
    from mp_former_amd import _lib
    from mp_former_amd.point_sample import MapSet, point_sample_offsets
    g = torch.Generator().manual_seed(11)
    N, (h, w), (H, W), Tmax = len(counts), hw, GT_HW, max(counts)
    masks = (torch.randn(N, Q, h, w, generator=g) * 3).to(dtype)
    gts = [torch.rand(t, H, W, generator=g) < 0.3 for t in counts]
    coords = torch.rand(N, P, 2, generator=g) * 1.1 - 0.05                      # some points outside the planes
    ms = MapSet([masks.to(DEV)])
    b, q = np.repeat(np.arange(N), Q), np.tile(np.arange(Q), N)
    offs = torch.from_numpy(ms.offsets(np.zeros(N * Q, np.int64), b, q)).to(DEV)
    gt_u8 = torch.cat(gts).to(DEV).view(torch.uint8)
    coords_d = coords.to(DEV)
    tsamp = point_sample_offsets(gt_u8.data_ptr(), torch.uint8, H, W, (torch.arange(sum(counts), device=DEV) * H * W).long(), coords_d,
                                 _i32(np.repeat(np.arange(N), counts)), DEV)
    firsts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    crow, first, cnt = _i32(b), _i32(firsts[b]), _i32(np.array(counts)[b])
    cost = torch.full((N * Q, Tmax), SENT, dtype=F32, device=DEV)
    _lib.call("mpf_match_cost", DEV, ms.base_ptr, _lib.DTYPE[dtype], h, w, offs.data_ptr(), coords_d.data_ptr(), crow.data_ptr(),
              tsamp.data_ptr(), first.data_ptr(), cnt.data_ptr(), cost.data_ptr(), N * Q, Tmax, P, 5.0, 5.0, Q if grouped else 1,
              _lib.stream_ptr(DEV))
    want = route if dtype == BF16 else "match_cost_kernel<float>"
    assert _lib.last_kernel() == want, _lib.last_kernel()
    C = cost.view(N, Q, Tmax).cpu()
    ts = tsamp.cpu()
    for i, T in enumerate(counts):
        assert (C[i, :, T:] == SENT).all(), f"image {i}: entries t >= {T} were written"
        if T:
            torch.testing.assert_close(ts[firsts[i]:firsts[i] + T].double(), LR.point_sample(gts[i], coords[i:i + 1]), rtol=0,
                                       atol=_sample_atol(H, W, 0.0, 1.0))
            _hold(want, f"cost {h}x{w} P={P} T={T}", C[i, :, :T], LR.match_cost(masks[i], gts[i], coords[i:i + 1], 5.0, 5.0), 2e-4, 2e-4)


# ---- importance selection ---------------------------------------------------------------------------------------------------------
def _sample_select(planes, coords, k):
    """the fused kernel through the ABI on a sentinel-filled output -> [R, k + 3, 2] on the host"""
    from mp_former_amd import _lib
    from mp_former_amd.point_sample import MapSet
    R, h, w = planes.shape
    ms = MapSet([planes.view(1, R, h, w).to(DEV)])
    offs = torch.from_numpy(ms.offsets(np.zeros(R, np.int64), np.zeros(R, np.int64), np.arange(R))).to(DEV)
    cd = coords.to(DEV)
    out = torch.full((R, k + 3, 2), SENT, dtype=F32, device=DEV)
    _lib.call("mpf_sample_select_uncertain", DEV, ms.base_ptr, _lib.MPF_BF16, h, w, offs.data_ptr(), cd.data_ptr(), out.data_ptr(),
              R, coords.shape[1], k, k + 3, _lib.stream_ptr(DEV))
    assert _lib.last_kernel() == "sample_select_kernel<bf16>", _lib.last_kernel()
    out = out.cpu()
    assert (out[:, k:] == SENT).all(), "coords_out[:, k:] was written"
    return out


@pytest.mark.parametrize("hw,M,k,seed", LR.SELECT_CASES)
def test_sample_select_against_fp64(hw, M, k, seed):
    """the input conditions (distinct coordinates, at most 4 candidates within 1e-5 of the k-th value) are asserted on the CPU by
    tests/test_loss_restate_cpu.py for exactly these problems"""
    planes, coords = LR.select_problem(hw, M, seed)
    keys = LR.point_sample(planes, coords).abs()
    out = _sample_select(planes, coords, k)
    for r in range(LR.SELECT_ROWS):
        LR.check_selection(LR.coords_to_index(coords[r], out[r, :k]), keys[r], k)


def test_two_step_selection_against_fp64():
    """mpf_point_sample + mpf_select_uncertain (the route of the maps the fused kernel does not take) on one of the same problems"""
    from mp_former_amd import _lib
    from mp_former_amd.point_sample import point_sample_offsets, select_uncertain
    hw, M, k, seed = LR.SELECT_CASES[2]
    planes, coords = LR.select_problem(hw, M, seed)
    keys = LR.point_sample(planes, coords).abs()
    pd, cd = planes.to(DEV), coords.to(DEV)
    offs = (torch.arange(LR.SELECT_ROWS, device=DEV) * hw[0] * hw[1]).long()
    logits = point_sample_offsets(pd.data_ptr(), BF16, hw[0], hw[1], offs, cd, None, DEV)
    assert _lib.last_kernel() == "point_sample_kernel<bf16>", _lib.last_kernel()
    lo, hi = float(planes.min()), float(planes.max())
    _hold("point_sample_kernel<bf16>", f"logits {hw[0]}x{hw[1]}", logits, LR.point_sample(planes, coords), 0.0, _sample_atol(*hw, lo, hi))
    out = select_uncertain(logits, cd, k, k).cpu()
    assert _lib.last_kernel() == "select_uncertain_kernel", _lib.last_kernel()
    for r in range(LR.SELECT_ROWS):
        LR.check_selection(LR.coords_to_index(coords[r], out[r]), keys[r], k)


def test_sample_select_with_a_third_of_the_candidates_outside_the_plane():
    """all of them tie at key 0: for k up to their count the output is exactly the first k of them by index (need_eq < count),
    above it they all come first among the entries below the threshold"""
    oc = LR.OUTSIDE_CASE
    planes, coords = LR.select_problem(oc["hw"], oc["M"], oc["seed"], zeros=oc["zeros"])
    keys = LR.point_sample(planes, coords).abs()
    for k in oc["ks"]:
        out = _sample_select(planes, coords, k)
        for r in range(LR.SELECT_ROWS):
            idx = LR.coords_to_index(coords[r], out[r, :k])
            if k <= oc["zeros"]:
                assert idx.tolist() == list(range(0, 3 * k, 3)), (k, r)
            else:
                LR.check_selection(idx, keys[r], k)


@pytest.mark.parametrize("M", [700, 5000])         # fewer entries than threads (empty slices) / 5 per thread with a short last slice
def test_select_uncertain_exact_order_with_planted_ties(M):
    """given values, so nothing is left to rounding: the output is coords_in[select_order] exactly, and [:, k:] keeps its fill"""
    from mp_former_amd import _lib
    g = torch.Generator().manual_seed(12)
    n = 3
    vals = torch.round(torch.randn(n, M, generator=g) * 8) / 8          # multiples of 1/8 of both signs: ties at every threshold
    vals[0, 3], vals[0, 7], vals[0, 600] = 0.0, -0.0, -0.0
    vals[1] = vals[1].abs() + 0.125                                      # no zero at all
    vals[1, 5], vals[1, 650] = -0.0, 0.0                                 # ... but these two: -0.0 first
    vals[2, :] = torch.where(torch.arange(M) % 2 == 0, torch.tensor(1.5), torch.tensor(-1.5))     # every entry ties
    assert bool((vals == 0).any()) and bool(torch.signbit(vals[1, 5]))
    coords = torch.rand(n, M, 2, generator=g)
    vd, cd = vals.to(DEV), coords.to(DEV)
    for k in (1, 2, 3, 40, M // 4, M - 1, M):
        out = torch.full((n, k + 2, 2), SENT, dtype=F32, device=DEV)
        _lib.call("mpf_select_uncertain", DEV, vd.data_ptr(), cd.data_ptr(), out.data_ptr(), n, M, k, k + 2, _lib.stream_ptr(DEV))
        assert _lib.last_kernel() == "select_uncertain_kernel", _lib.last_kernel()
        out = out.cpu()
        want = LR.select_order(vals, k)
        for r in range(n):
            assert torch.equal(out[r, :k], coords[r, want[r]]), (k, r)
        assert (out[:, k:] == SENT).all(), "coords_out[:, k:] was written"


# ---- mask-loss sums and gradient ----------------------------------------------------------------------------------------------------
SLOTS = 8
PAIR_SLOTS = [5, 0, 3, 6, 2]                # the planes of the pairs, out of SLOTS; the other planes belong to no pair


def _loss_problem(dtype, hw, P, n, packed, seed=13):
    """n pairs on n of SLOTS planes; with n = 5, pair 3 has an all-zero grad_sums row and every point of pair 4 lies wholly
    outside the plane.  Coordinates in [-0.1, 1.1]."""
    from mp_former_amd.matcher import GTMasks
    from mp_former_amd.point_sample import MapSet
    g = torch.Generator().manual_seed(seed)
    (h, w), (H, W) = hw, GT_HW
    maps = (torch.randn(2, SLOTS // 2, h, w, generator=g) * 2).to(dtype)
    gt = torch.rand(6, H, W, generator=g) < 0.4
    slots = np.array(PAIR_SLOTS[:n])
    gr = np.array([4, 0, 5, 2, 1][:n])
    coords = torch.rand(n, P, 2, generator=g) * 1.2 - 0.1
    if P >= 4:
        coords[0, :4] = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.5 / w, 0.5 / h], [1.0 - 0.5 / w, 0.3]])
    gs = torch.tensor([[1.0, -2.0, 0.5, 0.0]]) * torch.arange(1, n + 1)[:, None]
    if n == 5:
        gs[3] = 0.0
        coords[4, :, 0] = 1.3 + 0.3 * torch.rand(P, generator=g)
    md = maps.to(DEV)
    ms = MapSet([md])
    ti, bi, qi = np.zeros(n, np.int64), slots // (SLOTS // 2), slots % (SLOTS // 2)
    gt_d = gt.to(DEV)
    gsrc = GTMasks([{"masks": gt_d}]) if packed else gt_d.view(torch.uint8)
    assert not packed or gsrc.bits is not None
    return {"ms": ms, "maps": md, "po": torch.from_numpy(ms.offsets(ti, bi, qi)).to(DEV), "go": torch.from_numpy(ms.grad_offsets(ti, bi, qi)).to(DEV),
            "gsrc": gsrc, "gt_ptr": (gsrc.bits if packed else gsrc).data_ptr(), "gt_rows": _i32(gr), "coords": coords.to(DEV), "gs": gs.to(DEV),
            "slots": slots.tolist(), "pred_cpu": maps.flatten(0, 1)[slots.tolist()], "gt_cpu": gt[gr.tolist()], "coords_cpu": coords, "gs_cpu": gs,
            "n": n, "P": P, "hw": hw, "dtype": dtype, "packed": packed}


def _backward_dense(p, coords=None, fill=SENT):
    """mpf_mask_loss_backward_dense through the ABI into a buffer of SLOTS planes filled with ``fill`` -> the buffer"""
    from mp_former_amd import _lib
    (h, w), (H, W), dt = p["hw"], GT_HW, _lib.DTYPE[p["dtype"]]
    buf = torch.full((SLOTS, h, w), fill, dtype=p["dtype"], device=DEV)
    coords = p["coords"] if coords is None else coords
    _lib.call("mpf_mask_loss_backward_dense", DEV, p["ms"].base_ptr, dt, h, w, p["po"].data_ptr(), p["gt_ptr"],
              _lib.MPF_BITS if p["packed"] else _lib.MPF_U8, H, W, p["gt_rows"].data_ptr(), coords.data_ptr(), p["gs"].data_ptr(),
              buf.data_ptr(), dt, p["go"].data_ptr(), p["n"], p["P"], _lib.stream_ptr(DEV))
    assert _lib.last_kernel() == f"mask_loss_bwd_band_kernel<{NAME[p['dtype']]}>", _lib.last_kernel()
    return buf


def _hold_grad(route, what, got, ref, dtype):
    _hold(route, what, got, ref, 1e-4, 1e-4, rel_extra=2.0 ** -8 if dtype == BF16 else 0.0)


LOSS_CASES = [((5, 7), 5, 5), ((5, 7), 300, 5), ((5, 7), 1031, 5), ((5, 7), 2500, 5),            # 70-byte bf16 planes: generic forward
              ((32, 32), 5, 5), ((32, 32), 300, 5), ((32, 32), 1031, 5), ((32, 32), 2500, 5),    # LDS forward, one band
              ((256, 256), 1031, 1), ((256, 256), 2500, 1),      # the shipped plane, exactly 128 KiB in bf16: LDS forward, two bands
              ((400, 176), 300, 5), ((400, 176), 2500, 5)]       # above 128 KiB: generic forward; bands of 134 / 134 / 132 rows


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("hw,P,n", LOSS_CASES)
def test_mask_loss_sums_and_gradient_against_fp64(hw, P, n, dtype, packed):
    """P = 5 is below the 8 chunks of the generic forward (empty chunks) and below every block size; 1031 and 2500 are off every
    multiple of them.  The backward runs through the ABI into a sentinel-filled buffer: the planes of the pairs are written whole,
    the others not at all; a zero grad_sums row and a pair with all points outside give all-zero planes; a second run and a run
    on permuted points give the same bits."""
    from mp_former_amd import _lib
    from mp_former_amd.point_sample import MaskLossSums
    p = _loss_problem(dtype, hw, P, n, packed)
    lds = dtype == BF16 and (hw[0] * hw[1] * 2) % 16 == 0 and hw[0] * hw[1] * 2 <= 128 * 1024
    route = "mask_loss_fwd_lds_kernel" if lds else f"mask_loss_fwd_kernel<{NAME[dtype]}>"
    assert lds == (dtype == BF16 and hw in ((32, 32), (256, 256)))
    sums = MaskLossSums.apply(p["ms"], p["po"], p["go"], p["gsrc"], p["gt_rows"], p["coords"], p["maps"])
    assert _lib.last_kernel() == route, _lib.last_kernel()
    _hold(route, f"sums {hw[0]}x{hw[1]} P={P}", sums, LR.mask_loss_sums(p["pred_cpu"], p["gt_cpu"], p["coords_cpu"]), 2e-4, 2e-3)

    buf = _backward_dense(p)
    ref = LR.mask_loss_grad(p["pred_cpu"], p["gt_cpu"], p["coords_cpu"], p["gs_cpu"])
    got = buf.cpu()
    paired = torch.zeros(SLOTS, dtype=torch.bool)
    paired[p["slots"]] = True
    assert (got[~paired] == SENT).all(), "a plane of no pair was written"
    _hold_grad(f"mask_loss_bwd_band_kernel<{NAME[dtype]}>", f"grad {hw[0]}x{hw[1]} P={P}", got[p["slots"]], ref, dtype)
    if n == 5:
        assert (ref[3] == 0).all() and (ref[4] == 0).all()
        assert (got[p["slots"][3]] == 0).all(), "zero grad_sums row: the plane must be written as zeros"
        assert (got[p["slots"][4]] == 0).all(), "every point outside the plane: the plane must be written as zeros"
    assert torch.equal(_backward_dense(p, fill=3.0)[p["slots"]], buf[p["slots"]]), "two runs differ"
    perm = torch.randperm(P, generator=torch.Generator().manual_seed(14)).to(DEV)
    assert torch.equal(_backward_dense(p, coords=p["coords"][:, perm].contiguous()), buf), "a permutation of the points changes the sums"


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_band_backward_holds_240_coincident_full_magnitude_hits(dtype):
    """the documented fixed-point capacity (256 full-magnitude hits on one pixel): 240 points on one pixel centre, logit +12,
    target 0, grad_sums (1, 0, 0): every point adds sigmoid(12) = 0.999994 of the largest possible |d loss / d x|"""
    from mp_former_amd.point_sample import MapSet
    h = w = 32
    P, (H, W) = 240, GT_HW
    maps = torch.full((1, SLOTS, h, w), 12.0, dtype=dtype, device=DEV)
    coords = torch.tensor([(9 + 0.5) / w, (20 + 0.5) / h]).repeat(1, P, 1)              # exact in fp32: pixel (20, 9), fractions 0
    gt = torch.zeros(1, H, W, dtype=torch.uint8, device=DEV)
    ms = MapSet([maps])
    offs = torch.tensor([2 * h * w], dtype=torch.int64, device=DEV)
    gs = torch.tensor([[1.0, 0.0, 0.0, 0.0]])
    p = {"ms": ms, "po": offs, "go": offs, "gt_ptr": gt.data_ptr(), "gt_rows": _i32([0]), "coords": coords.to(DEV), "gs": gs.to(DEV), "n": 1, "P": P,
         "hw": (h, w), "dtype": dtype, "packed": False, "keep": gt}
    got = _backward_dense(p).cpu()
    ref = LR.mask_loss_grad(torch.full((1, h, w), 12.0), torch.zeros(1, H, W), coords, gs)
    assert abs(float(ref[0, 20, 9]) - 240 / (1 + np.exp(-12.0))) < 1e-9 and int((ref != 0).sum()) == 1
    _hold_grad(f"mask_loss_bwd_band_kernel<{NAME[dtype]}>", "240 coincident hits", got[2:3], ref, dtype)
    assert int((got[2] != 0).sum()) == 1 and (got[[0, 1, 3, 4, 5, 6, 7]] == SENT).all()


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("hw", [(5, 7), (32, 32)])
def test_atomic_backward_adds_onto_the_buffer(hw, dtype):
    """mpf_mask_loss_backward: fp32 gradient planes, += with global atomics, byte masks"""
    from mp_former_amd import _lib
    p = _loss_problem(dtype, hw, 1031, 5, False)
    (h, w), (H, W) = hw, GT_HW
    base = torch.randn(SLOTS, h, w, generator=torch.Generator().manual_seed(15))
    buf = base.to(DEV)
    _lib.call("mpf_mask_loss_backward", DEV, p["ms"].base_ptr, _lib.DTYPE[dtype], h, w, p["po"].data_ptr(), p["gt_ptr"], H, W,
              p["gt_rows"].data_ptr(), p["coords"].data_ptr(), p["gs"].data_ptr(), buf.data_ptr(), p["go"].data_ptr(), p["n"], p["P"],
              _lib.stream_ptr(DEV))
    route = f"mask_loss_bwd_kernel<{NAME[dtype]}>"
    assert _lib.last_kernel() == route, _lib.last_kernel()
    got = buf.cpu()
    paired = torch.zeros(SLOTS, dtype=torch.bool)
    paired[p["slots"]] = True
    assert torch.equal(got[~paired], base[~paired]), "a plane of no pair was touched"
    ref = LR.mask_loss_grad(p["pred_cpu"], p["gt_cpu"], p["coords_cpu"], p["gs_cpu"])
    _hold(route, f"base + grad {h}x{w}", got[p["slots"]], base[p["slots"]].double() + ref, 1e-4, 1e-4)
    assert torch.equal(got[p["slots"][3]], base[p["slots"][3]]) and torch.equal(got[p["slots"][4]], base[p["slots"][4]])


@pytest.mark.parametrize("dtype", [BF16, F32])
@pytest.mark.parametrize("packed", [False, True])
def test_mask_loss_sums_planes_equals_mask_loss_sums(dtype, packed):
    """the compact-planes form (its backward writes into an empty_like buffer) == MaskLossSums on the same planes, bit for bit,
    the all-zero plane of the pair with a zero grad_sums row included"""
    from mp_former_amd.point_sample import MapSet, MaskLossSums, MaskLossSumsPlanes
    hw, P = (32, 32), 300
    p = _loss_problem(dtype, hw, P, 5, packed)
    sums = MaskLossSums.apply(p["ms"], p["po"], p["go"], p["gsrc"], p["gt_rows"], p["coords"], p["maps"].requires_grad_(True))
    (sums * p["gs"]).sum().backward()
    g_maps = p["maps"].grad.flatten(0, 1)
    planes = p["maps"].detach().reshape(SLOTS, hw[0] * hw[1]).clone().requires_grad_(True)
    ms = MapSet([planes.view(1, SLOTS, *hw)])
    offs = (torch.tensor(p["slots"], dtype=torch.int64) * hw[0] * hw[1]).to(DEV)
    sums2 = MaskLossSumsPlanes.apply(ms, offs, p["gsrc"], p["gt_rows"], p["coords"], planes)
    assert torch.equal(sums2, sums)
    stale = torch.full_like(planes, SENT)       # so that the gradient's fresh buffer most likely starts from stale non-zero memory
    del stale
    (sums2 * p["gs"]).sum().backward()
    assert torch.equal(planes.grad.view(SLOTS, *hw)[p["slots"]], g_maps[p["slots"]])
    assert (planes.grad[p["slots"][3]] == 0).all()


# ---- bit-packed masks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", [(8, 20), (12, 40), (96, 64)])           # rows of 20 and 40 pixels straddle the 32-pixel words
def test_bit_packed_masks_against_the_restatement(HW):
    from mp_former_amd import _lib
    from mp_former_amd.matcher import GTMasks
    from mp_former_amd.point_sample import point_sample_offsets
    g = torch.Generator().manual_seed(16)
    (H, W), R, P = HW, 5, 1031
    masks = torch.rand(R, H, W, generator=g) < 0.35
    md = masks.to(DEV)
    gtm = GTMasks([{"masks": md[:2]}, {"masks": md[2:]}])
    assert _lib.last_kernel() == "pack_mask_bits_kernel", _lib.last_kernel()
    assert torch.equal(gtm.bits.cpu(), LR.pack_bits(masks))
    coords = torch.rand(2, P, 2, generator=g) * 1.2 - 0.1
    coords[0, :3] = torch.tensor([[0.0, 0.0], [1.0, 1.0], [1.5, -0.5]])
    cd = coords.to(DEV)
    offs = (torch.arange(R, device=DEV) * H * W).long()
    rows = _i32([0, 1, 0, 1, 1])
    a = point_sample_offsets(gtm.u8.data_ptr(), torch.uint8, H, W, offs, cd, rows, DEV)
    assert _lib.last_kernel() == "point_sample_kernel<u8>", _lib.last_kernel()
    b = point_sample_offsets(gtm.bits.data_ptr(), "bits", H, W, offs, cd, rows, DEV)
    assert _lib.last_kernel() == "point_sample_bits_kernel", _lib.last_kernel()
    assert torch.equal(a, b)
    _hold("point_sample_bits_kernel", f"samples {H}x{W}", b, LR.point_sample(masks, coords[[0, 1, 0, 1, 1]]), 0.0,
          _sample_atol(H, W, 0.0, 1.0))


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
def test_image_form_argument_errors_come_before_any_launch():
    """the pointers are never dereferenced: every call here fails a check (or has nothing to do) before it launches"""
    from mp_former_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    DT, SH, TL = -1, -2, -4                     # MPF_E_DTYPE, MPF_E_SHAPE, MPF_E_TOO_LARGE
    bf, u8, bits = _lib.MPF_BF16, _lib.MPF_U8, _lib.MPF_BITS

    def caller(fn, ok):
        return lambda **kw: fn(*{**ok, **kw}.values())

    ps = caller(lib.mpf_point_sample, dict(src=one, dt=bf, h=16, w=24, rows=one, coords=one, crow=None, out=one, n=4, P=100, st=None))
    assert ps(n=65536) == TL and b"65535" in lib.mpf_last_error()
    assert ps(dt=99) == DT and ps(dt=_lib.MPF_F64) == DT and ps(P=0) == SH and ps(n=0) == 0

    fw = caller(lib.mpf_mask_loss_forward, dict(pred=one, dt=bf, h=16, w=24, prow=one, gt=one, gdt=u8, H=5, W=7, grow=one, coords=one,
                                                partial=one, n=4, P=100, chunks=8, st=None))
    assert fw(n=65536) == TL and fw(dt=99) == DT and fw(dt=u8) == DT and fw(gdt=bf) == DT
    assert fw(gdt=bits) == SH and b"% 32" in lib.mpf_last_error()                    # 5 * 7 pixels
    assert fw(chunks=0) == SH and fw(n=0) == 0 and fw(n=0, gdt=bits, H=8, W=20) == 0

    bw = caller(lib.mpf_mask_loss_backward, dict(pred=one, dt=bf, h=16, w=24, prow=one, gt=one, H=5, W=7, grow=one, coords=one, gs=one,
                                                 gp=one, go=one, n=4, P=100, st=None))
    assert bw(n=65536) == TL and bw(dt=99) == DT and bw(dt=u8) == DT and bw(H=0) == SH and bw(n=0) == 0

    bd = caller(lib.mpf_mask_loss_backward_dense, dict(pred=one, dt=bf, h=16, w=24, prow=one, gt=one, gdt=u8, H=5, W=7, grow=one,
                                                       coords=one, gs=one, grad=one, gdt2=bf, go=one, n=4, P=100, st=None))
    assert bd(n=65536) == TL and bd(dt=99, gdt2=99) == DT and bd(gdt2=_lib.MPF_F32) == DT and bd(gdt=bf) == DT
    assert bd(gdt=bits) == SH and bd(w=16385) == TL and bd(n=0) == 0

    assert lib.mpf_pack_mask_bits(one, one, 35, None) == SH and lib.mpf_pack_mask_bits(one, one, 0, None) == 0

    mc = caller(lib.mpf_match_cost, dict(pred=one, dt=bf, h=16, w=24, offs=one, coords=one, crow=one, tsamp=one, first=one, cnt=one,
                                         cost=one, n=12, Tmax=5, P=500, wm=5.0, wd=5.0, group=6, st=None))
    assert mc(P=38401) == TL and b"38400" in lib.mpf_last_error()
    assert mc(dt=99) == DT and mc(dt=u8) == DT and mc(Tmax=0) == SH and mc(n=0) == 0 and mc(n=0, P=38400) == 0

    ss = caller(lib.mpf_sample_select_uncertain, dict(pred=one, dt=bf, h=16, w=24, offs=one, cin=one, cout=one, n=4, M=700, k=100, P_out=103,
                                                      st=None))
    assert ss(M=40961, k=100) == TL and ss(h=264, w=256) == TL and ss(h=5, w=7) == TL
    assert ss(k=701) == SH and ss(P_out=99) == SH and ss(dt=_lib.MPF_F32) == DT and ss(n=0) == 0 and ss(k=0, P_out=0) == 0

    su = caller(lib.mpf_select_uncertain, dict(vals=one, cin=one, cout=one, n=4, M=700, k=100, P_out=103, st=None))
    assert su(k=701) == SH and su(P_out=99) == SH and su(M=0, k=0) == SH and su(n=0) == 0 and su(k=0) == 0
