"""GPU: the clip matching cost kernel (csrc/loss.hip, mpf_match_cost_clip) against the fp64 restatement (tests/_vtrain_restate.py),
and the native VideoHungarianMatcher / VideoSetCriterion (mp_former_amd/video_losses.py) against what the reference's own classes
recorded in tests/golden/vtrain_small.npz, with the reference's random draws replayed."""
import ctypes

import numpy as np
import pytest
import torch

import _vtrain_restate as VR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FILL = -7.0
COUNTS = (3, 0, 11)            # tubes per clip: Tmax = 11 (three target passes of 4 with a tail of 3), one clip without any
W_MASK, W_DICE = 5.0, 5.0
GT_HW = (36, 52)


def _clip_problem(dtype, hw, Q, Fr, P, view, seed=5):
    """-> dict of device tensors for one call: B = 3 clips with COUNTS tubes, one point set per clip"""
    from mp_former_amd.point_sample import MapSet, point_sample_offsets
    from mp_former_amd.video_losses import clip_planes
    g = torch.Generator().manual_seed(seed)
    B, (h, w), (H, W) = len(COUNTS), hw, GT_HW
    Q0 = Q + 3 if view else Q
    parent = (torch.randn(B, Q0, Fr, h, w, generator=g) * 3).to(dtype).to(DEV)
    masks = parent[:, 2:2 + Q] if view else parent                         # a query-slice view of a larger tensor
    gts = [torch.rand(t, Fr, H, W, generator=g) < 0.3 for t in COUNTS]
    gts[0][1, Fr - 1] = False                                               # a tube absent from one frame
    coords = torch.rand(B, P, 2, generator=g)
    ms = MapSet([clip_planes(masks)])
    assert ms.bases[0].data_ptr() == parent.data_ptr()                      # addressed in place, no copy
    b = np.repeat(np.arange(B), Q); q = np.tile(np.arange(Q), B)
    offs = torch.from_numpy(ms.offsets(np.zeros(B * Q, np.int64), b, q * Fr)).to(DEV)
    planes = torch.cat(gts).flatten(0, 1).to(DEV).view(torch.uint8)          # row = tube * F + frame
    n_planes = planes.shape[0]
    clip_of_plane = torch.tensor(np.repeat(np.arange(B), np.array(COUNTS) * Fr), dtype=torch.int32, device=DEV)
    tsamp = point_sample_offsets(planes.data_ptr(), torch.uint8, H, W, (torch.arange(n_planes, device=DEV) * H * W).long(),
                                 coords.to(DEV), clip_of_plane, DEV)         # [Tt*F, P] = [Tt, F*P] frame-major
    firsts = np.concatenate([[0], np.cumsum(COUNTS)[:-1]])
    return {"ms": ms, "offs": offs, "F": Fr, "coords": coords.to(DEV), "crow": torch.from_numpy(b.astype(np.int32)).to(DEV),
            "tsamp": tsamp, "tfirst": torch.from_numpy(firsts[b].astype(np.int32)).to(DEV),
            "tcount": torch.from_numpy(np.array(COUNTS)[b].astype(np.int32)).to(DEV), "Q": Q, "P": P,
            "masks_cpu": masks.float().cpu(), "gts": gts, "coords_cpu": coords}


def _run_clip(p, group):
    """the raw entry point on a cost matrix pre-filled with FILL -> [B, Q, Tmax]"""
    from mp_former_amd import _lib
    ms, n, Tmax = p["ms"], p["offs"].numel(), max(COUNTS)
    cost = torch.full((n, Tmax), FILL, dtype=torch.float32, device=DEV)
    st = _lib.stream_ptr(DEV)
    nbytes = _lib.lib().mpf_match_cost_clip_workspace_bytes(n, p["F"], Tmax)
    assert nbytes == n * p["F"] * (2 + 3 * Tmax) * 4
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.call("mpf_match_cost_clip", DEV, ms.base_ptr, _lib.DTYPE[ms.dtype], ms.h, ms.w, p["offs"].data_ptr(), p["F"], ms.h * ms.w,
              p["coords"].data_ptr(), p["crow"].data_ptr(), p["tsamp"].data_ptr(), p["tfirst"].data_ptr(), p["tcount"].data_ptr(),
              cost.data_ptr(), n, Tmax, p["P"], W_MASK, W_DICE, group, ws.data_ptr(), nbytes, st)
    return cost.view(len(COUNTS), p["Q"], Tmax)


SHAPES = [((9, 13), 7, 3, 500, False),          # the fixture's: 234-byte bf16 planes, never staged in LDS
          ((16, 24), 12, 3, 1100, False),       # LDS form (bf16, grouped), more points than threads
          ((16, 24), 7, 3, 1100, True),         # odd group: the last workgroup of a run has one row; a query-slice view
          ((16, 24), 7, 1, 500, False),         # F = 1: the image kernel's problem
          ((16, 24), 12, 1, 500, False),
          ((16, 24), 7, 2, 9000, False)]        # a frame's logits above 32 KiB: the generic form raises its dynamic LDS limit


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hw,Q,Fr,P,view", SHAPES)
def test_match_cost_clip_matches_the_restatement(hw, Q, Fr, P, view, dtype, grouped):
    """rtol / atol 2e-4: the bound tests/test_loss_kernels_gpu.py holds mpf_match_cost to"""
    from mp_former_amd import _lib
    from mp_former_amd.point_sample import match_cost
    p = _clip_problem(dtype, hw, Q, Fr, P, view)
    group = Q if grouped else 1
    C = _run_clip(p, group)
    lds = dtype == torch.bfloat16 and grouped and (hw[0] * hw[1] * 2) % 16 == 0
    assert ("match_cost_clip_lds_kernel" in _lib.last_kernel()) == lds, _lib.last_kernel()
    assert "match_cost_clip" in _lib.last_kernel()
    assert torch.equal(C, _run_clip(p, group)), "two runs differ"
    C = C.cpu()
    for b, T in enumerate(COUNTS):
        assert (C[b, :, T:] == FILL).all(), "entries t >= t_count were written"
        if T:
            ref = VR.mask_dice_cost(p["masks_cpu"][b], p["gts"][b], p["coords_cpu"][b:b + 1], W_MASK, W_DICE)
            torch.testing.assert_close(C[b, :, :T].double(), ref, rtol=2e-4, atol=2e-4)
    if Fr == 1:
        img = match_cost(p["ms"], p["offs"], p["coords"], p["crow"], p["tsamp"], p["tfirst"], p["tcount"], max(COUNTS), W_MASK, W_DICE,
                         rows_per_group=group).view(len(COUNTS), Q, -1).cpu()
        for b, T in enumerate(COUNTS):
            torch.testing.assert_close(C[b, :, :T], img[b, :, :T], rtol=2e-4, atol=2e-4)


def test_match_cost_clip_argument_errors_come_before_any_launch():
    """the pointers are never dereferenced: every check runs first"""
    from mp_former_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    ok = dict(pred=one, dtype=_lib.MPF_BF16, h=16, w=24, offs=one, F=3, stride_f=384, coords=one, crow=one, tsamp=one, tfirst=one,
              tcount=one, cost=one, n=14, Tmax=11, P=500, wm=5.0, wd=5.0, group=7, ws=one, ws_bytes=10 ** 6, stream=None)

    def call(**kw):
        return lib.mpf_match_cost_clip(*{**ok, **kw}.values())

    need = lib.mpf_match_cost_clip_workspace_bytes(14, 3, 11)
    assert need == 14 * 3 * 35 * 4 and lib.mpf_match_cost_clip_workspace_bytes(0, 3, 11) == 0
    for k in ("pred", "offs", "coords", "crow", "tsamp", "tfirst", "tcount", "cost", "ws"):
        assert call(**{k: None}) == -3, k
    for kw in ({"n": -1}, {"Tmax": 0}, {"P": 0}, {"h": 0}, {"w": -2}, {"F": 0}, {"group": 0}, {"stride_f": 383}):
        assert call(**kw) == -2, kw
    assert call(dtype=_lib.MPF_U8) == -1 and call(dtype=99) == -1 and b"dtype" in lib.mpf_last_error()
    assert call(P=38401) == -4 and call(F=65536, stride_f=384) == -4
    assert call(ws_bytes=need - 1) == -2 and b"workspace" in lib.mpf_last_error()
    assert call(n=0, ws=None, ws_bytes=0) == 0                              # nothing to do, nothing launched


# ---- matcher and criterion against the reference's recorded results ---------------------------------------------------------------
@pytest.fixture(scope="module")
def fx():
    z, cfg, clips, targets, draws = VR.load_fixture()
    return {"z": z, "cfg": cfg, "draws": draws, "targets": [{k: v.to(DEV) for k, v in t.items()} for t in targets]}


def _modules(cfg):
    from mp_former_amd.video_losses import VideoHungarianMatcher, VideoSetCriterion
    m = VideoHungarianMatcher(cost_class=cfg["w_class"], cost_mask=cfg["w_mask"], cost_dice=cfg["w_dice"], num_points=cfg["P"])
    base = {"loss_ce": cfg["w_class"], "loss_mask": cfg["w_mask"], "loss_dice": cfg["w_dice"]}
    wd = dict(base)
    for i in range(cfg["L"] - 1):
        wd.update({k + f"_{i}": v for k, v in base.items()})
    c = VideoSetCriterion(cfg["K"], matcher=m, weight_dict=wd, eos_coef=cfg["eos_coef"], losses=["labels", "masks"],
                          num_points=cfg["P"], oversample_ratio=cfg["oversample"], importance_sample_ratio=cfg["importance"])
    return m, c.to(DEV)


def _outs(fx, variant, grad=False):
    z, cfg = fx["z"], fx["cfg"]
    masks = torch.from_numpy(z["pred_masks"]).to(DEV)
    if variant == "bf16":
        masks = masks.to(torch.bfloat16)
        assert torch.equal(masks.float().cpu(), torch.from_numpy(z["pred_masks_bf16"]))
    logits = torch.from_numpy(z["pred_logits"]).to(DEV)
    if grad:
        masks.requires_grad_(True); logits.requires_grad_(True)
    return masks, logits, [{"pred_logits": logits[l], "pred_masks": masks[l]} for l in range(cfg["L"])]


def _matcher_tags(fx):
    tags = VR.draws_to_tags(fx["draws"], fx["cfg"]["L"], fx["cfg"]["B"])
    return {k: v for k, v in tags.items() if k.startswith("match")}


@pytest.mark.parametrize("variant", ["f32", "bf16"])
def test_matcher_costs_and_every_assignment_equal_the_reference(fx, variant):
    from mp_former_amd import _rng
    from mp_former_amd.lsa import lsa_assign
    z, cfg, targets = fx["z"], fx["cfg"], fx["targets"]
    L, B, Q = cfg["L"], cfg["B"], cfg["Q"]
    matcher, _ = _modules(cfg)
    _, _, outs = _outs(fx, variant)
    try:
        _rng.install_replay(_matcher_tags(fx))
        C = matcher.cost_matrices(outs, targets)
        assert _rng.remaining() == 0
        _rng.install_replay(_matcher_tags(fx))
        host = matcher.match_many(outs, targets)                            # the reference's route: one D2H copy + SciPy
        _rng.install_replay(_matcher_tags(fx))
        first = matcher(outs[0] | {"aux_outputs": outs[1:]}, targets)       # the reference interface: the main output only
    finally:
        _rng.install_replay(None)
    Tmax = max(cfg["tubes"])
    assert C.shape == (L, B, Q, Tmax) and C.dtype == torch.float32
    # the device route: the problems the criterion hands to the solver
    problems, n = [], 0
    for l in range(L):
        for b, T in enumerate(cfg["tubes"]):
            if T:
                problems.append([(l * B + b) * Q * Tmax, Q, T, Tmax, n, 0, 0, 0, 0, 0, 0])
                n += min(Q, T)
    dev = lsa_assign(C, np.asarray(problems, dtype=np.int64), n)
    rows_d, cols_d = dev["rows"].cpu().numpy(), dev["cols"].cpu().numpy()
    Cc, n = C.cpu(), 0
    for l in range(L):
        for b, T in enumerate(cfg["tubes"]):
            i_ref, j_ref = z[f"{variant}_rows"][l, b], z[f"{variant}_cols"][l, b]
            k = min(Q, T)
            assert (i_ref[k:] == -1).all()
            assert np.array_equal(host[l][b][0].numpy(), i_ref[:k]) and np.array_equal(host[l][b][1].numpy(), j_ref[:k]), (l, b)
            if T:
                torch.testing.assert_close(Cc[l, b, :, :T], torch.from_numpy(z[f"{variant}_costs"][l, b, :, :T]), rtol=2e-4, atol=2e-4)
                assert np.array_equal(rows_d[n:n + k], i_ref[:k]) and np.array_equal(cols_d[n:n + k], j_ref[:k]), (l, b)
                n += k
    for b in range(B):
        assert torch.equal(first[b][0], host[0][b][0]) and torch.equal(first[b][1], host[0][b][1])
    assert "VideoHungarianMatcher" in repr(matcher)


@pytest.mark.parametrize("mask_dtype", [torch.bool, torch.uint8, torch.float32])
def test_bit_packed_store_gives_the_costs_of_the_byte_store(fx, mask_dtype):
    """ground truth 32 x 48 = 1536 pixels (a multiple of 32) is kept bit-packed; the samples, and with them the costs, are the
    byte store's exactly.  Masks may come as bool, uint8 or float."""
    from mp_former_amd import _rng
    from mp_former_amd.video_losses import GTTubes
    cfg = fx["cfg"]
    matcher, _ = _modules(cfg)
    _, _, outs = _outs(fx, "f32")
    g = torch.Generator().manual_seed(9)
    masks = [(torch.rand(t, cfg["F"], 32, 48, generator=g) < 0.3).to(DEV) for t in cfg["tubes"]]
    targets = [{"labels": fx["targets"][b]["labels"], "masks": m.to(mask_dtype)} for b, m in enumerate(masks)]
    packed, plain = GTTubes(targets), GTTubes(targets)
    assert packed.bits is not None and packed.counts == list(cfg["tubes"]) and packed.u8.shape[0] == sum(cfg["tubes"]) * cfg["F"]
    plain.bits = None
    got = []
    try:
        for store in (packed, plain):
            _rng.install_replay(_matcher_tags(fx))
            got.append(matcher.cost_matrices(outs, targets, gt=store))
    finally:
        _rng.install_replay(None)
    assert torch.equal(got[0], got[1])
    assert GTTubes(fx["targets"]).bits is None                              # 36 x 52 = 1872 pixels: the byte store


@pytest.mark.parametrize("device_lsa", ["1", "0"])
@pytest.mark.parametrize("variant", ["f32", "bf16"])
def test_criterion_losses_and_gradients_equal_the_reference(fx, variant, device_lsa, monkeypatch):
    """losses rtol 2e-3 / atol 1e-4 and gradients rtol 1e-2 / atol 1e-4 + 5e-3 max|ref|: the bounds of tests/test_head_gpu.py"""
    from mp_former_amd import _rng
    z, cfg, targets = fx["z"], fx["cfg"], fx["targets"]
    monkeypatch.setenv("MPF_DEVICE_LSA", device_lsa)
    _, crit = _modules(cfg)
    masks, logits, outs = _outs(fx, variant, grad=True)
    try:
        _rng.install_replay(VR.draws_to_tags(fx["draws"], cfg["L"], cfg["B"]))
        losses = crit(outs[0] | {"aux_outputs": outs[1:]}, targets)
        assert _rng.remaining() == 0
    finally:
        _rng.install_replay(None)
    names = cfg["loss_names"]
    assert sorted(losses) == names
    got = np.array([float(losses[k]) for k in names])
    print(variant, device_lsa, dict(zip(names, got)), z[f"{variant}_loss_values"])
    np.testing.assert_allclose(got, z[f"{variant}_loss_values"], rtol=2e-3, atol=1e-4)
    total = crit.weighted_total(losses)
    np.testing.assert_allclose(float(total), float(z[f"{variant}_total"]), rtol=2e-3)
    total.backward()
    for name, t in (("grad_masks", masks), ("grad_logits", logits)):
        ref = torch.from_numpy(z[f"{variant}_{name}"])
        assert t.grad.dtype == t.dtype
        torch.testing.assert_close(t.grad.float().cpu(), ref, rtol=1e-2, atol=1e-4 + 5e-3 * float(ref.abs().max()))


def test_batch_without_any_tube(fx):
    from mp_former_amd import _rng
    cfg = fx["cfg"]
    L, B, P = cfg["L"], cfg["B"], cfg["P"]
    _, crit = _modules(cfg)
    masks, logits, outs = _outs(fx, "bf16", grad=True)
    targets = [{"labels": torch.zeros(0, dtype=torch.int64, device=DEV),
                "masks": torch.zeros((0, cfg["F"], *cfg["padded"]), dtype=torch.bool, device=DEV)} for _ in range(B)]
    k = int(cfg["importance"] * P)
    tags = {}
    for sfx in [""] + [f"_{i}" for i in range(L - 1)]:
        tags["match" + sfx] = [torch.rand(1, P, 2) for _ in range(B)]
        tags["loss" + sfx + "_over"] = [torch.zeros(0, int(P * cfg["oversample"]), 2)]
        tags["loss" + sfx + "_rand"] = [torch.zeros(0, P - k, 2)]
    try:
        _rng.install_replay(tags)
        losses = crit(outs[0] | {"aux_outputs": outs[1:]}, targets)
        assert _rng.remaining() == 0
    finally:
        _rng.install_replay(None)
    assert sorted(losses) == cfg["loss_names"]
    for key, v in losses.items():
        assert float(v) == 0.0 if ("mask" in key or "dice" in key) else float(v) > 0.0, key
    crit.weighted_total(losses).backward()
    assert masks.grad is not None and bool((masks.grad == 0).all())         # a gradient path to pred_masks, carrying zero
    assert bool(torch.isfinite(logits.grad).all()) and bool((logits.grad != 0).any())


def test_step_makes_no_device_to_host_copy_on_the_default_route(fx, monkeypatch):
    """forward + backward under torch's synchronisation guard: any blocking copy or .item() raises"""
    cfg, targets = fx["cfg"], fx["targets"]
    monkeypatch.setenv("MPF_DEVICE_LSA", "1")
    _, crit = _modules(cfg)

    def step():
        masks, logits, outs = _outs(fx, "bf16", grad=True)
        losses = crit(outs[0] | {"aux_outputs": outs[1:]}, targets)
        crit.weighted_total(losses).backward()
        return losses

    step()                                                                   # first use: library load, pinned status word
    masks, logits, outs = _outs(fx, "bf16", grad=True)                       # (the uploads of the inputs are outside the guard)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        losses = crit(outs[0] | {"aux_outputs": outs[1:]}, targets)
        crit.weighted_total(losses).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v)) for v in losses.values())
