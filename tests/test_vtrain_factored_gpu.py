"""GPU: clip training from the mask factors (mask_fused.FactoredClipMasks through VideoHungarianMatcher / VideoSetCriterion and the
clip decoder's ``factored_masks``), against the fp64 restatement (tests/_vtrain_restate.py) on the unrounded product of the bf16
factors and against the same criterion on ``materialize()`` of the same factors, with the draws replayed.

B = 3 clips with 3, 0 and 11 tubes, T = 3, Q = 7, L = 2, 8 x 16 maps (T h w = 384), P = 500.  SEED is the first seed of
``_problem`` at which every assignment of the restatement beats its runner-up by at least 1e-2 (the costs of the two routes differ
by the bf16 rounding of the maps, ~2^-9 relative: an assignment that hinges on less could differ between them)."""
import numpy as np
import pytest
import torch

import _vtrain_restate as VR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SEED = 0
MARGIN = 1e-2
COUNTS = (3, 0, 11)
T, Q, L, HW, P, K = 3, 7, 2, (8, 16), 500, 5
GT_HW = (36, 52)
W_CLASS, W_MASK, W_DICE, EOS = 2.0, 5.0, 5.0, 0.1
OVERSAMPLE, IMPORTANCE = 3.0, 0.75
COST_RTOL = COST_ATOL = 2e-4


def _problem(seed, counts=COUNTS, hw=HW, frames=T):
    """CPU tensors: bf16 factors me [B, L * Q, 256] and mf [B * T, 256, h, w] (channel-last memory), class logits, targets and the
    draws in the reference's order"""
    g = torch.Generator().manual_seed(1000 + seed)
    B, (h, w) = len(counts), hw
    me = (torch.randn(B, L * Q, 256, generator=g) * 0.25).to(torch.bfloat16)
    mf = torch.randn(B * frames, h, w, 256, generator=g).to(torch.bfloat16).permute(0, 3, 1, 2)
    logits = torch.randn(L, B, Q, K + 1, generator=g)
    targets = [{"labels": torch.randint(0, K, (c,), generator=g), "masks": torch.rand(c, frames, *GT_HW, generator=g) < 0.4}
               for c in counts]
    k = int(IMPORTANCE * P)
    M = sum(min(Q, c) for c in counts)
    draws = []
    for _ in range(L):
        draws += [torch.rand(1, P, 2, generator=g) for _ in range(B)]
        draws += [torch.rand(M * frames, int(P * OVERSAMPLE), 2, generator=g), torch.rand(M * frames, P - k, 2, generator=g)]
    return {"me": me, "mf": mf, "logits": logits, "targets": targets, "draws": draws, "B": B, "T": frames, "hw": hw}


def _product64(pb):
    """the unrounded product of the bf16 factors, fp64 [B, L * Q, T, h, w]"""
    B, (h, w) = pb["B"], pb["hw"]
    mf5 = pb["mf"].double().view(B, pb["T"], 256, h, w)
    return torch.einsum("bqc,btchw->bqthw", pb["me"].double(), mf5)


def _restate(pb):
    maps = _product64(pb)
    outs = [{"pred_logits": pb["logits"][l].double(), "pred_masks": maps[:, l * Q:(l + 1) * Q]} for l in range(L)]
    outs = [outs[-1]] + outs[:-1]                                     # main output first, then the aux outputs
    return VR.criterion(outs, pb["targets"], pb["draws"], K, W_CLASS, W_MASK, W_DICE, EOS, P, OVERSAMPLE, IMPORTANCE)


@pytest.fixture(scope="module")
def ref():
    pb = _problem(SEED)
    losses, costs, assignments = _restate(pb)
    return {"pb": pb, "losses": losses, "costs": costs, "assignments": assignments}


def _modules():
    from mp_former_amd.video_losses import VideoHungarianMatcher, VideoSetCriterion
    m = VideoHungarianMatcher(cost_class=W_CLASS, cost_mask=W_MASK, cost_dice=W_DICE, num_points=P)
    base = {"loss_ce": W_CLASS, "loss_mask": W_MASK, "loss_dice": W_DICE}
    wd = dict(base)
    for i in range(L - 1):
        wd.update({k + f"_{i}": v for k, v in base.items()})
    c = VideoSetCriterion(K, matcher=m, weight_dict=wd, eos_coef=EOS, losses=["labels", "masks"], num_points=P,
                          oversample_ratio=OVERSAMPLE, importance_sample_ratio=IMPORTANCE)
    return m, c.to(DEV)


def _leaves(pb, grad=True):
    """-> (me, mf, mf4, logits) on the device: mf4 the clip as one tall image, a view of the channel-last mf"""
    B, (h, w), Fr = pb["B"], pb["hw"], pb["T"]
    me = pb["me"].to(DEV).requires_grad_(grad)
    mf = pb["mf"].to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(grad)
    mf4 = mf.view(B, Fr, 256, h, w).permute(0, 2, 1, 3, 4).reshape(B, 256, Fr * h, w)
    assert mf4.data_ptr() == mf.data_ptr()
    logits = pb["logits"].to(DEV).requires_grad_(grad)
    return me, mf, mf4, logits


def _outs(pb, logits, masks_of_layer):
    outs = [{"pred_logits": logits[l], "pred_masks": masks_of_layer(l)} for l in range(L)]
    return [outs[-1]] + outs[:-1]


def _factored_outs(pb, me, mf4, logits):
    from mp_former_amd.mask_fused import FactoredClipMasks
    whole = FactoredClipMasks(me, mf4, pb["T"])
    return _outs(pb, logits, lambda l: whole[:, l * Q:(l + 1) * Q])


def _materialised_outs(pb, me, mf4, logits):
    from mp_former_amd.mask_fused import FactoredClipMasks
    parent = FactoredClipMasks(me, mf4, pb["T"]).materialize()
    return _outs(pb, logits, lambda l: parent[:, l * Q:(l + 1) * Q])


def _targets(pb):
    return [{k: v.to(DEV) for k, v in t.items()} for t in pb["targets"]]


def _tags(pb):
    return VR.draws_to_tags(pb["draws"], L, pb["B"])


def _run(crit, outs, targets, tags):
    from mp_former_amd import _rng
    try:
        _rng.install_replay(tags)
        losses = crit(outs[0] | {"aux_outputs": outs[1:]}, targets)
        assert _rng.remaining() == 0
    finally:
        _rng.install_replay(None)
    return losses


def test_the_recorded_seed_keeps_every_assignment_clear_of_its_runner_up(ref):
    margins = [VR.second_best_margin(c) for cur in ref["costs"] for c in cur if c is not None]
    print("margins", margins)
    assert len(margins) == L * 2 and min(margins) >= MARGIN


def test_cost_matrices_from_factors_equal_the_restatement(ref):
    from mp_former_amd import _lib, _rng
    from mp_former_amd.lsa import lsa_assign
    pb = ref["pb"]
    matcher, _ = _modules()
    me, mf, mf4, logits = _leaves(pb, grad=False)
    outs, targets = _factored_outs(pb, me, mf4, logits), _targets(pb)
    tags = {k: v for k, v in _tags(pb).items() if k.startswith("match")}
    try:
        _rng.install_replay(tags)
        C = matcher.cost_matrices(outs, targets)
        assert _rng.remaining() == 0 and _lib.last_kernel() == "match_cost_fused_kernel"
        _rng.install_replay(tags)
        host = matcher.match_many(outs, targets)
    finally:
        _rng.install_replay(None)
    B, Tmax = pb["B"], max(COUNTS)
    assert C.shape == (L, B, Q, Tmax) and C.dtype == torch.float32
    problems, n = [], 0
    for l in range(L):
        for b, Tn in enumerate(COUNTS):
            if Tn:
                problems.append([(l * B + b) * Q * Tmax, Q, Tn, Tmax, n, 0, 0, 0, 0, 0, 0])
                n += min(Q, Tn)
    dev = lsa_assign(C, np.asarray(problems, dtype=np.int64), n)
    rows_d, cols_d = dev["rows"].cpu().numpy(), dev["cols"].cpu().numpy()
    Cc, n = C.cpu().double(), 0
    for l in range(L):
        for b, Tn in enumerate(COUNTS):
            i_ref, j_ref = ref["assignments"][l][b]
            assert np.array_equal(host[l][b][0].numpy(), i_ref) and np.array_equal(host[l][b][1].numpy(), j_ref), (l, b)
            if Tn:
                want = torch.from_numpy(ref["costs"][l][b])
                err = (Cc[l, b, :, :Tn] - want).abs()
                print(f"cost l={l} b={b} max abs err {float(err.max()):.3e}")
                assert bool((err <= COST_ATOL + COST_RTOL * want.abs()).all()), (l, b, float(err.max()))
                k = min(Q, Tn)
                assert np.array_equal(rows_d[n:n + k], i_ref) and np.array_equal(cols_d[n:n + k], j_ref), (l, b)
                n += k


def _no_product(monkeypatch):
    from mp_former_amd import mask_fused

    def boom(*a, **k):
        raise AssertionError("the factored step formed the full product")

    monkeypatch.setattr(mask_fused.FactoredClipMasks, "materialize", boom)
    monkeypatch.setattr(mask_fused, "full_product", boom)


@pytest.mark.parametrize("device_lsa", ["1", "0"])
def test_criterion_on_factors_equals_the_materialised_route_and_the_restatement(ref, device_lsa, monkeypatch):
    """losses of the two routes rtol 1e-5 (the planes are the same kernel's bits), gradients rtol 1e-2 / atol 1e-4 + 5e-3 max|ref|,
    losses against fp64 rtol 2e-3 / atol 1e-4 (the bounds of tests/test_vtrain_gpu.py)"""
    pb = ref["pb"]
    monkeypatch.setenv("MPF_DEVICE_LSA", device_lsa)
    matcher, crit = _modules()
    targets, tags = _targets(pb), _tags(pb)
    # the materialised route first (it needs the product)
    me_m, mf_m, mf4_m, lg_m = _leaves(pb)
    want = _run(crit, _materialised_outs(pb, me_m, mf4_m, lg_m), targets, tags)
    crit.weighted_total(want).backward()
    # same pairs: the host route of the matcher on both forms
    from mp_former_amd import _rng
    me, mf, mf4, lg = _leaves(pb)
    mtags = {k: v for k, v in tags.items() if k.startswith("match")}
    try:
        _rng.install_replay(mtags)
        pairs_f = matcher.match_many(_factored_outs(pb, me, mf4, lg), targets)
        _rng.install_replay(mtags)
        pairs_m = matcher.match_many(_materialised_outs(pb, me_m.detach(), mf4_m.detach(), lg_m.detach()), targets)
    finally:
        _rng.install_replay(None)
    for l in range(L):
        for b in range(pb["B"]):
            assert torch.equal(pairs_f[l][b][0], pairs_m[l][b][0]) and torch.equal(pairs_f[l][b][1], pairs_m[l][b][1]), (l, b)
    # the factored step: the product must never be formed
    with monkeypatch.context() as mp:
        _no_product(mp)
        got = _run(crit, _factored_outs(pb, me, mf4, lg), targets, tags)
        crit.weighted_total(got).backward()
    assert sorted(got) == sorted(want)
    for k in sorted(got):
        print(k, float(got[k]), float(want[k]), float(ref["losses"][k]))
        torch.testing.assert_close(got[k].float(), want[k].float(), rtol=1e-5, atol=0, msg=k)
        np.testing.assert_allclose(float(got[k]), float(ref["losses"][k]), rtol=2e-3, atol=1e-4, err_msg=k)
        if k.startswith("loss_ce"):
            assert float(got[k]) == float(want[k]), "the class targets (the pairs) differ"
    for name, a, b in (("me", me, me_m), ("mf", mf, mf_m), ("logits", lg, lg_m)):
        assert a.grad is not None and a.grad.dtype == a.dtype and a.grad.shape == a.shape, name
        r = b.grad.float()
        assert float(r.abs().max()) > 0, name
        torch.testing.assert_close(a.grad.float(), r, rtol=1e-2, atol=1e-4 + 5e-3 * float(r.abs().max()), msg=name)


def test_factored_step_makes_no_device_to_host_copy_on_the_default_route(ref, monkeypatch):
    pb = ref["pb"]
    monkeypatch.setenv("MPF_DEVICE_LSA", "1")
    _, crit = _modules()
    targets = _targets(pb)

    def step(sync):
        me, mf, mf4, lg = _leaves(pb)
        outs = _factored_outs(pb, me, mf4, lg)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode(sync)
        try:
            losses = crit(outs[0] | {"aux_outputs": outs[1:]}, targets)
            crit.weighted_total(losses).backward()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        return losses, (me, mf, lg)

    step("default")                                                   # first use: library load, pinned status word, scratch
    with monkeypatch.context() as mp:
        _no_product(mp)
        losses, leaves = step("error")
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    assert all(t.grad is not None and bool(torch.isfinite(t.grad.float()).all()) for t in leaves)


def _fallback_agrees(pb, monkeypatch, expect_zero_masks=False):
    """the criterion handed factors it cannot take evaluates them and gives what it gives on the evaluated tensors"""
    from mp_former_amd import mask_fused
    _, crit = _modules()
    targets, tags = _targets(pb), _tags(pb)
    me_m, mf_m, mf4_m, lg_m = _leaves(pb)
    want = _run(crit, _materialised_outs(pb, me_m, mf4_m, lg_m), targets, tags)
    crit.weighted_total(want).backward()
    calls = []
    real = mask_fused.FactoredClipMasks.materialize
    monkeypatch.setattr(mask_fused.FactoredClipMasks, "materialize", lambda self: calls.append(1) or real(self))
    me, mf, mf4, lg = _leaves(pb)
    got = _run(crit, _factored_outs(pb, me, mf4, lg), targets, tags)
    crit.weighted_total(got).backward()
    for k in sorted(want):
        torch.testing.assert_close(got[k].float(), want[k].float(), rtol=1e-5, atol=0, msg=k)
    for name, a, b in (("me", me, me_m), ("mf", mf, mf_m)):
        r = b.grad.float()
        assert a.grad is not None, name
        torch.testing.assert_close(a.grad.float(), r, rtol=1e-2, atol=1e-4 + 5e-3 * float(r.abs().max()), msg=name)
        if expect_zero_masks:
            assert bool((a.grad == 0).all()), name
    return calls, got


def test_fallback_129_tubes_in_one_clip(monkeypatch):
    calls, _ = _fallback_agrees(_problem(1, counts=(2, 129, 0)), monkeypatch)
    assert len(calls) == L


def test_fallback_maps_the_native_product_does_not_take(monkeypatch):
    """T h w = 30"""
    from mp_former_amd import mask_fused
    pb = _problem(2, hw=(2, 5))
    me, mf, mf4, _ = _leaves(pb, grad=False)
    assert pb["T"] * 2 * 5 == 30 and not mask_fused.supported(me, mf4)
    calls, _ = _fallback_agrees(pb, monkeypatch)
    assert len(calls) == L


def test_batch_without_any_tube_gives_a_zero_that_depends_on_both_factors(monkeypatch):
    pb = _problem(3, counts=(0, 0, 0))
    _, crit = _modules()
    me, mf, mf4, lg = _leaves(pb)
    with monkeypatch.context() as mp:
        _no_product(mp)
        losses = _run(crit, _factored_outs(pb, me, mf4, lg), _targets(pb), _tags(pb))
        crit.weighted_total(losses).backward()
    for key, v in losses.items():
        assert float(v) == 0.0 if ("mask" in key or "dice" in key) else float(v) > 0.0, key
    for t in (me, mf):
        assert t.grad is not None and bool((t.grad == 0).all())
    assert bool((lg.grad != 0).any())


@pytest.mark.parametrize("factored", [True, False])
def test_decoder_hands_over_factors_only_when_asked(factored):
    import json
    import os
    import _vdec_common as V
    from conftest import GOLDEN
    from mp_former_amd.mask_fused import FactoredClipMasks
    from mp_former_amd.video_decoder import VideoMultiScaleMaskedTransformerDecoder
    name = "vdec_small"
    z, cfg = np.load(os.path.join(GOLDEN, name + ".npz")), V.CONFIGS[name]
    m = VideoMultiScaleMaskedTransformerDecoder(**V.module_kwargs(cfg))
    m.load_state_dict(V.DP.det_state_dict(json.loads(str(z["param_names"])), name + "."), strict=True)
    m = m.to(DEV).train()
    assert m.factored_masks is False
    m.factored_masks = factored
    B, Fr = cfg["B"], cfg["num_frames"]
    xs, mf = V.inputs(name, cfg, 0, B, Fr)
    cl = lambda v: v.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # noqa: E731
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = m([cl(x) for x in xs], cl(mf))
    masks = [out["pred_masks"]] + [a["pred_masks"] for a in out["aux_outputs"]]
    assert len(masks) == cfg["dec_layers"] + 1
    shape = (B, cfg["Q"], Fr) + tuple(cfg["mf"])
    if factored:
        assert all(isinstance(mk, FactoredClipMasks) and mk.same_factors(masks[0]) and mk.shape == shape for mk in masks)
        assert sorted(mk.q0 for mk in masks) == [l * cfg["Q"] for l in range(len(masks))]
        assert masks[0].mf.shape == (B, 256, Fr * cfg["mf"][0], cfg["mf"][1]) and masks[0].T == Fr
    else:
        assert all(torch.is_tensor(mk) and mk.shape == shape for mk in masks)
        assert len({mk._base.data_ptr() for mk in masks}) == 1
