"""CPU: the restatement of the clip losses (tests/_vtrain_restate.py) reproduces what the reference's own VideoHungarianMatcher,
VideoSetCriterion and prepare_targets recorded in tests/golden/vtrain_small.npz; prepare_video_targets equals the reference's
targets; install_native_video_training carries every field over; the draw tags and shapes are the captured ones."""
import json
import types

import numpy as np
import pytest
import torch

import _vtrain_restate as VR


@pytest.fixture(scope="module")
def fx():
    return VR.load_fixture()


def _restated(fx, variant):
    z, cfg, _, targets, draws = fx
    outs = [{k: v.double().requires_grad_(True) for k, v in o.items()} for o in VR.fixture_outs(z, cfg, variant)]
    losses, costs, assignments = VR.criterion(outs, targets, draws, cfg["K"], cfg["w_class"], cfg["w_mask"], cfg["w_dice"],
                                              cfg["eos_coef"], cfg["P"], cfg["oversample"], cfg["importance"])
    return outs, losses, costs, assignments


@pytest.mark.parametrize("variant", ["f32", "bf16"])
def test_restatement_reproduces_the_reference(fx, variant):
    z, cfg = fx[0], fx[1]
    outs, losses, costs, assignments = _restated(fx, variant)
    for l in range(cfg["L"]):
        for b, T in enumerate(cfg["tubes"]):
            if T == 0:
                assert costs[l][b] is None and (z[f"{variant}_rows"][l, b] == -1).all()
                continue
            ref = z[f"{variant}_costs"][l, b, :, :T]
            # fp64 against the fp32 reference: costs are O(1..10), fp32 sums of 1500 terms
            np.testing.assert_allclose(costs[l][b], ref, rtol=0, atol=1e-6 * max(1.0, float(np.abs(ref).max())))
            assert np.isnan(z[f"{variant}_costs"][l, b, :, T:]).all()
            k = min(cfg["Q"], T)
            assert np.array_equal(assignments[l][b][0], z[f"{variant}_rows"][l, b, :k])
            assert np.array_equal(assignments[l][b][1], z[f"{variant}_cols"][l, b, :k])
            # the fixture's promise: every problem beats its second-best assignment by >= 1e-2
            assert VR.second_best_margin(ref) >= 1e-2
    names = cfg["loss_names"]
    assert sorted(losses) == names and len(names) == 3 * cfg["L"]
    np.testing.assert_allclose([float(losses[k].detach()) for k in names], z[f"{variant}_loss_values"], rtol=1e-5)
    by_kind = {"ce": cfg["w_class"], "mask": cfg["w_mask"], "dice": cfg["w_dice"]}
    weights = {k: by_kind[k.split("_")[1]] for k in names}
    total = sum(losses[k] * weights[k] for k in names)
    np.testing.assert_allclose(float(total.detach()), float(z[f"{variant}_total"]), rtol=1e-5)
    total.backward()
    for l, o in enumerate(outs):
        for key, name in (("pred_masks", "grad_masks"), ("pred_logits", "grad_logits")):
            ref = z[f"{variant}_{name}"][l]
            np.testing.assert_allclose(o[key].grad.numpy(), ref, rtol=1e-4, atol=1e-6 * float(np.abs(ref).max()) + 1e-9)


def test_cost_is_additive_over_frames_with_one_shared_point_set(fx):
    """what the kernel relies on: the five sums of a tube are the sums of its frames' sums"""
    z, cfg, _, targets, draws = fx
    o = VR.fixture_outs(z, cfg, "f32")[0]
    masks, tgt, coords = o["pred_masks"][2].double(), targets[2]["masks"].double(), draws[2].double()
    Fr = cfg["F"]
    x = torch.stack([VR.point_sample(masks[:, f:f + 1], coords.expand(masks.shape[0], -1, -1))[:, 0] for f in range(Fr)])
    t = torch.stack([VR.point_sample(tgt[:, f:f + 1], coords.expand(tgt.shape[0], -1, -1))[:, 0] for f in range(Fr)])
    sp = torch.nn.functional.softplus(x).sum(-1).sum(0)
    s = x.sigmoid()
    sx, ss = torch.einsum("fqp,fgp->qg", x, t), torch.einsum("fqp,fgp->qg", s, t)
    n = Fr * cfg["P"]
    cost = cfg["w_mask"] * (sp[:, None] - sx) / n + cfg["w_dice"] * (1 - (2 * ss + 1) / (s.sum(-1).sum(0)[:, None] + t.sum(-1).sum(0)[None] + 1))
    ref = VR.mask_dice_cost(masks, tgt, coords, cfg["w_mask"], cfg["w_dice"])
    torch.testing.assert_close(cost, ref, rtol=1e-12, atol=1e-12)


def test_prepare_video_targets_equals_the_reference(fx):
    from mp_former_amd.video_losses import prepare_video_targets
    _, cfg, clips, targets, _ = fx
    for c, ref in zip(clips, targets):
        Fr = cfg["F"]
        for got in (prepare_video_targets([c["masks"][f] for f in range(Fr)], [c["ids"][f] for f in range(Fr)], c["classes"][-1],
                                          cfg["padded"]),
                    VR.prepare_targets([c["masks"][f] for f in range(Fr)], [c["ids"][f] for f in range(Fr)], c["classes"][-1],
                                       cfg["padded"])):
            assert got["masks"].dtype == torch.bool and tuple(got["masks"].shape[1:]) == (Fr, *cfg["padded"])
            for k in ("labels", "ids", "masks"):
                assert torch.equal(got[k], ref[k]), k
    assert [len(t["labels"]) for t in targets] == cfg["tubes"]
    assert not targets[0]["masks"][1, 1].any() and int(targets[0]["ids"][1, 1]) == -1      # the tube absent from one frame


def test_install_native_video_training_copies_every_field():
    from mp_former_amd import d2_plugin
    from mp_former_amd.video_losses import VideoHungarianMatcher, VideoSetCriterion
    old_matcher = types.SimpleNamespace(cost_class=2.0, cost_mask=5.0, cost_dice=4.0, num_points=123)
    wd = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 4.0, "loss_ce_0": 2.0}
    old = types.SimpleNamespace(num_classes=40, matcher=old_matcher, weight_dict=wd, eos_coef=0.1, losses=["labels", "masks"],
                                num_points=123, oversample_ratio=3.0, importance_sample_ratio=0.75, empty_weight=torch.ones(41),
                                training=True)
    forward = object()
    model = types.SimpleNamespace(criterion=old, device=torch.device("cpu"), forward=forward, prepare_targets=None)
    crit = d2_plugin.install_native_video_training(model)
    assert model.criterion is crit and isinstance(crit, VideoSetCriterion) and isinstance(crit.matcher, VideoHungarianMatcher)
    assert model.forward is forward                                          # the eval branch is not routed anywhere
    m = crit.matcher
    assert (m.cost_class, m.cost_mask, m.cost_dice, m.num_points) == (2.0, 5.0, 4.0, 123)
    assert (crit.num_classes, crit.weight_dict, crit.eos_coef, crit.losses) == (40, wd, 0.1, ["labels", "masks"])
    assert (crit.num_points, crit.oversample_ratio, crit.importance_sample_ratio) == (123, 3.0, 0.75)
    assert crit.empty_weight.shape == (41,) and float(crit.empty_weight[-1]) == pytest.approx(0.1) and crit.training
    assert "VideoSetCriterion" in repr(crit) and "VideoHungarianMatcher" in repr(crit) and "cost_dice: 4.0" in repr(crit)
    # the new prepare_targets: per-frame instances -> prepare_video_targets with the padded size of the image list
    frame = lambda ids, cls, masks: types.SimpleNamespace(  # noqa: E731
        gt_ids=ids, gt_classes=cls, gt_masks=types.SimpleNamespace(tensor=masks), to=lambda dev: frame(ids, cls, masks))
    masks = torch.rand(2, 2, 5, 6) < 0.5
    video = {"instances": [frame(torch.tensor([3, -1]), torch.tensor([9, 9]), masks[0]),
                           frame(torch.tensor([3, -1]), torch.tensor([1, 2]), masks[1])]}
    out = model.prepare_targets([video], types.SimpleNamespace(tensor=torch.zeros(2, 3, 8, 8)))
    assert len(out) == 1 and out[0]["labels"].tolist() == [1] and out[0]["ids"].tolist() == [[3, 3]]
    assert out[0]["masks"].shape == (1, 2, 8, 8) and torch.equal(out[0]["masks"][0, :, :5, :6], masks[:, 0])
    assert not out[0]["masks"][..., 5:, :].any() and not out[0]["masks"][..., 6:].any()


def test_draw_tags_and_shapes_equal_the_captured_spec(fx):
    """per output: B matcher point sets (1, P, 2), then (M*F, 3P, 2) and (M*F, P-k, 2) — the order video_losses.py tags them in"""
    z, cfg, _, _, draws = fx
    spec = json.loads(str(z["rng_spec"]))
    assert all(s[0] == "rand" and s[2] == "float32" for s in spec)
    tags = VR.draws_to_tags(draws, cfg["L"], cfg["B"])
    P, Fr = cfg["P"], cfg["F"]
    M = sum(min(cfg["Q"], t) for t in cfg["tubes"])
    k = int(cfg["importance"] * P)
    assert list(tags) == ["match", "loss_over", "loss_rand", "match_0", "loss_0_over", "loss_0_rand"]
    for sfx in ("", "_0"):
        assert [tuple(t.shape) for t in tags["match" + sfx]] == [(1, P, 2)] * cfg["B"]
        assert [tuple(t.shape) for t in tags["loss" + sfx + "_over"]] == [(M * Fr, int(P * cfg["oversample"]), 2)]
        assert [tuple(t.shape) for t in tags["loss" + sfx + "_rand"]] == [(M * Fr, P - k, 2)]
