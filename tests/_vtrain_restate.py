"""The losses of a clip restated in torch (fp64 by default), in this project's own words: what
mask2former_video/video_maskformer_model.py:227-253 (targets), modeling/matcher.py:96-156 (matching cost + assignment) and
modeling/criterion.py:122-243 (losses) compute, with the random draws handed in as a list in the order the reference makes them:
per decoder output (main first, then each aux) one (1, P, 2) point set per clip for the matcher, then the (M*F, 3P, 2)
oversampled and the (M*F, P-k, 2) random loss points.  tests/test_vtrain_cpu.py holds it to the reference's recorded results
(tests/golden/vtrain_small.npz); tests/test_vtrain_gpu.py holds the native kernels to it at other shapes."""
import numpy as np
import torch
import torch.nn.functional as F
from scipy.optimize import linear_sum_assignment


def point_sample(x, coords):
    """x [N, C, H, W], coords [N, P, 2] in [0, 1] (x, y) -> [N, C, P]: bilinear, zeros outside, align_corners=False"""
    return F.grid_sample(x, 2.0 * coords.unsqueeze(2) - 1.0, mode="bilinear", padding_mode="zeros", align_corners=False).squeeze(3)


def prepare_targets(frame_masks, frame_ids, classes, padded_hw):
    """F x [G, h_f, w_f] masks, F x [G] ids, [G] classes -> labels [G'], ids [G', F], masks [G', F, H, W] bool: every frame
    zero-padded at the bottom / right, instances with id -1 in all frames dropped."""
    G, H, W = frame_masks[0].shape[0], padded_hw[0], padded_hw[1]
    masks = torch.zeros(G, len(frame_masks), H, W, dtype=torch.bool)
    for f, m in enumerate(frame_masks):
        masks[:, f, :m.shape[1], :m.shape[2]] = m.bool()
    ids = torch.stack(list(frame_ids), 1)
    keep = (ids != -1).any(1)
    return {"labels": classes[keep], "ids": ids[keep], "masks": masks[keep]}


def mask_dice_cost(masks, tgt, coords, w_mask, w_dice, dtype=torch.float64):
    """masks [Q, F, h, w] logits, tgt [G, F, H, W] 0/1, coords [1, P, 2]: the frames are channels, so one point set serves all
    of them and both sums run over the F*P samples -> w_mask * BCE cost + w_dice * dice cost, [Q, G]"""
    c = coords.to(dtype)
    x = point_sample(masks.to(dtype), c.expand(masks.shape[0], -1, -1)).flatten(1)          # [Q, F*P] frame-major
    t = point_sample(tgt.to(dtype), c.expand(tgt.shape[0], -1, -1)).flatten(1)              # [G, F*P]
    cm = (F.softplus(-x) @ t.T + F.softplus(x) @ (1 - t).T) / x.shape[1]
    s = x.sigmoid()
    cd = 1 - (2 * s @ t.T + 1) / (s.sum(1)[:, None] + t.sum(1)[None, :] + 1)
    return w_mask * cm + w_dice * cd


def matcher_cost(logits, masks, labels, tgt, coords, w_class, w_mask, w_dice, dtype=torch.float64):
    """+ the class cost -softmax(logits)[:, labels]; logits [Q, K+1] -> [Q, G]"""
    return mask_dice_cost(masks, tgt, coords, w_mask, w_dice, dtype) - w_class * logits.to(dtype).softmax(-1)[:, labels]


def assign(C):
    i, j = linear_sum_assignment(np.asarray(C))
    return i.astype(np.int64), j.astype(np.int64)


def second_best_margin(C):
    """How much the best assignment of C beats every other one by: re-solve with each matched edge forbidden in turn and take the
    smallest increase of the total (an assignment differs from the best one in at least one of its edges)."""
    C = np.asarray(C, dtype=np.float64)
    i, j = linear_sum_assignment(C)
    best = C[i, j].sum()
    margin = np.inf
    for r, c in zip(i, j):
        D = C.copy()
        D[r, c] = 1e9
        i2, j2 = linear_sum_assignment(D)
        margin = min(margin, D[i2, j2].sum() - best)
    return margin


def draws_to_tags(draws, L, B):
    """the FIFO of the reference's draws -> the tagged draws of mp_former_amd._rng"""
    q = list(draws)
    tags = {}
    for sfx in [""] + [f"_{i}" for i in range(L - 1)]:
        tags["match" + sfx] = [q.pop(0) for _ in range(B)]
        tags["loss" + sfx + "_over"] = [q.pop(0)]
        tags["loss" + sfx + "_rand"] = [q.pop(0)]
    assert not q, f"{len(q)} unconsumed draws"
    return tags


def criterion(outs, targets, draws, num_classes, w_class, w_mask, w_dice, eos_coef, P, oversample, importance, dtype=torch.float64):
    """outs: list (main, aux 0, ...) of {"pred_logits" [B, Q, K+1], "pred_masks" [B, Q, F, h, w]}; targets: list of
    {"labels", "masks" [G, F, H, W]} -> (losses dict with the reference's keys, costs[l][b] ([Q, G] or None), assignments[l][b])"""
    q = list(draws)
    B, Q = outs[0]["pred_logits"].shape[:2]
    dev = outs[0]["pred_logits"].device
    num_masks = max(float(sum(len(t["labels"]) for t in targets)), 1.0)                     # tubes, one process
    weight = torch.ones(num_classes + 1, dtype=dtype, device=dev)
    weight[-1] = eos_coef
    k_unc = int(importance * P)
    losses, costs, assignments = {}, [], []
    for sfx, o in zip([""] + [f"_{i}" for i in range(len(outs) - 1)], outs):
        logits, masks = o["pred_logits"].to(dtype), o["pred_masks"].to(dtype)
        cur_c, cur_a = [], []
        for b in range(B):
            coords = q.pop(0)
            if len(targets[b]["labels"]) == 0:
                cur_c.append(None)
                cur_a.append((np.zeros(0, np.int64), np.zeros(0, np.int64)))
                continue
            with torch.no_grad():
                C = matcher_cost(logits[b], masks[b], targets[b]["labels"], targets[b]["masks"], coords, w_class, w_mask, w_dice, dtype)
            cur_c.append(C.cpu().numpy())                                                 # (one blocking copy per (output, clip))
            cur_a.append(assign(cur_c[-1]))
        costs.append(cur_c)
        assignments.append(cur_a)
        # class loss: matched queries get their tube's label, the others "no object"
        tc = torch.full((B, Q), num_classes, dtype=torch.int64, device=dev)
        cur_t = [(torch.from_numpy(i).to(dev), torch.from_numpy(j).to(dev)) for i, j in cur_a]
        for b, (i, j) in enumerate(cur_t):
            tc[b, i] = targets[b]["labels"][j]
        losses["loss_ce" + sfx] = F.cross_entropy(logits.transpose(1, 2), tc, weight)
        # mask losses on (pair, frame) rows, one point set per row
        x_rows = torch.cat([masks[b][i] for b, (i, _) in enumerate(cur_t)]).flatten(0, 1)[:, None]
        t_rows = torch.cat([targets[b]["masks"][j].to(dtype) for b, (_, j) in enumerate(cur_t)]).flatten(0, 1)[:, None]
        over, rand = q.pop(0).to(dtype), q.pop(0).to(dtype)
        with torch.no_grad():
            unc = -point_sample(x_rows, over)[:, 0].abs()
            idx = unc.topk(k_unc, dim=1)[1]
            coords = torch.cat([torch.gather(over, 1, idx[:, :, None].expand(-1, -1, 2)), rand], 1)
            t = point_sample(t_rows, coords)[:, 0]
        x = point_sample(x_rows, coords)[:, 0]
        losses["loss_mask" + sfx] = F.binary_cross_entropy_with_logits(x, t, reduction="none").mean(1).sum() / num_masks
        s = x.sigmoid()
        losses["loss_dice" + sfx] = (1 - (2 * (s * t).sum(1) + 1) / (s.sum(1) + t.sum(1) + 1)).sum() / num_masks
    assert not q, f"{len(q)} unconsumed draws"
    return losses, costs, assignments


def load_fixture():
    """tests/golden/vtrain_small.npz (tests/golden/make_golden_vtrain.py) -> (z, cfg, clips, targets, draws): the raw per-frame
    annotations of every clip, the reference's targets (masks as bool), and the reference's draws regenerated from (seed, spec)
    and checked against the stored checksums."""
    import json
    import os
    from conftest import GOLDEN, regenerate_draws
    z = dict(np.load(os.path.join(GOLDEN, "vtrain_small.npz")))
    cfg = json.loads(str(z["cfg"]))
    draws = regenerate_draws(cfg["draw_seed"], json.loads(str(z["rng_spec"])))
    np.testing.assert_allclose(np.array([float(t.double().sum()) for t in draws]), z["rng_checksum"], rtol=0, atol=0,
                               err_msg="this torch build does not regenerate the fixture's random draws")
    Fr, (h, w), (H, W) = cfg["F"], cfg["image_size"], cfg["padded"]
    clips, targets = [], []
    for b in range(cfg["B"]):
        G, T = cfg["raw"][b], cfg["tubes"][b]
        fm = np.unpackbits(z[f"clip{b}_frame_masks"])[:Fr * G * h * w].reshape(Fr, G, h, w).astype(bool)
        clips.append({"masks": torch.from_numpy(fm), "ids": torch.from_numpy(z[f"clip{b}_frame_ids"]),
                      "classes": torch.from_numpy(z[f"clip{b}_frame_classes"])})
        m = np.unpackbits(z[f"clip{b}_masks"])[:T * Fr * H * W].reshape(T, Fr, H, W).astype(bool)
        targets.append({"labels": torch.from_numpy(z[f"clip{b}_labels"]), "ids": torch.from_numpy(z[f"clip{b}_ids"]),
                        "masks": torch.from_numpy(m)})
    return z, cfg, clips, targets, draws


def fixture_outs(z, cfg, variant):
    """the fixture's head outputs as the list (main, aux 0, ...) of dicts; variant "f32" or "bf16" (bf16-rounded masks, as fp32)"""
    masks = torch.from_numpy(z["pred_masks" if variant == "f32" else "pred_masks_bf16"])
    logits = torch.from_numpy(z["pred_logits"])
    return [{"pred_logits": logits[l], "pred_masks": masks[l]} for l in range(cfg["L"])]
