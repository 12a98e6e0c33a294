#!/usr/bin/env python3
"""Generate tests/golden/vtrain_small.npz by running the reference's OWN video training losses on the CPU: the unmodified
``VideoMaskFormer.prepare_targets`` (mask2former_video/video_maskformer_model.py:227-253), ``VideoHungarianMatcher``
(modeling/matcher.py) and ``VideoSetCriterion`` (modeling/criterion.py) on fixed head outputs (run where the reference is
importable; no test or benchmark reads it).  Usage:

    python tests/golden/make_golden_vtrain.py

The two modeling files are loaded from their paths behind _ref_import.setup() with one more stand-in,
``mask2former.utils.misc.is_dist_avail_and_initialized = lambda: False``; the model file gets them as its relative imports.  The
cost matrices are recorded where the reference hands them to SciPy (the matcher module's ``linear_sum_assignment`` name is wrapped:
same call, the argument kept).  The random draws are captured by ``RandCapture`` and stored as (seed, spec) for
``conftest.regenerate_draws``, with a checksum per draw.

B = 3 clips with 3, 0 and 11 tubes (4, 1 and 11 instances before the ones with id -1 in every frame are dropped), Q = 7, K = 5,
F = 3 frames of 33 x 50 padded to 36 x 52 (1872 pixels: not a multiple of 32), ground truth at density 0.3 with one tube absent
from (all-zero in) one frame, mask logits 9 x 13 ~ 3 N(0, 1), L = 2 outputs, P = 500 points, oversample 3, importance 0.75,
weights class 2 / mask 5 / dice 5, eos_coef 0.1; inputs in fp32 and bf16-rounded with the reference's results for both.  The seed
is advanced until every assignment problem beats its second-best assignment by >= 1e-2 (_vtrain_restate.second_best_margin).
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import as R  # noqa: E402
import make_golden_infer as GI  # noqa: E402
from _vtrain_restate import second_best_margin  # noqa: E402

B, Q, K, FRAMES, L = 3, 7, 5, 3, 2
RAW = (4, 1, 11)                # instances per clip; the last one of clips 0 and 1 has id -1 in every frame
TUBES = (3, 0, 11)
LOWRES = (9, 13)
IMAGE_SIZE = (33, 50)
PADDED = (36, 52)
P, OVERSAMPLE, IMPORTANCE = 500, 3.0, 0.75
W_CLASS, W_MASK, W_DICE, EOS = 2.0, 5.0, 5.0, 0.1
MARGIN = 1e-2
DRAW_SEED_OFFSET = 100000


class FrameInstances:
    """what prepare_targets reads of a detectron2 ``Instances``: image_size, gt_ids, gt_classes, gt_masks.tensor, len(), .to()"""

    def __init__(self, image_size, gt_ids, gt_classes, masks):
        self.image_size, self.gt_ids, self.gt_classes = image_size, gt_ids, gt_classes
        self.gt_masks = types.SimpleNamespace(tensor=masks)

    def __len__(self):
        return len(self.gt_ids)

    def to(self, device):
        return self


def _load(pkg, rel):
    path = os.path.join(R.REF, "mask2former_video", *rel.split("/"))
    spec = importlib.util.spec_from_file_location(pkg + "." + rel[:-3].replace("/", "."), path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    GI.load_maskformer()        # _ref_import.setup() and the detectron2 stand-ins of the model file's imports
    if "mask2former.utils" not in sys.modules:
        R._mod("mask2former.utils")
    R._mod("mask2former.utils.misc", is_dist_avail_and_initialized=lambda: False)
    pkg = "_mpf_ref_vtrain"
    R._mod(pkg)
    R._mod(pkg + ".modeling")
    R._mod(pkg + ".utils")
    R._mod(pkg + ".utils.memory", retry_if_cuda_oom=lambda f: f)
    matcher = _load(pkg, "modeling/matcher.py")
    criterion = _load(pkg, "modeling/criterion.py")
    model = _load(pkg, "video_maskformer_model.py")
    return matcher, criterion, model.VideoMaskFormer, matcher.linear_sum_assignment


def make_inputs(seed):
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn(L, B, Q, K + 1, generator=gen) * 2.0
    masks = torch.randn(L, B, Q, FRAMES, *LOWRES, generator=gen) * 3.0
    clips = []
    for b in range(B):
        G = RAW[b]
        fm = torch.rand(FRAMES, G, *IMAGE_SIZE, generator=gen) < 0.3
        ids = torch.arange(G)[None].repeat(FRAMES, 1)
        if G != TUBES[b]:
            ids[:, -1] = -1                                     # never seen: dropped by prepare_targets
        if b == 0:
            ids[1, 1] = -1                                      # tube 1 is absent from frame 1: an all-zero plane there
            fm[1, 1] = False
        # the class vector of every frame but the last is a decoy: the reference reads the last frame's (:246)
        classes = torch.randint(0, K, (FRAMES, G), generator=gen)
        clips.append({"masks": fm, "ids": ids, "classes": classes})
    return logits, masks, clips


def run_reference(ref, logits, masks, clips, draw_seed):
    matcher_mod, criterion_mod, VideoMaskFormer, solve = ref
    recorded = []

    def recording(C):
        recorded.append(np.asarray(C, dtype=np.float32).copy())
        return solve(C)

    matcher_mod.linear_sum_assignment = recording
    matcher = matcher_mod.VideoHungarianMatcher(cost_class=W_CLASS, cost_mask=W_MASK, cost_dice=W_DICE, num_points=P)
    base = {"loss_ce": W_CLASS, "loss_mask": W_MASK, "loss_dice": W_DICE}
    weight_dict = dict(base)
    for i in range(L - 1):
        weight_dict.update({k + f"_{i}": v for k, v in base.items()})
    criterion = criterion_mod.VideoSetCriterion(K, matcher=matcher, weight_dict=weight_dict, eos_coef=EOS, losses=["labels", "masks"],
                                                num_points=P, oversample_ratio=OVERSAMPLE, importance_sample_ratio=IMPORTANCE)
    model = VideoMaskFormer(backbone=GI._Backbone(), sem_seg_head=torch.nn.Identity(), criterion=criterion, num_queries=Q,
                            object_mask_threshold=0.8, overlap_threshold=0.8, metadata=None, size_divisibility=4,
                            sem_seg_postprocess_before_inference=True, pixel_mean=[0.0, 0.0, 0.0], pixel_std=[1.0, 1.0, 1.0],
                            num_frames=FRAMES)
    batched = [{"instances": [FrameInstances(IMAGE_SIZE, c["ids"][f], c["classes"][f], c["masks"][f]) for f in range(FRAMES)]}
               for c in clips]
    images = types.SimpleNamespace(tensor=torch.zeros(B * FRAMES, 3, *PADDED))
    targets = model.prepare_targets(batched, images)
    lg = logits.clone().requires_grad_(True)
    mk = masks.clone().requires_grad_(True)
    outputs = {"pred_logits": lg[0], "pred_masks": mk[0],
               "aux_outputs": [{"pred_logits": lg[l], "pred_masks": mk[l]} for l in range(1, L)]}
    torch.manual_seed(draw_seed)
    with R.RandCapture() as cap:
        losses = criterion(outputs, targets)
    total = sum(losses[k] * weight_dict[k] for k in losses if k in weight_dict)
    total.backward()
    # the matcher ran once per (output, clip), clips with no tube included (SciPy gets a [Q, 0] matrix there)
    assert len(recorded) == L * B
    costs = np.full((L, B, Q, max(TUBES)), np.nan, dtype=np.float32)
    rows = np.full((L, B, Q), -1, dtype=np.int64)
    cols = np.full((L, B, Q), -1, dtype=np.int64)
    for n, C in enumerate(recorded):
        l, b = divmod(n, B)
        C = C.reshape(Q, -1)
        costs[l, b, :, :C.shape[1]] = C
        i, j = solve(C)
        rows[l, b, :len(i)], cols[l, b, :len(i)] = i, j
    names = sorted(losses)
    return {"targets": targets, "costs": costs, "rows": rows, "cols": cols, "loss_names": names,
            "loss_values": np.asarray([float(losses[k]) for k in names], dtype=np.float64), "total": float(total),
            "grad_masks": mk.grad.numpy().copy(), "grad_logits": lg.grad.numpy().copy(),
            "spec": cap.spec, "checksum": np.asarray([float(t.double().sum()) for _, t in cap.log])}


def usable(results):
    for r in results:
        for l in range(L):
            for b in range(B):
                if TUBES[b] and second_best_margin(r["costs"][l, b, :, :TUBES[b]]) < MARGIN:
                    return False
    return True


def main():
    torch.set_num_threads(1)
    ref = load_reference()
    seed = 3000
    while True:
        logits, masks, clips = make_inputs(seed)
        masks_bf16 = masks.to(torch.bfloat16).float()
        results = [run_reference(ref, logits, m, clips, seed + DRAW_SEED_OFFSET) for m in (masks, masks_bf16)]
        if usable(results):
            break
        seed += 1
    f32, bf16 = results
    assert f32["spec"] == bf16["spec"] and np.array_equal(f32["checksum"], bf16["checksum"])
    assert [len(t["labels"]) for t in f32["targets"]] == list(TUBES)
    cfg = {"B": B, "Q": Q, "K": K, "F": FRAMES, "L": L, "raw": RAW, "tubes": TUBES, "lowres": LOWRES, "image_size": IMAGE_SIZE,
           "padded": PADDED, "P": P, "oversample": OVERSAMPLE, "importance": IMPORTANCE, "w_class": W_CLASS, "w_mask": W_MASK,
           "w_dice": W_DICE, "eos_coef": EOS, "seed": seed, "draw_seed": seed + DRAW_SEED_OFFSET, "loss_names": f32["loss_names"]}
    z = {"cfg": json.dumps(cfg), "rng_spec": json.dumps(f32["spec"]), "rng_checksum": f32["checksum"],
         "pred_logits": logits.numpy(), "pred_masks": masks.numpy(), "pred_masks_bf16": masks_bf16.numpy()}
    for b, c in enumerate(clips):
        z[f"clip{b}_frame_masks"] = np.packbits(c["masks"].numpy())
        z[f"clip{b}_frame_ids"] = c["ids"].numpy()
        z[f"clip{b}_frame_classes"] = c["classes"].numpy()
        t = f32["targets"][b]
        assert t["masks"].dtype == torch.float32 and set(t["masks"].unique().tolist()) <= {0.0, 1.0}
        z[f"clip{b}_labels"] = t["labels"].numpy()
        z[f"clip{b}_ids"] = t["ids"].numpy()
        z[f"clip{b}_masks"] = np.packbits(t["masks"].bool().numpy())
    for prefix, r in (("f32", f32), ("bf16", bf16)):
        for k in ("costs", "rows", "cols", "loss_values", "grad_masks", "grad_logits"):
            z[f"{prefix}_{k}"] = r[k]
        z[f"{prefix}_total"] = np.float64(r["total"])
    path = os.path.join(HERE, "vtrain_small.npz")
    np.savez_compressed(path, **z)
    print(f"{path}: {os.path.getsize(path)} bytes, seed {seed}")


if __name__ == "__main__":
    main()
