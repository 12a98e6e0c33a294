#!/usr/bin/env python3
"""Generate tests/golden/vinfer_small.npz by running the reference's OWN video eval branch (VideoMaskFormer.forward in eval mode
and inference_video, mask2former_video/video_maskformer_model.py:180-188, :204-287) on fixed head outputs, on the CPU (run where
the reference is importable; no test or benchmark reads it).  Usage:

    python tests/golden/make_golden_vinfer.py

A stub backbone and a stub sem_seg_head return fixed pred_logits / pred_masks, so the fixture pins everything the branch does
after the head: the upsample of all queries to the padded size, the top-10 selection, the crop, the resize and the threshold.  The
detectron2 symbols the file imports (:10-15) are the stand-ins of make_golden_infer.py on top of _ref_import.setup(); its own
relative imports (criterion, matcher, retry_if_cuda_oom) are stubbed: the eval branch uses none of the first two, and the third
is the identity here.

One clip: Q = 12, K = 5, F = 3 frames of 33 x 50 (padded to 36 x 52), mask logits 9 x 13 ~ 4 N(0, 1), output 47 x 71 (3337
positions, not a multiple of 64); inputs in fp32 and bf16-rounded with the reference's results for both.  The seed is advanced
until the top-10 scores are more than 1e-6 apart and the fp32 resampled logits are within the tests' tie band of the fp64 ones.
"""
import importlib.util
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import as R  # noqa: E402
import make_golden_infer as GI  # noqa: E402
from _video_restate import inference_video  # noqa: E402

Q, K, FRAMES = 12, 5, 3
LOWRES = (9, 13)
SIZE_DIV = 4
IMAGE_SIZE = (33, 50)           # padded: (36, 52)
OUTPUT_SIZE = (47, 71)
BAND = 2e-5                     # tests/test_infer_gpu.py


def load_video_maskformer():
    GI.load_maskformer()        # _ref_import.setup() and the detectron2 stand-ins of the image model's imports
    pkg = "_mpf_ref_video"
    R._mod(pkg)
    R._mod(pkg + ".modeling")
    R._mod(pkg + ".modeling.criterion", VideoSetCriterion=object)
    R._mod(pkg + ".modeling.matcher", VideoHungarianMatcher=object)
    R._mod(pkg + ".utils")
    R._mod(pkg + ".utils.memory", retry_if_cuda_oom=lambda f: f)
    path = os.path.join(R.REF, "mask2former_video", "video_maskformer_model.py")
    spec = importlib.util.spec_from_file_location(pkg + ".video_maskformer_model", path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.VideoMaskFormer


class _Head(nn.Module):
    def __init__(self, logits, masks):
        super().__init__()
        self.num_classes, self.logits, self.masks = K, logits, masks

    def forward(self, features):
        return {"pred_logits": self.logits[None].clone(), "pred_masks": self.masks[None].clone()}


def run_reference(VideoMaskFormer, logits, masks):
    model = VideoMaskFormer(backbone=GI._Backbone(), sem_seg_head=_Head(logits, masks), criterion=None, num_queries=Q,
                            object_mask_threshold=0.8, overlap_threshold=0.8, metadata=None, size_divisibility=SIZE_DIV,
                            sem_seg_postprocess_before_inference=True, pixel_mean=[0.0, 0.0, 0.0], pixel_std=[1.0, 1.0, 1.0],
                            num_frames=FRAMES).eval()
    batched = [{"image": [torch.zeros(3, *IMAGE_SIZE) for _ in range(FRAMES)], "height": OUTPUT_SIZE[0], "width": OUTPUT_SIZE[1]}]
    with torch.no_grad():
        return model(batched)


def make_inputs(seed):
    gen = torch.Generator().manual_seed(seed)
    masks = torch.randn(Q, FRAMES, *LOWRES, generator=gen) * 4.0
    logits = torch.randn(Q, K + 1, generator=gen) * 2.0
    return logits, masks


def usable(logits, masks):
    padded = tuple((s + SIZE_DIV - 1) // SIZE_DIV * SIZE_DIV for s in IMAGE_SIZE)
    for m in (masks, masks.to(torch.bfloat16).float()):
        r32 = inference_video(logits, m, IMAGE_SIZE, padded, *OUTPUT_SIZE)
        r64 = inference_video(logits, m, IMAGE_SIZE, padded, *OUTPUT_SIZE, dtype=torch.float64)
        if float((r32["logits"].double() - r64["logits"]).abs().max()) > BAND:
            return False
        if float((r32["scores"][:-1] - r32["scores"][1:]).min()) <= 1e-6:
            return False
    return True


def pack(out, prefix):
    assert tuple(out["image_size"]) == OUTPUT_SIZE
    return {prefix + "_scores": np.asarray(out["pred_scores"], dtype=np.float32),
            prefix + "_labels": np.asarray(out["pred_labels"], dtype=np.int64),
            prefix + "_masks": np.packbits(torch.stack(out["pred_masks"]).numpy()),
            prefix + "_masks_shape": np.asarray(torch.stack(out["pred_masks"]).shape, dtype=np.int64)}


def main():
    torch.set_num_threads(1)
    VideoMaskFormer = load_video_maskformer()
    seed = 2000
    while not usable(*make_inputs(seed)):
        seed += 1
    logits, masks = make_inputs(seed)
    masks_bf16 = masks.to(torch.bfloat16).float()
    z = {"pred_logits": logits.numpy(), "pred_masks": masks.numpy(), "pred_masks_bf16": masks_bf16.numpy(), "seed": np.int64(seed),
         "image_size": np.asarray(IMAGE_SIZE, dtype=np.int64), "output_size": np.asarray(OUTPUT_SIZE, dtype=np.int64),
         "size_divisibility": np.int64(SIZE_DIV), "num_classes": np.int64(K), "num_queries": np.int64(Q)}
    z.update(pack(run_reference(VideoMaskFormer, logits, masks), "f32"))
    z.update(pack(run_reference(VideoMaskFormer, logits, masks_bf16), "bf16"))
    path = os.path.join(HERE, "vinfer_small.npz")
    np.savez_compressed(path, **z)
    print(f"{path}: {os.path.getsize(path)} bytes, seed {seed}")


if __name__ == "__main__":
    main()
