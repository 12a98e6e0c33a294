#!/usr/bin/env python3
"""Generate tests/golden/infer_*.npz by running the reference's OWN eval branch (MaskFormer.forward in eval mode,
mask2former/maskformer_model.py:233-279 with semantic / panoptic / instance inference :301-401) on fixed head outputs
(run where the reference is importable; no test or benchmark reads it).  Usage:

    python tests/golden/make_golden_infer.py

A stub backbone and a stub sem_seg_head return fixed pred_logits / pred_masks, so the fixture pins everything the eval
branch does after the head: the upsample to the padded size, sem_seg_postprocess, and the three inference functions.
The detectron2 symbols maskformer_model.py imports (:8-18) are stubbed here with detectron2's semantics, on top of
_ref_import.setup() (which is used as is).  Each fixture holds N = 2 images (one output smaller than the padded size,
one larger, odd ratios), the inputs in fp32 and bf16-rounded, and the reference's results for both.
"""
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_import as R  # noqa: E402


# ---- detectron2 stand-ins (detectron2/structures, detectron2/modeling/postprocessing.py) -----------------------------------
class Boxes:
    def __init__(self, tensor):
        self.tensor = tensor


class Instances:
    def __init__(self, image_size, **kw):
        self.__dict__["_image_size"] = tuple(image_size)
        self.__dict__["_fields"] = dict(kw)

    @property
    def image_size(self):
        return self._image_size

    def __setattr__(self, k, v):
        self._fields[k] = v

    def __getattr__(self, k):
        if k in self.__dict__["_fields"]:
            return self.__dict__["_fields"][k]
        raise AttributeError(k)


class ImageList:
    """detectron2.structures.ImageList.from_tensors: pad to the largest image, rounded up to size_divisibility."""

    def __init__(self, tensor, image_sizes):
        self.tensor, self.image_sizes = tensor, image_sizes

    @staticmethod
    def from_tensors(tensors, size_divisibility=0, pad_value=0.0):
        sizes = [(int(t.shape[-2]), int(t.shape[-1])) for t in tensors]
        hmax, wmax = max(s[0] for s in sizes), max(s[1] for s in sizes)
        if size_divisibility > 1:
            d = size_divisibility
            hmax, wmax = (hmax + d - 1) // d * d, (wmax + d - 1) // d * d
        out = tensors[0].new_full((len(tensors), tensors[0].shape[0], hmax, wmax), pad_value)
        for i, t in enumerate(tensors):
            out[i, :, :t.shape[-2], :t.shape[-1]].copy_(t)
        return ImageList(out, sizes)


def sem_seg_postprocess(result, img_size, output_height, output_width):
    result = result[:, : img_size[0], : img_size[1]].expand(1, -1, -1, -1)
    return F.interpolate(result, size=(output_height, output_width), mode="bilinear", align_corners=False)[0]


def _box_xyxy_to_cxcywh(x):
    x0, y0, x1, y1 = x.unbind(-1)
    return torch.stack([(x0 + x1) / 2, (y0 + y1) / 2, (x1 - x0), (y1 - y0)], dim=-1)


def load_maskformer():
    R.setup()
    reg = R.Registry("META_ARCH")
    modeling = sys.modules["detectron2.modeling"]
    modeling.META_ARCH_REGISTRY = reg
    modeling.build_backbone = modeling.build_sem_seg_head = lambda *a, **k: None
    R._mod("detectron2.modeling.backbone", Backbone=nn.Module)
    R._mod("detectron2.modeling.postprocessing", sem_seg_postprocess=sem_seg_postprocess)
    R._mod("detectron2.data", MetadataCatalog=types.SimpleNamespace(get=lambda name: types.SimpleNamespace()))
    R._mod("detectron2.structures", Boxes=Boxes, ImageList=ImageList, Instances=Instances, BitMasks=object)
    R._mod("detectron2.utils.memory", retry_if_cuda_oom=lambda f: f)
    if "mask2former" not in sys.modules:
        R._mod("mask2former")
        R._mod("mask2former.util")
    R._mod("mask2former.util.box_ops", box_xyxy_to_cxcywh=_box_xyxy_to_cxcywh)
    sys.modules["mask2former.util"].box_ops = sys.modules["mask2former.util.box_ops"]
    return R.load("maskformer_model").MaskFormer


class _Backbone(nn.Module):
    size_divisibility = 0

    def forward(self, x):
        return {"res2": x}


class _Head(nn.Module):
    def __init__(self, num_classes, logits, masks):
        super().__init__()
        self.num_classes, self.logits, self.masks = num_classes, logits, masks

    def forward(self, features, mask=None, dn_args=None):
        return {"pred_logits": self.logits.clone(), "pred_masks": self.masks.clone()}


# ---- inputs ---------------------------------------------------------------------------------------------------------------
CASES = {
    # instance only (COCO instance config: before-inference post-processing forced on)
    "infer_instance": dict(K=7, Q=14, topk=12, semantic_on=False, instance_on=True, panoptic_on=False, before=True, things=None,
                           engineered=False),
    # all three on, things = the first 3 of 6 classes (COCO panoptic config)
    "infer_all": dict(K=6, Q=12, topk=10, semantic_on=True, instance_on=True, panoptic_on=True, before=True, things=[0, 1, 2],
                      engineered=True),
    # semantic only, inference at the cropped padded resolution (ADE20K / Cityscapes semantic configs)
    "infer_semantic": dict(K=5, Q=10, topk=100, semantic_on=True, instance_on=False, panoptic_on=False, before=False, things=None,
                           engineered=False),
}
LOWRES = (10, 14)
SIZE_DIV = 8
IMAGE_SIZES = [(37, 50), (33, 56)]          # padded batch: (40, 56)
OUTPUT_SIZES = [(29, 41), (61, 83)]         # one smaller than the padded size, one larger, odd ratios


def _blob(h, w, cy, cx, r, amp=5.0):
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    d = torch.sqrt((yy - cy) ** 2 + (xx - cx) ** 2)
    return (amp * torch.tanh((r - d) / 1.5)).float()


def make_inputs(c, gen):
    N, Q, K = 2, c["Q"], c["K"]
    h, w = LOWRES
    masks = torch.randn(N, Q, h, w, generator=gen) * 3.0
    logits = torch.randn(N, Q, K + 1, generator=gen) * 2.0
    if c["engineered"]:
        # image 0: stuff merge (q0, q1 both class 3), an overlap rejection (q3's wider disk wins q2's rim, so q2 keeps too
        # little of its own area), a no-object query (q4);
        # the remaining queries stay below the object-mask threshold.  Image 1: nothing kept.
        logits[:] = torch.randn(N, Q, K + 1, generator=gen) * 0.3
        strong = {0: (3, 7.0), 1: (3, 7.0), 2: (0, 8.0), 3: (1, 6.0), 5: (4, 7.0)}
        for q, (cls, v) in strong.items():
            logits[0, q, cls] = v
        logits[0, 4, K] = 8.0                                           # no-object
        masks[0, 0] = _blob(h, w, 2.0, 3.0, 3.0)
        masks[0, 1] = _blob(h, w, 7.5, 11.0, 2.5)
        masks[0, 2] = _blob(h, w, 5.0, 7.0, 3.0)
        masks[0, 3] = _blob(h, w, 5.2, 7.3, 3.4)                        # covers q2's disk and more
        masks[0, 4] = _blob(h, w, 8.0, 2.0, 3.0)
        masks[0, 5] = _blob(h, w, 1.0, 12.0, 2.0)
        logits[1] = torch.randn(Q, K + 1, generator=gen) * 0.3          # max prob < 0.8 everywhere
        logits[1, :3, K] = 6.0                                          # and a few no-object queries
    return logits, masks


def run_reference(MaskFormer, c, logits, masks):
    head = _Head(c["K"], logits, masks)
    meta = types.SimpleNamespace(thing_dataset_id_to_contiguous_id={100 + i: i for i in (c["things"] or [])})
    model = MaskFormer(backbone=_Backbone(), sem_seg_head=head, criterion=None, num_queries=c["Q"], object_mask_threshold=0.8,
                       overlap_threshold=0.8, metadata=meta, size_divisibility=SIZE_DIV, sem_seg_postprocess_before_inference=c["before"],
                       pixel_mean=[0.0, 0.0, 0.0], pixel_std=[1.0, 1.0, 1.0], semantic_on=c["semantic_on"],
                       panoptic_on=c["panoptic_on"], instance_on=c["instance_on"], test_topk_per_image=c["topk"], scalar=1,
                       noise_scale=0.0).eval()
    batched = [{"image": torch.zeros(3, *s), "height": o[0], "width": o[1]} for s, o in zip(IMAGE_SIZES, OUTPUT_SIZES)]
    with torch.no_grad():
        return model(batched)


def pack(results, prefix):
    z = {}
    for n, r in enumerate(results):
        p = f"{prefix}_{n}_"
        if "sem_seg" in r:
            z[p + "sem_seg"] = r["sem_seg"].float().numpy()
        if "panoptic_seg" in r:
            ids, info = r["panoptic_seg"]
            z[p + "pan_ids"] = ids.numpy().astype(np.int32)
            z[p + "pan_segments"] = np.array([[s["id"], int(s["isthing"]), s["category_id"]] for s in info], dtype=np.int64).reshape(-1, 3)
        if "instances" in r:
            ins = r["instances"]
            z[p + "inst_masks"] = ins.pred_masks.numpy().astype(np.uint8)
            z[p + "inst_scores"] = ins.scores.float().numpy()
            z[p + "inst_classes"] = ins.pred_classes.numpy().astype(np.int64)
    return z


def main():
    torch.set_num_threads(1)
    MaskFormer = load_maskformer()
    for i, (name, c) in enumerate(CASES.items()):
        gen = torch.Generator().manual_seed(1000 + i)
        logits, masks = make_inputs(c, gen)
        masks_bf16 = masks.to(torch.bfloat16).float()
        z = {"pred_logits": logits.numpy(), "pred_masks": masks.numpy(), "pred_masks_bf16": masks_bf16.numpy(),
             "image_sizes": np.array(IMAGE_SIZES, dtype=np.int64), "output_sizes": np.array(OUTPUT_SIZES, dtype=np.int64),
             "config": np.array(json.dumps({"num_classes": c["K"], "num_queries": c["Q"], "object_mask_threshold": 0.8,
                                            "overlap_threshold": 0.8, "test_topk_per_image": c["topk"],
                                            "semantic_on": c["semantic_on"], "instance_on": c["instance_on"],
                                            "panoptic_on": c["panoptic_on"], "sem_seg_postprocess_before_inference": c["before"],
                                            "thing_ids": c["things"] or [], "size_divisibility": SIZE_DIV}))}
        z.update(pack(run_reference(MaskFormer, c, logits, masks), "f32"))
        z.update(pack(run_reference(MaskFormer, c, logits, masks_bf16), "bf16"))
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **z)
        print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
