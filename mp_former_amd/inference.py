"""Inference post-processing: the eval branch of MaskFormer.forward (mask2former/maskformer_model.py:236-279) with its
semantic / panoptic / instance inference (:301-401), on the native kernels of csrc/seg_infer.hip.

``postprocess`` takes the head's outputs (``pred_logits`` [N, Q, K+1], ``pred_masks`` [N, Q, h, w], fp32 or bf16) and
returns the reference's list of per-image dicts.  Each kernel reads the low-resolution logits once and writes only the
final result: the [Q, Hp, Wp] upsampled and [Q, H, W] cropped-and-resized tensors of the reference are never formed.
The per-pixel work runs on the device; what stays on the host is the panoptic segment table (sequential, a few dozen
entries), fed by ONE device-to-host copy of the per-query area counters.  CPU tensors and other dtypes raise: there is
no torch fallback.

Deviations from the reference, by design:
* ``instances`` are sorted by score, descending (the reference's ``topk(sorted=False)`` order is unspecified);
* all results are fp32 whatever the mask dtype (bf16 logits are widened on load; the reference would compute in bf16).
"""
from dataclasses import dataclass, field

import torch
import torch.nn.functional as F

from . import _lib

_MASK_DTYPES = (torch.float32, torch.bfloat16)


@dataclass
class InferenceConfig:
    """The inference attributes of the reference's ``MaskFormer`` (maskformer_model.py:73-98, from_config :151-170)."""
    num_classes: int
    num_queries: int = 100
    object_mask_threshold: float = 0.8
    overlap_threshold: float = 0.8
    test_topk_per_image: int = 100
    semantic_on: bool = False
    instance_on: bool = True
    panoptic_on: bool = False
    sem_seg_postprocess_before_inference: bool = True
    thing_ids: frozenset = field(default_factory=frozenset)     # contiguous ids of the thing classes

    def __post_init__(self):
        self.thing_ids = frozenset(int(i) for i in self.thing_ids)
        if not self.semantic_on and not self.sem_seg_postprocess_before_inference:
            raise ValueError("sem_seg_postprocess_before_inference=False needs semantic_on (maskformer_model.py:97-98)")
        if (self.instance_on or self.panoptic_on) and not self.sem_seg_postprocess_before_inference:
            raise ValueError("instance / panoptic inference runs on masks at the output size (from_config :155-159)")

    @classmethod
    def from_maskformer(cls, model):
        """Read the attributes of a reference ``MaskFormer`` instance."""
        meta = getattr(model, "metadata", None)
        things = getattr(meta, "thing_dataset_id_to_contiguous_id", None) or {}
        return cls(num_classes=int(model.sem_seg_head.num_classes), num_queries=int(model.num_queries),
                   object_mask_threshold=float(model.object_mask_threshold), overlap_threshold=float(model.overlap_threshold),
                   test_topk_per_image=int(model.test_topk_per_image), semantic_on=bool(model.semantic_on),
                   instance_on=bool(model.instance_on), panoptic_on=bool(model.panoptic_on),
                   sem_seg_postprocess_before_inference=bool(model.sem_seg_postprocess_before_inference),
                   thing_ids=frozenset(things.values()))


# ---- results containers -----------------------------------------------------------------------------------------------------
class _Boxes:
    """Stand-in for detectron2.structures.Boxes (only ``tensor``) when detectron2 is not importable."""

    def __init__(self, tensor):
        self.tensor = tensor

    def __len__(self):
        return self.tensor.shape[0]


class _Instances:
    """Stand-in for detectron2.structures.Instances: ``image_size`` and the attributes set on it."""

    def __init__(self, image_size, **fields):
        self._image_size = tuple(image_size)
        self._fields = {}
        for k, v in fields.items():
            setattr(self, k, v)

    @property
    def image_size(self):
        return self._image_size

    def __setattr__(self, name, value):
        if name.startswith("_"):
            super().__setattr__(name, value)
        else:
            self._fields[name] = value

    def __getattr__(self, name):
        f = self.__dict__.get("_fields", {})
        if name in f:
            return f[name]
        raise AttributeError(name)

    def has(self, name):
        return name in self._fields

    def get_fields(self):
        return dict(self._fields)

    def __len__(self):
        for v in self._fields.values():
            return len(v)
        return 0


def _structures():
    try:
        from detectron2.structures import Boxes, Instances
        return Boxes, Instances
    except ImportError:
        return _Boxes, _Instances


# ---- host side of panoptic inference ---------------------------------------------------------------------------------------
def segment_table(labels, mask_area, original_area, intersection, thing_ids, overlap_threshold):
    """The sequential segment decision of panoptic_inference (maskformer_model.py:330-360) from the per-kept-entry areas.
    -> (lut, segments_info): lut[n] = the id painted where entry n wins with sigmoid >= 0.5 (0 = dropped)."""
    lut = [0] * len(labels)
    segments_info = []
    stuff_memory = {}
    current = 0
    for k, cls in enumerate(labels):
        cls = int(cls)
        isthing = cls in thing_ids
        ma, oa, inter = int(mask_area[k]), int(original_area[k]), int(intersection[k])
        if ma > 0 and oa > 0 and inter > 0:
            if ma / oa < overlap_threshold:
                continue
            if not isthing:
                if cls in stuff_memory:
                    lut[k] = stuff_memory[cls]
                    continue
                stuff_memory[cls] = current + 1
            current += 1
            lut[k] = current
            segments_info.append({"id": current, "isthing": bool(isthing), "category_id": cls})
    return lut, segments_info


# ---- native calls -----------------------------------------------------------------------------------------------------------
def _geom(masks_n, image_size, padded_hw, out_hw):
    Q, h, w = masks_n.shape
    return [Q, h, w, int(padded_hw[0]), int(padded_hw[1]), int(image_size[0]), int(image_size[1]), int(out_hw[0]), int(out_hw[1])]


def _masks_arg(pm):
    """(pointer of image 0, stride_q, dtype code) of [N, Q, h, w] logits whose [h, w] planes are contiguous."""
    if pm.dtype not in _MASK_DTYPES:
        raise TypeError(f"pred_masks must be float32 or bfloat16, got {pm.dtype}")
    if not (pm.stride(-1) == 1 and pm.stride(-2) == pm.shape[-1]):
        pm = pm.contiguous()
    return pm, pm.stride(0), pm.stride(1), _lib.DTYPE[pm.dtype]


class _Image:
    """Per-image launch state: the softmax prologue's outputs in one scratch buffer."""

    def __init__(self, cls, K, thr, dev, stream, slot):
        Q = cls.shape[0]
        self.Q, self.K = Q, K
        nbytes = 4 * (Q * K + 2 * Q + Q) + 4 * (1 + 2 * Q + 3 * Q)
        ws = _lib.scratch(("seg_infer.softmax", slot), dev, stream, nbytes)
        f = ws[:4 * (Q * K + 3 * Q)].view(torch.float32)
        self.probs = f[:Q * K].view(Q, K)
        self.max_score, self.max_label, self.kept_score = f[Q * K:Q * K + Q], f[Q * K + Q:Q * K + 2 * Q].view(torch.int32), f[Q * K + 2 * Q:]
        # {count, kept query [Q], kept label [Q], areas [3][Q]}: one device-to-host copy for the panoptic table
        self.ints = ws[4 * (Q * K + 3 * Q):4 * (Q * K + 3 * Q) + 4 * (1 + 5 * Q)].view(torch.int32)
        self.kept, self.areas = self.ints[:1 + 2 * Q], self.ints[1 + 2 * Q:]
        _lib.call("mpf_seg_softmax", dev, cls.data_ptr(), Q, K + 1, float(thr), self.probs.data_ptr(), self.max_score.data_ptr(),
                  self.max_label.data_ptr(), self.kept.data_ptr(), self.kept_score.data_ptr(), stream)


def _semantic(mptr, sq, dt, geom, probs, K, dev, stream):
    H, W = geom[-2:]
    out = torch.empty((K, H, W), dtype=torch.float32, device=dev)
    _lib.call("mpf_seg_semantic", dev, mptr, sq, dt, *geom, probs.data_ptr(), K, out.data_ptr(), stream)
    return out


def _instances(mptr, sq, dt, geom, img, cfg, thing_lut, dev, stream, image_hw):
    Q, K = img.Q, img.K
    H, W = geom[-2:]
    k = min(int(cfg.test_topk_per_image), Q * K)
    sc, idx = img.probs.reshape(-1).topk(k, sorted=True)
    labels = idx % K
    query = idx // K
    if cfg.panoptic_on:                                 # keep only thing classes (:381-389); the boolean index syncs
        keep = thing_lut[labels]
        sc, labels, query = sc[keep], labels[keep], query[keep]
    T = int(sc.shape[0])
    Boxes, Instances = _structures()
    result = Instances(image_hw)
    if T == 0:
        result.pred_masks = torch.zeros((0, H, W), dtype=torch.float32, device=dev)
        result.pred_boxes = Boxes(torch.zeros(0, 4))
        result.scores = sc
        result.pred_classes = labels
        return result
    query = query.contiguous()
    scores = torch.empty(T, dtype=torch.float32, device=dev)
    nws = _lib.lib().mpf_seg_instance_workspace_bytes(T, H, W)
    ws = _lib.scratch("seg_infer.instance", dev, stream, nws)
    _lib.call("mpf_seg_instance_scores", dev, mptr, sq, dt, *geom, query.data_ptr(), sc.data_ptr(), T, scores.data_ptr(), ws.data_ptr(),
              ws.numel(), stream)
    scores, order = scores.sort(descending=True, stable=True)
    query, labels = query[order].contiguous(), labels[order]
    masks = torch.empty((T, H, W), dtype=torch.float32, device=dev)
    _lib.call("mpf_seg_instance_masks", dev, mptr, sq, dt, *geom, query.data_ptr(), T, masks.data_ptr(), stream)
    result.pred_masks = masks
    result.pred_boxes = Boxes(torch.zeros(T, 4))
    result.scores = scores
    result.pred_classes = labels
    return result


def _panoptic(mptr, sq, dt, geom, img, cfg, dev, stream):
    Q = img.Q
    H, W = geom[-2:]
    code = torch.empty((H, W), dtype=torch.int32, device=dev)
    _lib.call("mpf_seg_panoptic_areas", dev, mptr, sq, dt, *geom, img.kept.data_ptr(), img.kept_score.data_ptr(), code.data_ptr(),
              img.areas.data_ptr(), stream)
    host = img.ints.cpu()                                # the one device-to-host copy of panoptic inference
    n = int(host[0])
    labels = host[1 + Q:1 + Q + n].tolist()
    ar = host[1 + 2 * Q:].view(3, Q)
    lut, segments_info = segment_table(labels, ar[0, :n].tolist(), ar[1, :n].tolist(), ar[2, :n].tolist(), cfg.thing_ids,
                                       cfg.overlap_threshold)
    ids = torch.empty((H, W), dtype=torch.int32, device=dev)
    lut_d = torch.tensor(lut + [0], dtype=torch.int32).to(dev)
    _lib.call("mpf_seg_panoptic_paint", dev, code.data_ptr(), H, W, lut_d.data_ptr(), ids.data_ptr(), stream)
    return ids, segments_info


def postprocess(pred_logits, pred_masks, image_sizes, padded_hw, output_sizes, cfg):
    """The reference's eval branch after the head (maskformer_model.py:236-279).

    pred_logits [N, Q, K+1] (any float dtype; widened to fp32), pred_masks [N, Q, h, w] fp32 / bf16 with contiguous [h, w]
    planes (a slice of the decoder's [N, L*Q, h, w] tensor is used in place), image_sizes [(hi, wi)] per image,
    padded_hw = the padded batch size (images.tensor.shape[-2:]), output_sizes [(height, width)] per image.
    -> list of dicts with "sem_seg" [K, height, width], "panoptic_seg" (ids int32 [height, width], segments_info) and
    "instances" (pred_masks [T, height, width] 0/1 fp32, pred_boxes zeros, scores, pred_classes), per the *_on flags."""
    if not (pred_masks.is_cuda and pred_logits.is_cuda):
        raise RuntimeError("postprocess: Not implemented on the CPU (device tensors only)")
    N, Q, K1 = pred_logits.shape
    K = K1 - 1
    if K != cfg.num_classes:
        raise ValueError(f"pred_logits has {K} classes + no-object, config {cfg.num_classes}")
    if pred_masks.dim() != 4 or pred_masks.shape[:2] != (N, Q):
        raise ValueError(f"pred_masks {tuple(pred_masks.shape)} does not match pred_logits {tuple(pred_logits.shape)}")
    pm, sn, sq, dt = _masks_arg(pred_masks)
    dev = pm.device
    out = []
    thing_lut = None
    if cfg.instance_on and cfg.panoptic_on:
        thing_lut = torch.zeros(K, dtype=torch.bool)
        for i in cfg.thing_ids:
            if 0 <= i < K:
                thing_lut[i] = True
        thing_lut = thing_lut.to(dev)
    stream = _lib.stream_ptr(dev)
    logits = pred_logits.detach().float()
    for n in range(N):
        mptr = pm.data_ptr() + n * sn * pm.element_size()
        hi, wi = int(image_sizes[n][0]), int(image_sizes[n][1])
        H, W = int(output_sizes[n][0]), int(output_sizes[n][1])
        img = _Image(logits[n].contiguous(), K, cfg.object_mask_threshold, dev, stream, n)
        res = {}
        if cfg.semantic_on:
            if cfg.sem_seg_postprocess_before_inference:
                res["sem_seg"] = _semantic(mptr, sq, dt, _geom(pm[n], (hi, wi), padded_hw, (H, W)), img.probs, K, dev, stream)
            else:   # inference on the cropped padded grid, then the reference's own resize of the K planes (:264-265)
                r = _semantic(mptr, sq, dt, _geom(pm[n], (hi, wi), padded_hw, (hi, wi)), img.probs, K, dev, stream)
                res["sem_seg"] = F.interpolate(r[None], size=(H, W), mode="bilinear", align_corners=False)[0]
        if cfg.panoptic_on:
            res["panoptic_seg"] = _panoptic(mptr, sq, dt, _geom(pm[n], (hi, wi), padded_hw, (H, W)), img, cfg, dev, stream)
        if cfg.instance_on:
            res["instances"] = _instances(mptr, sq, dt, _geom(pm[n], (hi, wi), padded_hw, (H, W)), img, cfg, thing_lut, dev, stream,
                                          (H, W))
        out.append(res)
    return out
