"""Inference post-processing: the eval branch of MaskFormer.forward (mask2former/maskformer_model.py:236-279) with its
semantic / panoptic / instance inference (:301-401), on the native kernels of csrc/seg_infer.hip.

``postprocess`` takes the head's outputs (``pred_logits`` [N, Q, K+1], ``pred_masks`` [N, Q, h, w], fp32 or bf16) and
returns the reference's list of per-image dicts.  Each kernel reads the low-resolution logits once and writes only the
final result: the [Q, Hp, Wp] upsampled and [Q, H, W] cropped-and-resized tensors of the reference are never formed.
The per-pixel work runs on the device; what stays on the host is the panoptic segment table (sequential, a few dozen
entries), fed by ONE device-to-host copy of the per-query area counters.  CPU tensors and other dtypes raise: there is
no torch fallback.

``InferenceConfig.instance_boxes`` (off by default: the reference's zeros) fills ``pred_boxes`` with the bounding boxes of the
instance masks, which the reference leaves commented out as slow (maskformer_model.py:393-395): ``mask_boxes`` reads them off
the packed bits (csrc/seg_box.hip), and ``InstanceAP(iou_type="bbox")`` scores COCO's box AP on them.

For an evaluation loop the largest results can be had in the form their consumers use (both off by default):
* ``InferenceConfig.semantic_labels``: ``"sem_seg_labels"`` int32 [H, W] (the argmax every evaluator takes) instead of the
  fp32 [K, H, W] ``"sem_seg"``, which is then never written; ``SemSegConfusion`` accumulates the (K+1) x (K+1) counts of mIoU
  from such label maps on the device.
* ``InferenceConfig.instance_masks = "rle"``: ``pred_masks_rle`` (uncompressed COCO run lengths) instead of the fp32
  [T, H, W] ``pred_masks``; only the run lengths cross to the host (``rle_compress`` makes them the strings a COCO json holds).

The ground-truth side of such a loop reads a COCO / YouTube-VIS json without pycocotools and without a dense mask on the host:
``polygon_bits``, ``rle_bits`` and ``segmentation_bits`` turn polygons, uncompressed and compressed RLE into the packed bits the
scoring classes take (csrc/seg_codec.hip); ``unpack_masks`` / ``polygon_masks`` give dense targets on the device.

``SemanticTTA`` is the reference's semantic test-time augmentation (mask2former/test_time_augmentation.py): the mean of the
views' "sem_seg", flipped views mirrored back, accumulated view by view in one [K, H, W] buffer on the device.

``postprocess_video`` is the eval branch of the reference's ``VideoMaskFormer`` (mask2former_video/video_maskformer_model.py:
204-287) for one clip, on csrc/seg_video.hip: the top entries are selected first and only their frames are resampled, as dense
bool masks, packed bits or run lengths; ``InstanceAP(tubes=True)`` / ``TubeAP`` scores such tubes as the reference's
YouTube-VIS evaluation does.

Deviations from the reference, by design:
* ``instances`` are sorted by score, descending (the reference's ``topk(sorted=False)`` order is unspecified);
* all results are fp32 whatever the mask dtype (bf16 logits are widened on load; the reference would compute in bf16).
"""
from dataclasses import dataclass, field

import numpy as np
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
    semantic_labels: bool = False       # "sem_seg_labels" int32 [H, W] instead of "sem_seg" fp32 [K, H, W]
    instance_masks: str = "dense"       # "dense": pred_masks fp32 [T, H, W]; "rle": pred_masks_rle (uncompressed COCO RLE)
    instance_boxes: bool = False        # pred_boxes = the masks' bounding boxes (maskformer_model.py:393-395) instead of zeros

    def __post_init__(self):
        self.thing_ids = frozenset(int(i) for i in self.thing_ids)
        if self.semantic_labels and not self.semantic_on:
            raise ValueError("semantic_labels needs semantic_on")
        if self.instance_masks not in ("dense", "rle"):
            raise ValueError(f"instance_masks must be 'dense' or 'rle', got {self.instance_masks!r}")
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

    def to(self, *args, **kwargs):
        return type(self)(self.tensor.to(*args, **kwargs))


class _BitMasks(_Boxes):
    """Stand-in for detectron2.structures.BitMasks (``tensor`` bool [N, H, W], ``to``, ``len``)."""


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

    def to(self, *args, **kwargs):
        return type(self)(self._image_size, **{k: v.to(*args, **kwargs) if hasattr(v, "to") else v for k, v in self._fields.items()})

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
def _planes(pm):
    """[N, Q, h, w] mask logits as the kernels read them: fp32 / bf16 with contiguous [h, w] planes (copied only if they are not)."""
    if pm.dtype not in _MASK_DTYPES:
        raise TypeError(f"pred_masks must be float32 or bfloat16, got {pm.dtype}")
    if not (pm.stride(-1) == 1 and pm.stride(-2) == pm.shape[-1]):
        pm = pm.contiguous()
    return pm


class _View:
    """One image's mask logits and sizes, as the per-pixel entry points take them: image ``n`` of ``pm`` ([N, Q, h, w] from
    ``_planes``), its image size (hi, wi) on the padded grid and its output size (H, W).  Carries the device and stream of its
    launches."""

    def __init__(self, pm, n, image_size, padded_hw, out_hw, stream):
        self.dev, self.stream = pm.device, stream
        self.ptr = pm.data_ptr() + n * pm.stride(0) * pm.element_size()
        self.stride_q, self.dtype = pm.stride(1), _lib.DTYPE[pm.dtype]
        self.low = tuple(pm.shape[1:])                                       # Q, h, w
        self.padded = (int(padded_hw[0]), int(padded_hw[1]))
        self.image = (int(image_size[0]), int(image_size[1]))
        self.out = (int(out_hw[0]), int(out_hw[1]))

    def args(self, out_hw=None):
        """The twelve leading arguments (masks, stride_q, dtype, Q, h, w, Hp, Wp, hi, wi, H, W) for the view's output size, or for
        ``out_hw``: the "after" mode computes on the cropped padded grid, (hi, wi)."""
        return (self.ptr, self.stride_q, self.dtype, *self.low, *self.padded, *self.image, *(out_hw or self.out))


class _Image:
    """Per-image launch state: the softmax prologue's outputs in one scratch buffer.  Its layout: a float part {probs [Q, K],
    max_score [Q], max_label [Q] (int32 bits), kept_score [Q]}, then an int part {count, kept query [Q], kept label [Q],
    areas [3][Q]}, which is what panoptic inference copies to the host, in one piece."""

    def __init__(self, cls, K, thr, dev, stream, slot):
        Q = cls.shape[0]
        self.Q, self.K = Q, K
        nf, ni = Q * K + 3 * Q, 1 + 5 * Q
        ws = _lib.scratch(("seg_infer.softmax", slot), dev, stream, 4 * (nf + ni))
        f, self.ints = ws[:4 * nf].view(torch.float32), ws[4 * nf:4 * (nf + ni)].view(torch.int32)
        probs, self.max_score, max_label, self.kept_score = f.split([Q * K, Q, Q, Q])
        self.probs, self.max_label = probs.view(Q, K), max_label.view(torch.int32)
        self.kept, self.areas = self.ints.split([1 + 2 * Q, 3 * Q])
        _lib.call("mpf_seg_softmax", dev, cls.data_ptr(), Q, K + 1, float(thr), self.probs.data_ptr(), self.max_score.data_ptr(),
                  self.max_label.data_ptr(), self.kept.data_ptr(), self.kept_score.data_ptr(), stream)


def _semantic(view, img, out_hw=None):
    """The scores [K, H, W] at the view's output size, or at ``out_hw``."""
    out = torch.empty((img.K, *(out_hw or view.out)), dtype=torch.float32, device=view.dev)
    _lib.call("mpf_seg_semantic", view.dev, *view.args(out_hw), img.probs.data_ptr(), img.K, out.data_ptr(), view.stream)
    return out


def _semantic_labels(view, img):
    """"before" mode: the label map straight from the logits, in one launch."""
    out = torch.empty(view.out, dtype=torch.int32, device=view.dev)
    _lib.call("mpf_seg_semantic_labels", view.dev, *view.args(), img.probs.data_ptr(), img.K, out.data_ptr(), view.stream)
    return out


def _labels_resize(view, scores):
    """"after" mode: scores [K, hi, wi] on the cropped grid -> labels [H, W] of their bilinear resize."""
    out = torch.empty(view.out, dtype=torch.int32, device=view.dev)
    _lib.call("mpf_seg_labels_resize", view.dev, scores.data_ptr(), *scores.shape, *view.out, out.data_ptr(), view.stream)
    return out


def _instance_rle(view, query, T):
    """The masks of the sorted entries as uncompressed COCO RLE dicts; two device-to-host copies: offsets, then counts."""
    (H, W), dev, stream = view.out, view.dev, view.stream
    nws = _lib.lib().mpf_seg_instance_rle_workspace_bytes(T, H, W)
    ws = _lib.scratch("seg_infer.rle", dev, stream, nws)
    offsets = torch.empty(T + 1, dtype=torch.int64, device=dev)
    _lib.call("mpf_seg_instance_rle_count", dev, *view.args(), query.data_ptr(), T, offsets.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    off = offsets.cpu().numpy()                          # copy 1: where every entry's counts lie
    total = int(off[T])
    pos = _lib.scratch("seg_infer.rle_pos", dev, stream, 4 * total)
    counts = torch.empty(total, dtype=torch.int32, device=dev)
    _lib.call("mpf_seg_instance_rle_write", dev, ws.data_ptr(), ws.numel(), T, H, W, offsets.data_ptr(), total, pos.data_ptr(),
              counts.data_ptr(), stream)
    host = counts.cpu().numpy().view(np.uint32)          # copy 2: the packed counts
    return [{"size": [H, W], "counts": host[off[t]:off[t + 1]].tolist()} for t in range(T)]


def _instance_selection(view, img, cfg, thing_lut):
    """The entries of instance_inference (maskformer_model.py:362-401), sorted by their final score, descending and stable
    -> (scores fp32 [T], labels int64 [T], query int64 [T] contiguous).  Shared by ``postprocess`` and ``instance_bits``."""
    Q, K = img.Q, img.K
    (H, W), dev, stream = view.out, view.dev, view.stream
    k = min(int(cfg.test_topk_per_image), Q * K)
    sc, idx = img.probs.reshape(-1).topk(k, sorted=True)
    labels = idx % K
    query = idx // K
    if cfg.panoptic_on:                                 # keep only thing classes (:381-389); the boolean index syncs
        keep = thing_lut[labels]
        sc, labels, query = sc[keep], labels[keep], query[keep]
    T = int(sc.shape[0])
    if T == 0:
        return sc, labels, query
    query = query.contiguous()
    scores = torch.empty(T, dtype=torch.float32, device=dev)
    nws = _lib.lib().mpf_seg_instance_workspace_bytes(T, H, W)
    ws = _lib.scratch("seg_infer.instance", dev, stream, nws)
    _lib.call("mpf_seg_instance_scores", dev, *view.args(), query.data_ptr(), sc.data_ptr(), T, scores.data_ptr(), ws.data_ptr(),
              ws.numel(), stream)
    scores, order = scores.sort(descending=True, stable=True)
    return scores, labels[order], query[order].contiguous()


def _instance_boxes(view, query, T):
    """The bounding boxes int32 [T, 4] (XYXY) of the sorted entries' masks: their packed bits (``mpf_seg_instance_bits``, the ``m > 0``
    decision of the dense masks and of the run lengths) go to scratch and ``mask_boxes`` reads them."""
    (H, W), dev = view.out, view.dev
    if not T:
        return torch.zeros((0, 4), dtype=torch.int32, device=dev)
    nwords = (H * W + 63) // 64
    bits = _lib.scratch("seg_infer.box_bits", dev, view.stream, 8 * T * nwords)[:8 * T * nwords].view(torch.int64).view(T, nwords)
    _lib.call("mpf_seg_instance_bits", dev, *view.args(), query.data_ptr(), T, bits.data_ptr(), view.stream)
    return mask_boxes(bits, (H, W))


def _instances(view, img, cfg, thing_lut):
    (H, W), dev = view.out, view.dev
    scores, labels, query = _instance_selection(view, img, cfg, thing_lut)
    T = int(scores.shape[0])
    Boxes, Instances = _structures()
    result = Instances((H, W))
    if cfg.instance_masks == "rle":
        result.pred_masks_rle = _instance_rle(view, query, T) if T else []
    else:
        result.pred_masks = torch.empty((T, H, W), dtype=torch.float32, device=dev)
        if T:
            _lib.call("mpf_seg_instance_masks", dev, *view.args(), query.data_ptr(), T, result.pred_masks.data_ptr(), view.stream)
    result.pred_boxes = Boxes(_instance_boxes(view, query, T).float() if cfg.instance_boxes else torch.zeros(T, 4))
    result.scores = scores
    result.pred_classes = labels
    return result


def _panoptic(view, img, cfg):
    Q = img.Q
    (H, W), dev, stream = view.out, view.dev, view.stream
    code = torch.empty((H, W), dtype=torch.int32, device=dev)
    _lib.call("mpf_seg_panoptic_areas", dev, *view.args(), img.kept.data_ptr(), img.kept_score.data_ptr(), code.data_ptr(),
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


def _images(who, pred_logits, pred_masks, image_sizes, padded_hw, output_sizes, cfg):
    """The checks of ``postprocess`` and ``instance_bits`` on the head's outputs, then their iteration over the batch: yields
    (view, img, thing_lut) per image: the softmax prologue of the image launched, and the per-batch table of the thing classes
    (None unless instance and panoptic inference run together)."""
    if not (pred_masks.is_cuda and pred_logits.is_cuda):
        raise RuntimeError(f"{who}: Not implemented on the CPU (device tensors only)")
    N, Q, K1 = pred_logits.shape
    K = K1 - 1
    if K != cfg.num_classes:
        raise ValueError(f"pred_logits has {K} classes + no-object, config {cfg.num_classes}")
    if pred_masks.dim() != 4 or pred_masks.shape[:2] != (N, Q):
        raise ValueError(f"pred_masks {tuple(pred_masks.shape)} does not match pred_logits {tuple(pred_logits.shape)}")
    pm = _planes(pred_masks)
    dev = pm.device
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
        view = _View(pm, n, image_sizes[n], padded_hw, output_sizes[n], stream)
        yield view, _Image(logits[n].contiguous(), K, cfg.object_mask_threshold, dev, stream, n), thing_lut


def postprocess(pred_logits, pred_masks, image_sizes, padded_hw, output_sizes, cfg):
    """The reference's eval branch after the head (maskformer_model.py:236-279).

    pred_logits [N, Q, K+1] (any float dtype; widened to fp32), pred_masks [N, Q, h, w] fp32 / bf16 with contiguous [h, w]
    planes (a slice of the decoder's [N, L*Q, h, w] tensor is used in place), image_sizes [(hi, wi)] per image,
    padded_hw = the padded batch size (images.tensor.shape[-2:]), output_sizes [(height, width)] per image.
    -> list of dicts with "sem_seg" [K, height, width], "panoptic_seg" (ids int32 [height, width], segments_info) and
    "instances" (pred_masks [T, height, width] 0/1 fp32, pred_boxes zeros, scores, pred_classes), per the *_on flags.
    cfg.semantic_labels: "sem_seg_labels" int32 [height, width] in place of "sem_seg"; cfg.instance_masks == "rle":
    instances.pred_masks_rle (list of T {"size", "counts"} dicts) in place of pred_masks; cfg.instance_boxes: pred_boxes fp32
    [T, 4] XYXY on the device, the bounding boxes of the masks (``mask_boxes``), in place of the zeros."""
    out = []
    for view, img, thing_lut in _images("postprocess", pred_logits, pred_masks, image_sizes, padded_hw, output_sizes, cfg):
        res = {}
        if cfg.semantic_on and cfg.semantic_labels:
            if cfg.sem_seg_postprocess_before_inference:
                res["sem_seg_labels"] = _semantic_labels(view, img)
            else:   # the scores on the cropped padded grid (network resolution), then resize + argmax in one pass
                res["sem_seg_labels"] = _labels_resize(view, _semantic(view, img, view.image))
        elif cfg.semantic_on:
            if cfg.sem_seg_postprocess_before_inference:
                res["sem_seg"] = _semantic(view, img)
            else:   # inference on the cropped padded grid, then the reference's own resize of the K planes (:264-265)
                r = _semantic(view, img, view.image)
                res["sem_seg"] = F.interpolate(r[None], size=view.out, mode="bilinear", align_corners=False)[0]
        if cfg.panoptic_on:
            res["panoptic_seg"] = _panoptic(view, img, cfg)
        if cfg.instance_on:
            res["instances"] = _instances(view, img, cfg, thing_lut)
        out.append(res)
    return out


def instance_bits(pred_logits, pred_masks, image_sizes, padded_hw, output_sizes, cfg):
    """The "instances" of ``postprocess`` (same arguments) with their masks as packed bits, for ``InstanceAP``: per image a dict
    with "bits" int64 [T, nwords] on the device (position p = x * H + y, 64 per word, bit b of word j = position 64 j + b, zero at
    and past H * W), "size" (H, W), "scores" and "pred_classes".  Selection, scores and order are those of ``postprocess``; the
    dense [T, H, W] masks are never written.  cfg.instance_boxes: also "boxes" int32 [T, 4], ``mask_boxes`` of the bits."""
    if not cfg.instance_on:
        raise ValueError("instance_bits needs instance_on")
    out = []
    for view, img, thing_lut in _images("instance_bits", pred_logits, pred_masks, image_sizes, padded_hw, output_sizes, cfg):
        H, W = view.out
        scores, labels, query = _instance_selection(view, img, cfg, thing_lut)
        T = int(scores.shape[0])
        bits = torch.empty((T, (H * W + 63) // 64), dtype=torch.int64, device=view.dev)
        if T:
            _lib.call("mpf_seg_instance_bits", view.dev, *view.args(), query.data_ptr(), T, bits.data_ptr(), view.stream)
        res = {"bits": bits, "size": (H, W), "scores": scores, "pred_classes": labels}
        if cfg.instance_boxes:
            res["boxes"] = mask_boxes(bits, (H, W))
        out.append(res)
    return out


# ---- video instance segmentation ------------------------------------------------------------------------------------------------
VIDEO_MASK_FORMS = ("dense", "bits", "rle")


@dataclass
class VideoInferenceConfig:
    """The inference attributes of the reference's ``VideoMaskFormer`` (mask2former_video/video_maskformer_model.py:255-287)."""
    num_classes: int
    num_queries: int = 100
    topk: int = 10                      # the reference hard-codes 10 (:260)
    masks: str = "dense"                # "dense": bool [T, F, H, W]; "bits": packed words and frame areas; "rle": uncompressed COCO RLE

    def __post_init__(self):
        if self.masks not in VIDEO_MASK_FORMS:
            raise ValueError(f"masks must be one of {VIDEO_MASK_FORMS}, got {self.masks!r}")
        if int(self.topk) <= 0:
            raise ValueError("topk must be positive")

    @classmethod
    def from_video_maskformer(cls, model, masks="dense"):
        """Read the attributes of a reference ``VideoMaskFormer`` instance."""
        return cls(num_classes=int(model.sem_seg_head.num_classes), num_queries=int(model.num_queries), masks=masks)


def bits_rle(bits, size):
    """Packed masks int64 [M, nwords] of ``size`` (H, W) on the device -> M uncompressed COCO RLE dicts {"size", "counts"}: the count /
    scan / scatter / difference passes of the instance route on bits the caller holds already (``mpf_seg_bits_rle_count`` /
    ``_write``).  Two device-to-host copies whatever M is: the offsets, then the counts."""
    bits = _bits_arg(bits, "bits")
    H, W = _bits_size(bits, size, "bits_rle")
    M, dev = bits.shape[0], bits.device
    if M == 0:
        return []
    stream = _lib.stream_ptr(dev)
    ws = _lib.scratch("seg_video.rle", dev, stream, _lib.lib().mpf_seg_bits_rle_workspace_bytes(M, H, W))
    offsets = torch.empty(M + 1, dtype=torch.int64, device=dev)
    _lib.call("mpf_seg_bits_rle_count", dev, bits.data_ptr(), M, H, W, offsets.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    off = offsets.cpu().numpy()                          # copy 1: where every mask's counts lie
    total = int(off[M])
    pos = _lib.scratch("seg_video.rle_pos", dev, stream, 4 * total)
    counts = torch.empty(total, dtype=torch.int32, device=dev)
    _lib.call("mpf_seg_bits_rle_write", dev, bits.data_ptr(), ws.data_ptr(), ws.numel(), M, H, W, offsets.data_ptr(), total, pos.data_ptr(),
              counts.data_ptr(), stream)
    host = counts.cpu().numpy().view(np.uint32)          # copy 2: the packed counts
    return [{"size": [H, W], "counts": host[off[m]:off[m + 1]].tolist()} for m in range(M)]


def postprocess_video(pred_logits, pred_masks, image_size, padded_hw, output_size, cfg):
    """The reference's video eval branch after the head (mask2former_video/video_maskformer_model.py:204-225 and inference_video,
    :255-287) for ONE clip: pred_logits [Q, K+1] (any float dtype; widened to fp32), pred_masks [Q, F, h, w] fp32 / bf16 with
    contiguous [h, w] planes (a slice of a larger decoder output is read in place), image_size (hi, wi) of the frames on the padded
    grid, padded_hw = images.tensor.shape[-2:], output_size (height, width), cfg a ``VideoInferenceConfig``.

    The top ``cfg.topk`` (query, class) entries are selected first and only their F planes are resampled
    (``seg_video_bits_kernel``): the reference's [Q, F, Hp, Wp] upsampled tensor never exists.  There is no mask-score factor: the
    video route has none.  -> the reference's ``video_output`` dict, "image_size" (height, width) and, by ``cfg.masks``:
    * "dense": "pred_scores" / "pred_labels" python lists, "pred_masks" bool [T, F, height, width];
    * "rle":   the same lists and "pred_masks_rle", T lists of F {"size", "counts"} dicts (uncompressed, column-major);
    * "bits":  "bits" int64 [T, F, nwords] (``instance_bits``' layout per frame), "frame_area" int32 [T, F], "size", and
      "pred_scores" / "pred_labels" as device tensors: no device-to-host copy at all (the form ``TubeAP.update`` takes).
    Every form carries "pred_queries", the query of each entry.  An empty ``pred_logits`` gives the reference's empty result.

    Deviations from the reference, by design:
    * the entries are sorted by score, descending and stable (the reference's ``topk(sorted=False)`` order is unspecified);
    * the dense masks stay on the device (the reference returns a list of CPU tensors);
    * bf16 logits are widened on load and resampled in fp32."""
    if not (pred_masks.is_cuda and pred_logits.is_cuda):
        raise RuntimeError("postprocess_video: Not implemented on the CPU (device tensors only)")
    if pred_logits.dim() != 2 or pred_masks.dim() != 4 or pred_masks.shape[0] != pred_logits.shape[0]:
        raise ValueError(f"one clip: pred_logits [Q, K+1] and pred_masks [Q, F, h, w], got {tuple(pred_logits.shape)} and "
                         f"{tuple(pred_masks.shape)}")
    Q, K = pred_logits.shape[0], pred_logits.shape[1] - 1
    if Q and K != cfg.num_classes:
        raise ValueError(f"pred_logits has {K} classes + no-object, config {cfg.num_classes}")
    H, W = int(output_size[0]), int(output_size[1])
    F_ = pred_masks.shape[1]
    pm = _planes(pred_masks)
    dev = pm.device
    stream = _lib.stream_ptr(dev)
    nwords = (H * W + 63) // 64
    if Q == 0 or F_ == 0:
        sc = torch.empty(0, dtype=torch.float32, device=dev)
        labels = query = torch.empty(0, dtype=torch.int64, device=dev)
    else:
        img = _Image(pred_logits.detach().float().contiguous(), K, 0.0, dev, stream, "video")
        sc, idx = img.probs.reshape(-1).topk(min(int(cfg.topk), Q * K), sorted=True)
        sc, order = sc.sort(descending=True, stable=True)
        idx = idx[order]
        labels, query = idx % K, (idx // K).contiguous()
    T = int(sc.shape[0])
    bits = torch.empty((T, F_, nwords), dtype=torch.int64, device=dev)
    frame_area = torch.empty((T, F_), dtype=torch.int32, device=dev)
    dense = torch.empty((T, F_, H, W), dtype=torch.bool, device=dev) if cfg.masks == "dense" else None
    if T:
        _lib.call("mpf_seg_video_bits", dev, pm.data_ptr(), pm.stride(0), pm.stride(1), _lib.DTYPE[pm.dtype], Q, F_, pm.shape[2], pm.shape[3],
                  int(padded_hw[0]), int(padded_hw[1]), int(image_size[0]), int(image_size[1]), H, W, query.data_ptr(), T, bits.data_ptr(),
                  frame_area.data_ptr(), _lib.ptr(dense), stream)
    out = {"image_size": (H, W)}
    if cfg.masks == "bits":
        out.update(pred_scores=sc, pred_labels=labels, pred_queries=query, bits=bits, frame_area=frame_area, size=(H, W))
        return out
    out.update(pred_scores=sc.tolist(), pred_labels=labels.tolist(), pred_queries=query.tolist())
    if cfg.masks == "dense":
        out["pred_masks"] = dense
    else:
        rle = bits_rle(bits.view(T * F_, nwords), (H, W))
        out["pred_masks_rle"] = [rle[t * F_:(t + 1) * F_] for t in range(T)]
    return out


# ---- semantic test-time augmentation --------------------------------------------------------------------------------------------
TTA_ADD, TTA_HFLIP = 1, 2     # the mode bits of mpf_seg_tta_accumulate / mpf_seg_tta_resize_add


class SemanticTTA:
    """The accumulation of the reference's ``SemanticSegmentorWithTTA._inference_one_image`` (test_time_augmentation.py:71-98)
    for ONE image: ``sem_seg = (sum_v flip_v(S_v)) / V`` over the views in the order they are added, S_v = the view's "sem_seg" at
    the output size (``cfg.sem_seg_postprocess_before_inference`` as in ``postprocess``), flip_v = the W axis of that output
    reversed where the view was flipped.  Every view goes from its logits into one fp32 [K, H, W] accumulator
    (``seg_tta_accumulate_kernel``, in "after" mode through ``seg_tta_resize_add_kernel``): no per-view [K, H, W] tensor, no flip
    copy.  "After" mode does hold one view's [K, hi, wi] scores at a time, in native scratch that grows to the largest view and
    stays allocated between images.  With ``cfg.semantic_labels`` the accumulator is native scratch (one image at a time per stream) and ``result`` gives
    the argmax of the mean, bit for bit that of the dense result.  ``add`` and ``result`` make no device-to-host copy."""

    def __init__(self, cfg):
        if not cfg.semantic_on:
            raise ValueError("SemanticTTA needs semantic_on (the reference has test-time augmentation for sem_seg only)")
        self.cfg = cfg
        self.reset()

    def reset(self):
        self._acc, self._shape, self._count = None, None, 0

    def add(self, pred_logits, pred_masks, image_size, padded_hw, output_size, hflip=False):
        """One view: pred_logits [Q, K+1] or [1, Q, K+1], pred_masks [Q, h, w] or [1, Q, h, w] (fp32 / bf16), the view's image size
        and padded size, the output size of the image (the same for every view), and whether the view was flipped."""
        cfg = self.cfg
        if pred_logits.dim() == 3 and pred_logits.shape[0] == 1:
            pred_logits = pred_logits[0]
        if pred_masks.dim() == 4 and pred_masks.shape[0] == 1:
            pred_masks = pred_masks[0]
        if pred_logits.dim() != 2 or pred_masks.dim() != 3 or pred_masks.shape[0] != pred_logits.shape[0]:
            raise ValueError(f"one view at a time: pred_logits {tuple(pred_logits.shape)}, pred_masks {tuple(pred_masks.shape)}")
        K = pred_logits.shape[1] - 1
        H, W = int(output_size[0]), int(output_size[1])
        if K != cfg.num_classes:
            raise ValueError(f"pred_logits has {K} classes + no-object, config {cfg.num_classes}")
        if self._count and (K, H, W) != self._shape:
            raise ValueError(f"every view of an image has the same classes and output size: got {(K, H, W)}, first view {self._shape}")
        if not (pred_masks.is_cuda and pred_logits.is_cuda):
            raise RuntimeError("SemanticTTA.add: Not implemented on the CPU (device tensors only)")
        pm = _planes(pred_masks[None])
        dev = pm.device
        stream = _lib.stream_ptr(dev)
        if not self._count:
            self._shape = (K, H, W)
            if cfg.semantic_labels:
                self._acc = _lib.scratch("seg_infer.tta_acc", dev, stream, 4 * K * H * W)[:4 * K * H * W].view(torch.float32).view(K, H, W)
            else:
                self._acc = torch.empty((K, H, W), dtype=torch.float32, device=dev)
        elif dev != self._acc.device:
            raise RuntimeError(f"view on {dev}, the accumulator on {self._acc.device}")
        view = _View(pm, 0, image_size, padded_hw, (H, W), stream)
        img = _Image(pred_logits.detach().float().contiguous(), K, cfg.object_mask_threshold, dev, stream, "tta")
        mode = (TTA_ADD if self._count else 0) | (TTA_HFLIP if hflip else 0)
        if cfg.sem_seg_postprocess_before_inference:
            _lib.call("mpf_seg_tta_accumulate", dev, *view.args(), img.probs.data_ptr(), K, mode, self._acc.data_ptr(), stream)
        else:   # the scores on the cropped padded grid (store mode, never mirrored), then resize + flip + add in one pass
            hi, wi = view.image
            r = _lib.scratch("seg_infer.tta_scores", dev, stream, 4 * K * hi * wi)
            _lib.call("mpf_seg_tta_accumulate", dev, *view.args(view.image), img.probs.data_ptr(), K, 0, r.data_ptr(), stream)
            _lib.call("mpf_seg_tta_resize_add", dev, r.data_ptr(), K, hi, wi, H, W, mode, self._acc.data_ptr(), stream)
        self._count += 1

    def result(self):
        """-> {"sem_seg": fp32 [K, H, W]} (the accumulator itself, divided in place) or, with cfg.semantic_labels,
        {"sem_seg_labels": int32 [H, W]}; then ready for the next image."""
        if not self._count:
            raise RuntimeError("SemanticTTA.result: no view was added")
        acc, (K, H, W), dev = self._acc, self._shape, self._acc.device
        stream = _lib.stream_ptr(dev)
        if self.cfg.semantic_labels:
            labels = torch.empty((H, W), dtype=torch.int32, device=dev)
            _lib.call("mpf_seg_tta_finish", dev, acc.data_ptr(), K, H, W, self._count, labels.data_ptr(), stream)
            res = {"sem_seg_labels": labels}
        else:
            _lib.call("mpf_seg_tta_finish", dev, acc.data_ptr(), K, H, W, self._count, None, stream)
            res = {"sem_seg": acc}
        self.reset()
        return res


# ---- semantic evaluation on the device ------------------------------------------------------------------------------------------
class SemSegConfusion:
    """The per-pixel part of detectron2's ``SemSegEvaluator``: the (K+1) x (K+1) confusion counts of predicted label against
    ground truth (row = prediction, column = ground truth, index K = ignored / out of range), accumulated on the device by
    ``mpf_seg_confusion_add``.  ``update`` launches and returns; only ``matrix`` copies to the host."""

    def __init__(self, num_classes, ignore_label=255, device="cuda:0"):
        self.num_classes = int(num_classes)
        self.ignore_label = int(ignore_label)
        self.device = torch.device(device)
        if self.num_classes <= 0:
            raise ValueError("num_classes must be positive")
        self._conf = None

    def _buffer(self):
        if self._conf is None:
            if self.device.type != "cuda":
                raise RuntimeError("SemSegConfusion: Not implemented on the CPU (device tensors only)")
            self._conf = torch.zeros((self.num_classes + 1) ** 2, dtype=torch.int64, device=self.device)
        return self._conf

    def reset(self):
        if self._conf is not None:
            self._conf.zero_()

    def update(self, labels, gt):
        """labels: int32 [H, W] on the device ("sem_seg_labels"); gt: any integer dtype, [H, W]."""
        if labels.dim() != 2 or tuple(labels.shape) != tuple(gt.shape):
            raise ValueError(f"labels {tuple(labels.shape)} and gt {tuple(gt.shape)} must be the same [H, W]")
        if labels.dtype != torch.int32:
            raise TypeError(f"labels must be int32, got {labels.dtype}")
        if gt.dtype.is_floating_point or gt.dtype.is_complex or gt.dtype == torch.bool:
            raise TypeError(f"gt must be an integer tensor, got {gt.dtype}")
        conf = self._buffer()
        if labels.device != conf.device:
            raise RuntimeError(f"labels are on {labels.device}, the counters on {conf.device}")
        labels = labels.contiguous()
        gt = gt.to(device=conf.device, dtype=torch.int32).contiguous()
        _lib.call("mpf_seg_confusion_add", conf.device, labels.data_ptr(), gt.data_ptr(), labels.numel(), self.num_classes,
                  self.ignore_label, conf.data_ptr(), _lib.stream_ptr(conf.device))

    def matrix(self):
        """-> int64 numpy [K+1, K+1] (one device-to-host copy)"""
        k1 = self.num_classes + 1
        if self._conf is None:
            return np.zeros((k1, k1), dtype=np.int64)
        return self._conf.cpu().numpy().reshape(k1, k1)

    def results(self, class_names=None):
        return confusion_results(self.matrix(), class_names)


def confusion_results(conf, class_names=None):
    """detectron2's ``SemSegEvaluator.evaluate`` on a [K+1, K+1] confusion matrix (row = prediction): mIoU, fwIoU, mACC, pACC and
    the per-class IoU-{name} / ACC-{name} (x 100; names default to the class index)."""
    conf = np.asarray(conf, dtype=np.int64)
    k = conf.shape[0] - 1
    if conf.shape != (k + 1, k + 1) or k <= 0:
        raise ValueError(f"confusion matrix must be [K+1, K+1], got {conf.shape}")
    if class_names is not None and len(class_names) != k:
        raise ValueError(f"{len(class_names)} class names for {k} classes")
    c = conf[:-1, :-1]
    tp = np.diag(c).astype(np.float64)
    pos_gt = c.sum(0).astype(np.float64)
    pos_pred = c.sum(1).astype(np.float64)
    acc = np.full(k, np.nan)
    iou = np.full(k, np.nan)
    acc_valid = pos_gt > 0
    acc[acc_valid] = tp[acc_valid] / pos_gt[acc_valid]
    union = pos_gt + pos_pred - tp
    iou_valid = acc_valid & (union > 0)
    iou[iou_valid] = tp[iou_valid] / union[iou_valid]
    n_gt = pos_gt.sum()
    class_weights = pos_gt / n_gt if n_gt > 0 else np.zeros(k)
    res = {
        "mIoU": 100 * (iou[iou_valid].sum() / iou_valid.sum()) if iou_valid.any() else float("nan"),
        "fwIoU": 100 * float((iou[iou_valid] * class_weights[iou_valid]).sum()) if n_gt > 0 else float("nan"),
        "mACC": 100 * (acc[acc_valid].sum() / acc_valid.sum()) if acc_valid.any() else float("nan"),
        "pACC": 100 * tp.sum() / n_gt if n_gt > 0 else float("nan"),
    }
    names = [str(i) for i in range(k)] if class_names is None else list(class_names)
    for i, name in enumerate(names):
        res[f"IoU-{name}"] = 100 * float(iou[i])
        res[f"ACC-{name}"] = 100 * float(acc[i])
    return {key: float(v) for key, v in res.items()}


# ---- panoptic evaluation on the device ------------------------------------------------------------------------------------------
PQ_CROWD, PQ_CROWD_WINS = 1, 2      # the gt_flags bits of mpf_seg_pq_match


def _pq_side(segments, K, void_id, what, crowd=False):
    """One side's listed segments -> (ids ascending, categories, flags) as int32 arrays; ValueError on what the host can see."""
    ids, cats, flags = [], [], []
    winner = {}                                         # category -> position of the crowd segment that comes last (line 118)
    for n, s in enumerate(segments):
        i, c = int(s["id"]), int(s["category_id"])
        if not 0 <= c < K:
            raise ValueError(f"{what}: category_id {c} of segment {i} is outside [0, {K})")
        if i < 0 or i >= 1 << 31 or i == void_id:
            raise ValueError(f"{what}: segment id {i} is negative, too large or the void id")
        ids.append(i)
        cats.append(c)
        flags.append(PQ_CROWD if crowd and int(s.get("iscrowd", 0)) == 1 else 0)
        if flags[-1]:
            winner[c] = n
    if len(set(ids)) != len(ids):
        raise ValueError(f"{what}: duplicate segment ids")
    for n in winner.values():
        flags[n] |= PQ_CROWD_WINS
    order = np.argsort(np.asarray(ids, dtype=np.int64), kind="stable")
    pick = lambda v: np.asarray(v, dtype=np.int32)[order]      # noqa: E731
    return pick(ids), pick(cats), pick(flags)


class PanopticQuality:
    """The per-image part of panopticapi's ``pq_compute`` (``pq_compute_single_core``; the reference carries the same body as
    ``pq_compute_single_image`` in tools/evaluate_pq_for_semantic_segmentation.py:41-136): tp / fp / fn and the summed IoU per
    category, accumulated on the device by ``mpf_seg_pq_pairs`` + ``mpf_seg_pq_match`` from the id map ``postprocess`` returns.
    ``update`` / ``update_semantic`` launch and return; only ``stats`` copies to the host.  The counters are integers and the IoU
    sum is float64 in the single-process reference's order, so ``stats`` is that reference's ``PQStat`` bit for bit.

    Deviation: a ground-truth segment's area is its pixel count in ``gt`` (panopticapi reads the annotation's "area", which is the
    same number for a consistent annotation)."""

    def __init__(self, num_classes, thing_ids, void_id=0, device="cuda:0"):
        self.num_classes = int(num_classes)
        self.thing_ids = frozenset(int(i) for i in thing_ids)
        self.void_id = int(void_id)
        self.device = torch.device(device)
        if self.num_classes <= 0:
            raise ValueError("num_classes must be positive")
        self._state = None          # int64 [4K + 1]: tp, fp, fn, iou (float64 bits), error count

    def _buffers(self):
        if self._state is None:
            if self.device.type != "cuda":
                raise RuntimeError("PanopticQuality: Not implemented on the CPU (device tensors only)")
            self._state = torch.zeros(4 * self.num_classes + 1, dtype=torch.int64, device=self.device)
        p, K = self._state.data_ptr(), self.num_classes
        return [p + 8 * K * i for i in range(5)]           # tp, fp, fn, iou, err

    def reset(self):
        if self._state is not None:
            self._state.zero_()

    def _check_maps(self, pred, gt, rgb_ok):
        if self.device.type != "cuda" or not (pred.is_cuda and gt.is_cuda):
            raise RuntimeError("PanopticQuality: Not implemented on the CPU (device tensors only)")
        if pred.dim() != 2 or pred.dtype != torch.int32:
            raise ValueError(f"the prediction must be int32 [H, W], got {pred.dtype} {tuple(pred.shape)}")
        rgb = rgb_ok and gt.dim() == 3
        if rgb and (gt.dtype != torch.uint8 or gt.shape[2] != 3):
            raise ValueError(f"an RGB ground truth must be uint8 [H, W, 3], got {gt.dtype} {tuple(gt.shape)}")
        if tuple(gt.shape[:2]) != tuple(pred.shape) or gt.dim() != (3 if rgb else 2):
            raise ValueError(f"prediction {tuple(pred.shape)} and ground truth {tuple(gt.shape)} must be the same [H, W]")
        if pred.numel() == 0:
            raise ValueError("empty image")
        if pred.device != self.device or gt.device != self.device:
            raise RuntimeError(f"maps on {pred.device} / {gt.device}, the counters on {self.device}")
        return rgb

    def _run(self, pred, gt, fmt, G, S, gt_ids, gt_base, pred_ids, pred_base, gt_cat, gt_flags, pred_cat, implicit):
        dev = self.device
        stream = _lib.stream_ptr(dev)
        tp, fp, fn, iou, err = self._buffers()
        nbytes = _lib.lib().mpf_seg_pq_workspace_bytes(G, S)
        table = _lib.scratch("seg_pq.table", dev, stream, nbytes, zeroed=True)     # zero between calls: the match kernel clears it
        _lib.call("mpf_seg_pq_pairs", dev, pred.data_ptr(), gt.data_ptr(), fmt, pred.numel(), gt_ids, G, gt_base, pred_ids, S, pred_base,
                  self.void_id, table.data_ptr(), table.numel(), stream)
        _lib.call("mpf_seg_pq_match", dev, table.data_ptr(), table.numel(), G, S, self.num_classes, gt_cat, gt_flags, pred_cat, implicit,
                  tp, fp, fn, iou, err, stream)

    def update(self, pred_ids, segments_info, gt, gt_segments):
        """pred_ids int32 [H, W] and segments_info ({"id", "category_id"}) as ``postprocess`` returns them; gt int32 [H, W] ids or
        uint8 [H, W, 3] RGB (id = R + 256 G + 65536 B) on the device; gt_segments: {"id", "category_id", "iscrowd"} with contiguous
        category ids, in the annotation's order."""
        from . import _h2d
        K = self.num_classes
        rgb = self._check_maps(pred_ids, gt, True)
        if not rgb and gt.dtype != torch.int32:
            raise ValueError(f"a ground-truth id map must be int32, got {gt.dtype}")
        g_ids, g_cat, g_flags = _pq_side(gt_segments, K, self.void_id, "gt_segments", crowd=True)
        p_ids, p_cat, _ = _pq_side(segments_info, K, self.void_id, "segments_info")
        G, S = len(g_ids), len(p_ids)
        ptrs = [None] * 5
        if G + S:
            meta = _h2d.upload(np.concatenate([g_ids, p_ids, g_cat, g_flags, p_cat]), self.device)
            self._meta = meta                               # (the caching allocator keeps it valid on this stream anyway)
            off = np.cumsum([0, G, S, G, G])
            ptrs = [meta.data_ptr() + 4 * int(o) for o in off]

        def side(ids, n, ptr):
            """-> (table pointer or None, base): a contiguous id range needs no table"""
            if n == 0:
                return None, 0
            if int(ids[-1]) - int(ids[0]) == n - 1:
                return None, int(ids[0])
            return ptr, 0
        gp, gbase = side(g_ids, G, ptrs[0])
        pp, pbase = side(p_ids, S, ptrs[1])
        self._run(pred_ids.contiguous(), gt.contiguous(), 1 if rgb else 0, G, S, gp, gbase, pp, pbase,
                  ptrs[2] if G else None, ptrs[3] if G else None, ptrs[4] if S else None, 0)

    def update_semantic(self, pred_labels, gt_labels):
        """The route of the reference tool (:50-60): pred_labels int32 [H, W], gt_labels any integer dtype [H, W]; every class with
        a pixel is one segment of its side, ``void_id`` is the ignore label.  A prediction outside [0, K) is an error at ``stats``."""
        self._check_maps(pred_labels, gt_labels, False)
        if gt_labels.dtype.is_floating_point or gt_labels.dtype.is_complex or gt_labels.dtype == torch.bool:
            raise ValueError(f"gt_labels must be an integer tensor, got {gt_labels.dtype}")
        K = self.num_classes
        gt = gt_labels.to(dtype=torch.int32).contiguous()
        self._run(pred_labels.contiguous(), gt, 0, K, K, None, 0, None, 0, None, None, None, 1)

    def stats(self):
        """-> {"tp", "fp", "fn"} int64 [K] and "iou" float64 [K] (one device-to-host copy); ValueError where the reference raises
        KeyError: a predicted id that segments_info does not list, or a listed prediction without a pixel."""
        K = self.num_classes
        if self._state is None:
            host = np.zeros(4 * K + 1, dtype=np.int64)
        else:
            host = self._state.cpu().numpy()
        if host[4 * K]:
            raise ValueError(f"PanopticQuality: {int(host[4 * K])} prediction pixels / segments disagree with their segments_info "
                             "(an id that is not listed, or a listed segment without a pixel)")
        return {"tp": host[:K].copy(), "fp": host[K:2 * K].copy(), "fn": host[2 * K:3 * K].copy(),
                "iou": host[3 * K:4 * K].copy().view(np.float64)}

    @staticmethod
    def combine(list_of_stats):
        """The sum over ranks or shards, in list order."""
        out = None
        for s in list_of_stats:
            if out is None:
                out = {k: np.array(s[k], dtype=np.float64 if k == "iou" else np.int64) for k in ("tp", "fp", "fn", "iou")}
            else:
                for k in out:
                    out[k] = out[k] + np.asarray(s[k], dtype=out[k].dtype)
        if out is None:
            raise ValueError("combine: no stats")
        return out

    def results(self):
        """The nine keys of detectron2's ``COCOPanopticEvaluator`` (x 100)."""
        r = pq_results(self.stats(), self.thing_ids)
        out = {}
        for name, suffix in (("All", ""), ("Things", "_th"), ("Stuff", "_st")):
            for m in ("pq", "sq", "rq"):
                out[m.upper() + suffix] = 100 * r[name][m]
        return out


def pq_results(stats, thing_ids):
    """panopticapi's ``PQStat.pq_average`` for all / thing / stuff categories -> {"All", "Things", "Stuff": {pq, sq, rq, n},
    "per_class": {category: {pq, sq, rq}}}.  A category without entries is left out of n; a group with n == 0 gives nan (the
    reference divides by zero there)."""
    tp, fp, fn = (np.asarray(stats[k], dtype=np.int64) for k in ("tp", "fp", "fn"))
    iou = np.asarray(stats["iou"], dtype=np.float64)
    K = tp.shape[0]
    things = frozenset(int(i) for i in thing_ids)
    per_class = {}
    for c in range(K):
        t, p, n = int(tp[c]), int(fp[c]), int(fn[c])
        if t + p + n == 0:
            per_class[c] = {"pq": 0.0, "sq": 0.0, "rq": 0.0}
            continue
        den = t + 0.5 * p + 0.5 * n
        per_class[c] = {"pq": float(iou[c]) / den, "sq": float(iou[c]) / t if t != 0 else 0.0, "rq": t / den}
    out = {"per_class": per_class}
    for name, want in (("All", None), ("Things", True), ("Stuff", False)):
        pq = sq = rq = 0.0
        n = 0
        for c in range(K):
            if want is not None and (c in things) != want:
                continue
            if int(tp[c]) + int(fp[c]) + int(fn[c]) == 0:
                continue
            n += 1
            pq += per_class[c]["pq"]
            sq += per_class[c]["sq"]
            rq += per_class[c]["rq"]
        nan = float("nan")
        out[name] = {"pq": pq / n if n else nan, "sq": sq / n if n else nan, "rq": rq / n if n else nan, "n": n}
    return out


# ---- instance mask AP on the device ---------------------------------------------------------------------------------------------
AP_CROWD_RULES = {"coco": 0, "union": 1}      # the crowd_rule argument of mpf_seg_ap_match
COCO_AREA_RNGS = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))     # all, small, medium, large
YTVIS_AREA_RNGS = ((0.0, 1e10), (0.0, 128.0 ** 2), (128.0 ** 2, 256.0 ** 2), (256.0 ** 2, 1e10))    # ytvoseval.py:543
_AP_REC = 4                                   # int64 words of a detection's record


def _bits_arg(bits, what):
    if not bits.is_cuda:
        raise RuntimeError(f"{what}: Not implemented on the CPU (device tensors only)")
    if bits.dim() != 2 or bits.dtype != torch.int64:
        raise ValueError(f"{what} must be packed bits int64 [M, nwords], got {bits.dtype} {tuple(bits.shape)}")
    return bits.contiguous()


def pack_masks(masks):
    """Dense masks [M, H, W] on the device (uint8, bool or float32; non-zero = set) -> packed bits int64 [M, nwords], in the layout
    of ``instance_bits``: position p = x * H + y, 64 positions per word, bit b of word j = position 64 j + b, zero past H * W."""
    if not masks.is_cuda:
        raise RuntimeError("pack_masks: Not implemented on the CPU (device tensors only)")
    if masks.dim() != 3 or masks.shape[1] == 0 or masks.shape[2] == 0:
        raise ValueError(f"masks must be [M, H, W] with H, W > 0, got {tuple(masks.shape)}")
    if masks.dtype not in (torch.uint8, torch.bool, torch.float32):
        raise TypeError(f"masks must be uint8, bool or float32, got {masks.dtype}")
    masks = masks.contiguous()
    M, H, W = masks.shape
    dev = masks.device
    bits = torch.empty((M, (H * W + 63) // 64), dtype=torch.int64, device=dev)
    if M:
        _lib.call("mpf_seg_pack_masks", dev, masks.data_ptr(), _lib.DTYPE[masks.dtype], M, H, W, bits.data_ptr(), _lib.stream_ptr(dev))
    return bits


def mask_pair_counts(a_bits, b_bits):
    """Two sets of packed masks of one image, A [T, nwords] and B [G, nwords] -> (inter int32 [T, G] = the pixels a_t and b_g share,
    area_a int32 [T], area_b int32 [G]), on the device."""
    a, b = _bits_arg(a_bits, "a_bits"), _bits_arg(b_bits, "b_bits")
    if a.device != b.device:
        raise RuntimeError(f"a_bits on {a.device}, b_bits on {b.device}")
    if a.shape[1] != b.shape[1] or a.shape[1] == 0:
        raise ValueError(f"both sides need the same nwords > 0, got {a.shape[1]} and {b.shape[1]}")
    T, G, nwords = a.shape[0], b.shape[0], a.shape[1]
    dev = a.device
    inter = torch.empty((T, G), dtype=torch.int32, device=dev)
    area_a = torch.empty(T, dtype=torch.int32, device=dev)
    area_b = torch.empty(G, dtype=torch.int32, device=dev)
    if T or G:
        _lib.call("mpf_seg_mask_pairs", dev, a.data_ptr() if T else None, T, b.data_ptr() if G else None, G, nwords,
                  inter.data_ptr() if T and G else None, area_a.data_ptr() if T else None, area_b.data_ptr() if G else None,
                  _lib.stream_ptr(dev))
    return inter, area_a, area_b


AP_IOU_TYPES = ("segm", "boundary", "bbox")


def boundary_dilation(H, W, dilation_ratio=0.02):
    """boundary-iou-api's dilation distance for an H x W image: ``int(round(dilation_ratio * sqrt(H^2 + W^2)))`` with python's
    round (halves to even), at least 1."""
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError(f"need H, W > 0, got {H} x {W}")
    return max(1, int(round(float(dilation_ratio) * np.sqrt(H ** 2 + W ** 2))))


def _bits_size(bits, size, what):
    """(H, W) of packed masks, checked against their words"""
    if size is None or len(size) != 2:
        raise ValueError(f"{what}: size must be (H, W), got {size!r}")
    H, W = int(size[0]), int(size[1])
    if H <= 0 or W <= 0 or bits.shape[1] != (H * W + 63) // 64:
        raise ValueError(f"{what}: size {H} x {W} does not fit nwords = {bits.shape[1]} ({(H * W + 63) // 64} expected)")
    return H, W


def mask_boundaries(bits, size, dilation_ratio=0.02, d=None):
    """Packed masks int64 [M, nwords] of an image of ``size`` (H, W) -> their boundaries in the same layout: ``mask & ~eroded``, the
    erosion by ``d`` pixels (3 x 3 element, d iterations, outside the image unset) of boundary-iou-api's ``mask_to_boundary``.
    ``d`` defaults to ``boundary_dilation(H, W, dilation_ratio)``."""
    bits = _bits_arg(bits, "bits")
    H, W = _bits_size(bits, size, "mask_boundaries")
    d = boundary_dilation(H, W, dilation_ratio) if d is None else int(d)
    if d < 1:
        raise ValueError(f"d must be at least 1, got {d}")
    dev = bits.device
    out = torch.empty_like(bits)
    if bits.shape[0]:
        _lib.call("mpf_seg_mask_boundary", dev, bits.data_ptr(), bits.shape[0], H, W, d, out.data_ptr(), _lib.stream_ptr(dev))
    return out


def mask_boxes(bits, size):
    """Packed masks int64 [M, nwords] of an image of ``size`` (H, W), or tubes int64 [T, F, nwords] -> their bounding boxes int32
    [M, 4] (or [T, F, 4]) on the device, XYXY as Detectron2's ``BitMasks.get_bounding_boxes`` gives them (the call the reference's
    instance_inference leaves commented out, maskformer_model.py:393-395): (min x, min y, max x + 1, max y + 1) over the set
    pixels, (0, 0, 0, 0) for an empty mask.  One read of the words, one launch."""
    if not bits.is_cuda:
        raise RuntimeError("mask_boxes: Not implemented on the CPU (device tensors only)")
    tubes = bits.dim() == 3
    flat = _bits_arg(bits.flatten(0, 1) if tubes else bits, "bits")
    H, W = _bits_size(flat, size, "mask_boxes")
    dev = flat.device
    boxes = torch.empty((flat.shape[0], 4), dtype=torch.int32, device=dev)
    if flat.shape[0]:
        _lib.call("mpf_seg_bits_boxes", dev, flat.data_ptr(), flat.shape[0], H, W, boxes.data_ptr(), _lib.stream_ptr(dev))
    return boxes.view(bits.shape[0], bits.shape[1], 4) if tubes else boxes


def boxes_xyxy_to_xywh(boxes):
    """[N, 4] (x0, y0, x1, y1) of any dtype -> float64 [N, 4] (x, y, w, h), the form a COCO json holds and
    ``InstanceAP(iou_type="bbox")`` takes."""
    b = boxes.to(torch.float64).reshape(-1, 4)
    return torch.cat([b[:, :2], b[:, 2:] - b[:, :2]], dim=1)


# ---- COCO ground truth to packed bits: polygons and run lengths ------------------------------------------------------------------
def rle_to_string(counts):
    """pycocotools' ``rleToString``: run lengths -> the COCO "counts" string.  From the third count on the difference to the count
    two places back is stored, in groups of 5 bits, lowest first, bit 0x20 = "more follows", characters offset by 48.  Byte-serial
    and a few hundred bytes long: host work."""
    cnts = [int(c) for c in counts]
    out = []
    for i, c in enumerate(cnts):
        if c < 0:
            raise ValueError(f"counts must be non-negative, got {c}")
        x = c - (cnts[i - 2] if i > 2 else 0)
        more = True
        while more:
            g = x & 0x1f
            x >>= 5                                          # arithmetic: a negative difference ends in -1
            more = (x != -1) if g & 0x10 else (x != 0)
            if more:
                g |= 0x20
            out.append(chr(g + 48))
    return "".join(out)


def rle_from_string(s):
    """pycocotools' ``rleFrString``: the COCO "counts" string (str or bytes) -> the run lengths, a list of ints."""
    data = s.encode("ascii") if isinstance(s, str) else bytes(s)
    cnts = []
    p, n = 0, len(data)
    while p < n:
        x, k, more = 0, 0, True
        while more:
            if p >= n:
                raise ValueError("counts string ends inside a number")
            g = data[p] - 48
            if not 0 <= g < 64:
                raise ValueError(f"counts string holds {chr(data[p])!r}: not a character of the COCO encoding")
            x |= (g & 0x1f) << (5 * k)
            more = bool(g & 0x20)
            p += 1
            k += 1
            if not more and g & 0x10:
                x |= -1 << (5 * k)                           # sign-extend
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def rle_compress(rle):
    """An uncompressed RLE dict {"size", "counts": list} (what ``bits_rle`` and the "rle" forms give) -> the dict a COCO json holds,
    "counts" the string of ``rle_to_string``."""
    return {"size": [int(rle["size"][0]), int(rle["size"][1])], "counts": rle_to_string(rle["counts"])}


_NP2T = {np.dtype(np.float64): torch.float64, np.dtype(np.int64): torch.int64, np.dtype(np.int32): torch.int32}


def _codec_device(device, what):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{what}: Not implemented on the CPU (device tensors only)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _codec_size(size, what):
    if size is None or len(size) != 2:
        raise ValueError(f"{what}: size must be (H, W), got {size!r}")
    H, W = int(size[0]), int(size[1])
    if H <= 0 or W <= 0 or H * W >= 1 << 31:
        raise ValueError(f"{what}: need H, W > 0 and H * W < 2^31, got {H} x {W}")
    return H, W


def _stage(dev, arrays):
    """numpy arrays -> their device copies through ONE pinned staging buffer: one host-to-device copy, every array 8-byte aligned"""
    offs, n = [], 0
    for a in arrays:
        offs.append(n)
        n += (a.nbytes + 7) // 8 * 8
    host = np.zeros(max(n, 8), dtype=np.uint8)
    for a, o in zip(arrays, offs):
        host[o:o + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    d = torch.from_numpy(host).pin_memory().to(dev, non_blocking=True)
    return [d[o:o + a.nbytes].view(_NP2T[a.dtype]) if a.nbytes else torch.empty(0, dtype=_NP2T[a.dtype], device=dev)
            for a, o in zip(arrays, offs)]


def _ring_arrays(polygons, what):
    """the checked rings of a list of objects -> (xy float64 [V, 2], ring_off int64 [R + 1], ring_obj int32 [R])"""
    rings, ring_obj = [], []
    for m, obj in enumerate(polygons):
        if not isinstance(obj, (list, tuple)):
            raise ValueError(f"{what}: object {m} must be a list of rings [x0, y0, x1, y1, ...], got {type(obj).__name__}")
        for ring in obj:
            a = np.asarray(ring, dtype=np.float64).reshape(-1)
            if a.size % 2:
                raise ValueError(f"{what}: object {m} has a ring of odd length {a.size}")
            if a.size < 6:
                raise ValueError(f"{what}: object {m} has a ring of {a.size} numbers: a polygon needs at least 6 (3 vertices)")
            if not np.isfinite(a).all():
                raise ValueError(f"{what}: object {m} has a non-finite coordinate")
            if (np.abs(5.0 * a + 0.5) >= 2.0 ** 31).any():
                raise ValueError(f"{what}: object {m} has a coordinate c with |5 c + .5| >= 2^31")
            rings.append(a)
            ring_obj.append(m)
    ring_off = np.zeros(len(rings) + 1, dtype=np.int64)
    if rings:
        ring_off[1:] = np.cumsum([r.size // 2 for r in rings])
    xy = np.concatenate(rings) if rings else np.zeros(0, dtype=np.float64)
    return xy, ring_off, np.asarray(ring_obj, dtype=np.int32)


def _rle_arrays(rles, H, W, what):
    """the checked run lengths of a list of RLE dicts of one size -> (counts uint32 as int32 bits, off int64 [M + 1]); (H, W) None:
    taken from the first dict -> also (H, W)"""
    runs = []
    for m, r in enumerate(rles):
        if not isinstance(r, dict) or "size" not in r or "counts" not in r:
            raise ValueError(f"{what}: entry {m} must be a dict with \"size\" and \"counts\"")
        sz = (int(r["size"][0]), int(r["size"][1]))
        if H is None:
            H, W = _codec_size(sz, what)
        if sz != (H, W):
            raise ValueError(f"{what}: entry {m} has size {sz[0]} x {sz[1]}, expected {H} x {W}")
        c = r["counts"]
        c = rle_from_string(c) if isinstance(c, (str, bytes, bytearray)) else [int(v) for v in c]
        if any(v < 0 for v in c):
            raise ValueError(f"{what}: entry {m} has a negative count")
        if sum(c) != H * W:
            raise ValueError(f"{what}: the counts of entry {m} sum to {sum(c)}, not H * W = {H * W}")
        runs.append(np.asarray(c, dtype=np.int64))
    off = np.zeros(len(runs) + 1, dtype=np.int64)
    if runs:
        off[1:] = np.cumsum([r.size for r in runs])
    counts = (np.concatenate(runs) if runs else np.zeros(0, dtype=np.int64)).astype(np.uint32).view(np.int32)
    return counts, off, (H, W)


def _toggle_fill(dev, H, W, M, poly, poly_obj, rle, rle_obj):
    """bits int64 [M, nwords] from the toggle planes of both sources: poly = (xy, ring_off), rle = (counts, off), *_obj the object of
    every plane (int32).  The polygon planes come first, so the caller numbers the objects so that (poly_obj, rle_obj) is
    non-decreasing.  One host-to-device copy, one toggle launch per source kind, one fill."""
    nwords = (H * W + 63) // 64
    bits = torch.empty((M, nwords), dtype=torch.int64, device=dev)
    if M == 0:
        return bits
    Rp, Rr = len(poly_obj), len(rle_obj)
    stream = _lib.stream_ptr(dev)
    planes = torch.empty((Rp + Rr, nwords), dtype=torch.int64, device=dev)
    xy, ring_off, counts, off, plane_obj = _stage(dev, [poly[0], poly[1], rle[0], rle[1], np.concatenate([poly_obj, rle_obj]).astype(np.int32)])
    if Rp:
        _lib.call("mpf_seg_poly_toggles", dev, xy.data_ptr(), ring_off.data_ptr(), Rp, H, W, planes.data_ptr(), stream)
    if Rr:
        _lib.call("mpf_seg_rle_toggles", dev, counts.data_ptr(), off.data_ptr(), Rr, H, W, planes[Rp:].data_ptr(), stream)
    _lib.call("mpf_seg_toggles_fill", dev, planes.data_ptr() if Rp + Rr else None, plane_obj.data_ptr() if Rp + Rr else None, Rp + Rr, M, H, W,
              bits.data_ptr(), stream)
    return bits


_NO_POLY = (np.zeros(0, dtype=np.float64), np.zeros(1, dtype=np.int64))
_NO_RLE = (np.zeros(0, dtype=np.int32), np.zeros(1, dtype=np.int64))
_NO_OBJ = np.zeros(0, dtype=np.int32)


def polygon_bits(polygons, size, device="cuda"):
    """COCO polygon segmentations -> packed bits int64 [M, nwords] on the device, as pycocotools' ``frPyObjects`` + ``merge`` decide
    them (``rleFrPoly`` per ring, the union of an object's rings).  ``polygons``: a list over objects, each a list of rings
    [x0, y0, x1, y1, ...] (the "segmentation" list of a COCO annotation; an object without a ring is empty); ``size`` (H, W).
    Only the vertices cross to the device: vertices, ring offsets and the ring -> object table in one staging buffer, one copy.
    ValueError on a ring of odd length, of fewer than 6 numbers (detectron2's filter), with a non-finite coordinate or with
    |5 c + .5| >= 2^31."""
    H, W = _codec_size(size, "polygon_bits")
    xy, ring_off, ring_obj = _ring_arrays(polygons, "polygon_bits")
    dev = _codec_device(device, "polygon_bits")
    return _toggle_fill(dev, H, W, len(polygons), (xy, ring_off), ring_obj, _NO_RLE, _NO_OBJ)


def rle_bits(rles, size=None, device="cuda"):
    """COCO RLE segmentations {"size": [H, W], "counts": list | str | bytes} -> packed bits int64 [M, nwords] on the device
    (pycocotools' ``rleDecode``, never dense: COCO's column-major order is the packed layout's).  Strings are decoded on the host
    (``rle_from_string``); only the run lengths cross.  Checked on the host before anything is launched: all sizes equal (and equal
    to ``size`` where given; an empty list needs it), every mask's counts summing to H * W."""
    H, W = _codec_size(size, "rle_bits") if size is not None else (None, None)
    if H is None and not len(rles):
        raise ValueError("rle_bits: size must be given for an empty list")
    counts, off, (H, W) = _rle_arrays(rles, H, W, "rle_bits")
    dev = _codec_device(device, "rle_bits")
    return _toggle_fill(dev, H, W, len(rles), _NO_POLY, _NO_OBJ, (counts, off), np.arange(len(rles), dtype=np.int32))


def segmentation_bits(segms, size, device="cuda"):
    """A mixed list of COCO segmentations -> packed bits int64 [M, nwords] on the device, in input order (pycocotools' ``annToRLE``
    without the dense mask): an entry is a polygon list, an RLE dict with a list, or one with a string, or None (all zero: a
    YouTube-VIS frame without annotation).  One toggle-plane batch per source kind, one fill, one host-to-device copy (a second,
    of M indices, where both kinds occur: the rows are then put back in input order)."""
    H, W = _codec_size(size, "segmentation_bits")
    poly_idx = [i for i, s in enumerate(segms) if isinstance(s, (list, tuple))]
    rle_idx = [i for i, s in enumerate(segms) if isinstance(s, dict)]
    for i, s in enumerate(segms):
        if s is not None and not isinstance(s, (list, tuple, dict)):
            raise ValueError(f"segmentation_bits: entry {i} is a {type(s).__name__}: expected polygons, an RLE dict or None")
    xy, ring_off, ring_obj = _ring_arrays([segms[i] for i in poly_idx], "segmentation_bits")
    counts, off, _ = _rle_arrays([segms[i] for i in rle_idx], H, W, "segmentation_bits")
    dev = _codec_device(device, "segmentation_bits")
    M = len(segms)
    if not poly_idx or not rle_idx:                          # one kind: its objects keep their places, the others have no plane
        return _toggle_fill(dev, H, W, M, (xy, ring_off), np.asarray(poly_idx, dtype=np.int32)[ring_obj] if poly_idx else _NO_OBJ,
                            (counts, off), np.asarray(rle_idx, dtype=np.int32))
    # both kinds: polygons first, then run lengths (plane_obj non-decreasing), and the rows put back in input order
    part = _toggle_fill(dev, H, W, len(poly_idx) + len(rle_idx), (xy, ring_off), ring_obj, (counts, off),
                        len(poly_idx) + np.arange(len(rle_idx), dtype=np.int32))
    bits = part.new_zeros((M, part.shape[1]))
    bits[_stage(dev, [np.asarray(poly_idx + rle_idx, dtype=np.int64)])[0]] = part
    return bits


def unpack_masks(bits, size, dtype=torch.bool):
    """Packed bits int64 [M, nwords] of ``size`` (H, W) -> dense masks [M, H, W] on the device, row-major, bool (default), uint8 or
    float32: the inverse of ``pack_masks``, for consumers that want dense targets."""
    bits = _bits_arg(bits, "bits")
    H, W = _bits_size(bits, size, "unpack_masks")
    if dtype not in (torch.bool, torch.uint8, torch.float32):
        raise TypeError(f"dtype must be bool, uint8 or float32, got {dtype}")
    M, dev = bits.shape[0], bits.device
    out = torch.empty((M, H, W), dtype=torch.uint8, device=dev)
    if M:
        _lib.call("mpf_seg_unpack_masks", dev, bits.data_ptr(), M, H, W, out.data_ptr(), _lib.stream_ptr(dev))
    return out.view(torch.bool) if dtype == torch.bool else out.to(dtype)


def polygon_masks(polygons, size, dtype=torch.bool, device="cuda"):
    """COCO polygons -> dense masks [M, H, W] on the device: the device form of the training mappers' ``convert_coco_poly_to_mask``
    / detectron2's ``polygons_to_bitmask`` (``polygon_bits``, then ``unpack_masks``); only the vertices cross."""
    return unpack_masks(polygon_bits(polygons, size, device=device), size, dtype=dtype)


class InstanceAP:
    """The per-image part of the COCO mask evaluation (``COCOeval.evaluateImg``; the reference carries the same body as
    ``evaluateVid`` in mask2former_video/data_video/datasets/ytvis_api/ytvoseval.py:267-345) on the device, and its ``accumulate`` /
    ``summarize`` (:347-525) on the host.  ``update`` counts the pair intersections of packed masks (``mpf_seg_mask_pairs``) and runs
    the greedy matching for every (category, area range, IoU threshold) (``mpf_seg_ap_match``); it launches and returns.  One record
    per detection accumulates in a device buffer; only ``stats`` copies to the host.  IoUs are correctly rounded float64 quotients of
    integer counts and the thresholds are uploaded as the host computed them, so the records are the reference's
    dtMatches / dtIgnore / gtIgnore bit for bit.

    crowd_rule: "coco" = pycocotools' rleIou (a crowd ground truth's IoU is inter / detection area); "union" = the reference file's
    own computeIoU (the plain union for every pair).

    iou_type: "segm" = mask AP; "boundary" = Boundary AP as tools/evaluate_coco_boundary_ap.py computes it with boundary-iou-api: a
    pair's IoU is min(mask IoU, IoU of the two masks' boundaries), the boundaries ``mask_boundaries`` with ``dilation_ratio``;
    area ranges, matching, accumulate and summarize are the same.  "bbox" = COCO's box AP: a pair's IoU is pycocotools' ``bbIou`` of
    two XYWH float64 boxes (``mpf_seg_ap_match_box``, every operation rounded on its own: an IEEE double restatement gives the same
    bits), the boxes given to ``update`` or derived from the masks with ``mask_boxes``; an unmatched detection's area is w * h.

    tubes: the YouTube-VIS form of the same file (``TubeAP``): a "mask" is a tube int64 [F, nwords], the packed words of its frames,
    an image a video.  The IoU is ``iou_seq`` (:203-217): the frames' words concatenated, a frame without annotation all-zero words.
    The area ranges test ``avg_area`` (:100-104, :283, :330), the mean of a tube's non-zero frame areas
    (``mpf_seg_tube_areas``), on both sides, through ``mpf_seg_ap_match_tube``.  The defaults become crowd_rule "union" (what the
    reference file computes) and ``YTVIS_AREA_RNGS``; ``results`` adds AR1 and AR10.  Boundary IoU has no tube form.

    Deviation: with ``gt_areas=None`` a ground truth's area is its pixel count (COCO reads the annotation's "area")."""

    def __init__(self, num_classes, iou_thrs=None, area_rngs=None, max_dets=(1, 10, 100), crowd_rule=None, device="cuda:0",
                 iou_type="segm", dilation_ratio=0.02, tubes=False):
        if iou_type not in AP_IOU_TYPES:
            raise ValueError(f"iou_type must be 'segm', 'boundary' or 'bbox', got {iou_type!r}")
        self.tubes = bool(tubes)
        if self.tubes and iou_type != "segm":
            raise ValueError("tubes=True evaluates mask tubes: iou_type must be 'segm'")
        if crowd_rule is None:
            crowd_rule = "union" if self.tubes else "coco"
        if area_rngs is None:
            area_rngs = YTVIS_AREA_RNGS if self.tubes else COCO_AREA_RNGS
        self.iou_type = iou_type
        self.dilation_ratio = float(dilation_ratio)
        self.num_classes = int(num_classes)
        if self.num_classes <= 0:
            raise ValueError("num_classes must be positive")
        self.iou_thrs = np.linspace(.5, 0.95, 10) if iou_thrs is None else np.array(iou_thrs, dtype=np.float64)
        self.area_rngs = np.array(area_rngs, dtype=np.float64)
        self.rec_thrs = np.linspace(.0, 1.00, 101)
        if self.iou_thrs.ndim != 1 or self.iou_thrs.size == 0:
            raise ValueError("iou_thrs must be a non-empty list of thresholds")
        if self.area_rngs.ndim != 2 or self.area_rngs.shape[1] != 2 or self.area_rngs.shape[0] == 0:
            raise ValueError("area_rngs must be [A, 2] (low, high) pairs")
        if self.area_rngs.shape[0] * self.iou_thrs.size > 64:
            raise ValueError(f"{self.area_rngs.shape[0]} area ranges x {self.iou_thrs.size} thresholds do not fit the 64 bits of a record")
        self.max_dets = tuple(sorted(int(m) for m in max_dets))        # evaluate() sorts them (:148)
        if not self.max_dets or self.max_dets[0] <= 0:
            raise ValueError("max_dets must be a non-empty list of positive counts")
        if crowd_rule not in AP_CROWD_RULES:
            raise ValueError(f"crowd_rule must be 'coco' or 'union', got {crowd_rule!r}")
        self.crowd_rule = crowd_rule
        self.device = torch.device(device)
        self._rec = self._npig = self._settings = None
        self._n = self._images = 0

    # ---- device side ----
    def _buffers(self):
        if self._npig is None:
            if self.device.type != "cuda":
                raise RuntimeError("InstanceAP: Not implemented on the CPU (device tensors only)")
            self._npig = torch.zeros(self.num_classes * self.area_rngs.shape[0], dtype=torch.int64, device=self.device)
            self._rec = torch.empty((256, _AP_REC), dtype=torch.int64, device=self.device)
            # the float64 values as the host holds them: a kernel that rebuilt 0.5 + 0.05 i would differ in the last bit
            self._settings = torch.from_numpy(np.concatenate([self.iou_thrs, self.area_rngs.reshape(-1)])).to(self.device)

    def reset(self):
        self._n = self._images = 0
        if self._npig is not None:
            self._npig.zero_()

    def _small(self, v, n, dtype, what):
        from . import _h2d
        if torch.is_tensor(v) and v.is_cuda:
            t = v.to(device=self.device, dtype=dtype)
        elif len(v) == 0:
            t = torch.empty(0, dtype=dtype, device=self.device)
        else:
            t = _h2d.upload(v, self.device, dtype)          # host data goes up without stalling the launch thread
        t = t.reshape(-1).contiguous()
        if t.numel() != n:
            raise ValueError(f"{what} has {t.numel()} entries for {n} masks")
        return t

    def update(self, dt_bits, scores, classes, gt_bits, gt_classes, gt_crowd, gt_areas=None, size=None, pair_counts=None,
               dt_frame_area=None, gt_frame_area=None, dt_boxes=None, gt_boxes=None):
        """One image.  dt_bits int64 [D, nwords] and gt_bits int64 [G, nwords] packed masks on the device (``instance_bits`` /
        ``pack_masks``), scores [D], classes [D], gt_classes [G], gt_crowd [G] (0 / 1), gt_areas [G] or None (= the pixel counts).
        The detections may come in any order: they are sorted by score, descending and stable (the reference's mergesort of -score).
        size: (H, W) of the image, required with iou_type="boundary" (the words alone do not tell H from W).
        pair_counts: what ``mask_pair_counts(dt_bits, gt_bits)`` returned for these masks, where the caller has it already.
        tubes: one video.  dt_bits int64 [D, F, nwords] (``postprocess_video``, "bits" form) and gt_bits int64 [G, F, nwords]
        (``pack_masks`` of the frames; a frame without annotation all zero); dt_frame_area int32 [D, F] / gt_frame_area int32 [G, F]
        where the caller has them (``postprocess_video`` returns the detections'), else counted here; gt_areas [G] replaces the ground
        truths' avg_area.
        iou_type="bbox": dt_boxes [D, 4] / gt_boxes [G, 4], XYWH float64 as a COCO json holds them (host or device).  A side given as
        None is derived on the device from its bits (``boxes_xyxy_to_xywh(mask_boxes(bits, size))``; size is then required); a side
        whose boxes are given may pass its bits as None.  gt_areas None: the pixel counts where gt_bits is given, else w * h.
        No device-to-host copy."""
        if self.device.type != "cuda":
            raise RuntimeError("InstanceAP: Not implemented on the CPU (device tensors only)")
        if self.iou_type == "bbox":
            if dt_frame_area is not None or gt_frame_area is not None:
                raise ValueError("InstanceAP.update: frame areas belong to tubes=True")
            return self._update_bbox(dt_bits, scores, classes, gt_bits, gt_classes, gt_crowd, gt_areas, size, dt_boxes, gt_boxes)
        if dt_boxes is not None or gt_boxes is not None:
            raise ValueError("InstanceAP.update: boxes belong to iou_type='bbox'")
        if self.tubes:
            dt_tubes, gt_tubes = _tubes_arg(dt_bits, "dt_bits"), _tubes_arg(gt_bits, "gt_bits")
            if dt_tubes.shape[0] and gt_tubes.shape[0] and dt_tubes.shape[1:] != gt_tubes.shape[1:]:
                raise ValueError(f"detections are tubes of {tuple(dt_tubes.shape[1:])} (frames, words), ground truths of "
                                 f"{tuple(gt_tubes.shape[1:])}: not one video")
            dt_bits, gt_bits = dt_tubes.flatten(1), gt_tubes.flatten(1)
        elif dt_frame_area is not None or gt_frame_area is not None:
            raise ValueError("InstanceAP.update: frame areas belong to tubes=True")
        dt_bits, gt_bits = _bits_arg(dt_bits, "dt_bits"), _bits_arg(gt_bits, "gt_bits")
        if dt_bits.device != self.device or gt_bits.device != self.device:
            raise RuntimeError(f"masks on {dt_bits.device} / {gt_bits.device}, the records on {self.device}")
        D, G = dt_bits.shape[0], gt_bits.shape[0]
        if D and G and dt_bits.shape[1] != gt_bits.shape[1]:
            raise ValueError(f"detections have {dt_bits.shape[1]} words per mask, ground truths {gt_bits.shape[1]}: not one image")
        boundary = self.iou_type == "boundary"
        if boundary:
            if size is None:
                raise ValueError("InstanceAP.update: iou_type='boundary' needs size=(H, W)")
            H, W = _bits_size(dt_bits if D else gt_bits, size, "InstanceAP.update")
        if pair_counts is not None:
            inter, area_d, area_g = pair_counts
            if tuple(inter.shape) != (D, G) or area_d.numel() != D or area_g.numel() != G or inter.dtype != torch.int32:
                raise ValueError(f"pair_counts are not the int32 counts of {D} x {G} masks")
        self._buffers()
        scores = self._small(scores, D, torch.float32, "scores")
        classes = self._small(classes, D, torch.int32, "classes")
        gt_cat = self._small(gt_classes, G, torch.int32, "gt_classes")
        crowd = self._small(gt_crowd, G, torch.int32, "gt_crowd")
        image = self._images
        self._images += 1
        if D == 0 and G == 0:
            return
        nwords = dt_bits.shape[1] if D else gt_bits.shape[1]
        if not D:
            dt_bits = dt_bits.new_empty((0, nwords))
        if not G:
            gt_bits = gt_bits.new_empty((0, nwords))
        inter, area_d, area_g = mask_pair_counts(dt_bits, gt_bits) if pair_counts is None else pair_counts
        scores, order = scores.sort(descending=True, stable=True)
        classes, area_d, inter = classes[order].contiguous(), area_d[order].contiguous(), inter[order].contiguous()
        if boundary:
            d = boundary_dilation(H, W, self.dilation_ratio)
            inter_b, area_db, area_gb = mask_pair_counts(mask_boundaries(dt_bits, (H, W), d=d), mask_boundaries(gt_bits, (H, W), d=d))
            area_db, inter_b = area_db[order].contiguous(), inter_b[order].contiguous()
        if self.tubes:
            dt_area = tube_avg_areas(tube_frame_areas(dt_tubes) if dt_frame_area is None else dt_frame_area, D)[order].contiguous()
            tube_gt_area = tube_avg_areas(tube_frame_areas(gt_tubes) if gt_frame_area is None else gt_frame_area, G)
        else:
            tube_gt_area = None
        own_area = area_g.double() if tube_gt_area is None else tube_gt_area
        gt_area = own_area if gt_areas is None else self._small(gt_areas, G, torch.float64, "gt_areas")
        counts = (_lib.ptr(inter) if D and G else None, area_d.data_ptr() if D else None, area_g.data_ptr() if G else None)
        if boundary:
            counts += (_lib.ptr(inter_b) if D and G else None, area_db.data_ptr() if D else None, area_gb.data_ptr() if G else None)
        entry = "mpf_seg_ap_match_tube" if self.tubes else "mpf_seg_ap_match_boundary" if boundary else "mpf_seg_ap_match"
        areas = (gt_area.data_ptr() if G else None,) + ((dt_area.data_ptr() if D else None,) if self.tubes else ())
        self._match(entry, counts, D, G, scores, classes, gt_cat, crowd, areas, image)

    def _match(self, entry, source, D, G, scores, classes, gt_cat, crowd, areas, image):
        """The launch every IoU type ends in: ``source`` = the leading pointers of ``entry`` (counts or boxes), ``areas`` = gt_area
        (and the tubes' dt_area); the detections in score order.  The records of the D detections are appended."""
        dev = self.device
        if self._n + D > self._rec.shape[0]:                # grow by doubling; the old buffer stays valid for the queued launches
            grown = torch.empty((max(2 * self._rec.shape[0], self._n + D), _AP_REC), dtype=torch.int64, device=dev)
            grown[:self._n] = self._rec[:self._n]
            self._rec = grown
        stream = _lib.stream_ptr(dev)
        Tn, A = self.iou_thrs.size, self.area_rngs.shape[0]
        ws = _lib.scratch("seg_ap.gt_marks", dev, stream, max(1, _lib.lib().mpf_seg_ap_workspace_bytes(G, A, Tn)))
        sp = self._settings.data_ptr()
        _lib.call(entry, dev, *source,
                  D, G, scores.data_ptr() if D else None, classes.data_ptr() if D else None,
                  gt_cat.data_ptr() if G else None, crowd.data_ptr() if G else None, *areas, sp, Tn, sp + 8 * Tn,
                  A, self.num_classes, self.max_dets[-1], AP_CROWD_RULES[self.crowd_rule], image,
                  self._rec.data_ptr() + 8 * _AP_REC * self._n, self._npig.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        self._n += D

    def _update_bbox(self, dt_bits, scores, classes, gt_bits, gt_classes, gt_crowd, gt_areas, size, dt_boxes, gt_boxes):
        """``update`` of iou_type="bbox": a side's boxes are those given (XYWH) or ``mask_boxes`` of its bits"""
        dev = self.device

        def checked(bits, boxes, what):                     # -> (bits, how many), before anything is uploaded or launched
            if bits is not None:
                bits = _bits_arg(bits, f"{what}_bits")
                if bits.device != dev:
                    raise RuntimeError(f"{what}_bits on {bits.device}, the records on {dev}")
            if boxes is None:
                if bits is None:
                    raise ValueError(f"InstanceAP.update: iou_type='bbox' needs {what}_boxes or {what}_bits")
                if size is None:
                    raise ValueError(f"InstanceAP.update: iou_type='bbox' derives {what}_boxes from the bits and needs size=(H, W)")
                _bits_size(bits, size, "InstanceAP.update")
                return bits, bits.shape[0]
            if bits is not None and bits.shape[0] != len(boxes):
                raise ValueError(f"{len(boxes)} {what}_boxes for {bits.shape[0]} masks")
            return bits, len(boxes)

        def xywh(bits, boxes, n, what):
            if boxes is None:
                return boxes_xyxy_to_xywh(mask_boxes(bits, size))
            return self._small(boxes, 4 * n, torch.float64, f"{what}_boxes").view(n, 4)
        (dt_bits, D), (gt_bits, G) = checked(dt_bits, dt_boxes, "dt"), checked(gt_bits, gt_boxes, "gt")
        dt_box, gt_box = xywh(dt_bits, dt_boxes, D, "dt"), xywh(gt_bits, gt_boxes, G, "gt")
        self._buffers()
        scores = self._small(scores, D, torch.float32, "scores")
        classes = self._small(classes, D, torch.int32, "classes")
        gt_cat = self._small(gt_classes, G, torch.int32, "gt_classes")
        crowd = self._small(gt_crowd, G, torch.int32, "gt_crowd")
        if gt_areas is not None:
            gt_area = self._small(gt_areas, G, torch.float64, "gt_areas")
        elif gt_bits is not None:                           # as "segm": the pixel counts
            gt_area = mask_pair_counts(gt_bits, gt_bits.new_empty((0, gt_bits.shape[1])))[1].double() if G else gt_box.new_empty(0)
        else:
            gt_area = (gt_box[:, 2] * gt_box[:, 3]).contiguous()
        image = self._images
        self._images += 1
        if D == 0 and G == 0:
            return
        scores, order = scores.sort(descending=True, stable=True)
        classes, dt_box = classes[order].contiguous(), dt_box[order].contiguous()
        self._match("mpf_seg_ap_match_box", (dt_box.data_ptr() if D else None, gt_box.data_ptr() if G else None), D, G, scores, classes,
                    gt_cat, crowd, (gt_area.data_ptr() if G else None,), image)

    # ---- host side ----
    def stats(self):
        """-> for the N recorded detections, in update order and score order inside an image: "scores" float32 [N], "category",
        "rank" (inside its image and category), "image" int64 [N], "matched" and "ignored" bool [N, A, Tn], and "npig" int64 [K, A]
        (the non-ignored ground truths).  One device-to-host copy."""
        K, A, Tn, n = self.num_classes, self.area_rngs.shape[0], self.iou_thrs.size, self._n
        if self._npig is None:
            host = np.zeros(K * A, dtype=np.int64)
        else:
            host = torch.cat([self._rec[:n].reshape(-1), self._npig]).cpu().numpy()
        rec = host[:_AP_REC * n].reshape(n, _AP_REC).view(np.uint64)
        shifts = np.arange(A * Tn, dtype=np.uint64)
        unpack = lambda w: ((w[:, None] >> shifts[None, :]) & np.uint64(1)).astype(bool).reshape(n, A, Tn)      # noqa: E731
        return {"scores": (rec[:, 0] & np.uint64(0xffffffff)).astype(np.uint32).view(np.float32),
                "category": (rec[:, 0] >> np.uint64(32)).astype(np.int64), "rank": (rec[:, 1] & np.uint64(0xffffffff)).astype(np.int64),
                "image": (rec[:, 1] >> np.uint64(32)).astype(np.int64), "matched": unpack(rec[:, 2]), "ignored": unpack(rec[:, 3]),
                "npig": host[_AP_REC * n:].reshape(K, A).copy()}

    @staticmethod
    def combine(list_of_stats):
        """Ranks or shards: the records concatenated in list order, npig summed."""
        if not list_of_stats:
            raise ValueError("combine: no stats")
        keys = ("scores", "category", "rank", "image", "matched", "ignored")
        out = {k: np.concatenate([np.asarray(s[k]) for s in list_of_stats]) for k in keys}
        out["npig"] = np.sum([np.asarray(s["npig"], dtype=np.int64) for s in list_of_stats], axis=0)
        return out

    def accumulate(self, stats=None):
        """``accumulate`` of the reference (:385-442) from the records -> {"precision" [Tn, R, K, A, M], "recall" [Tn, K, A, M],
        "scores" [Tn, R, K, A, M]} float64, -1 where a (category, range) has no non-ignored ground truth; R = the 101 recall points."""
        s = self.stats() if stats is None else stats
        return ap_accumulate(s, self.num_classes, self.iou_thrs, self.rec_thrs, self.area_rngs.shape[0], self.max_dets)

    def summarize(self, stats=None):
        """The 12 statistics of the reference's ``_summarizeDets`` (:490-504)."""
        return ap_summarize(self.accumulate(stats), self.iou_thrs, self.max_dets)

    def results(self, class_names=None, stats=None):
        """detectron2's ``COCOEvaluator`` keys for "segm": AP, AP50, AP75, APs, APm, APl (x 100, nan where the statistic is -1) and
        one AP-{name} per category (names default to the class index).  tubes: AR1 and AR10 too, statistics 6 and 7
        (``YTVISEvaluator._derive_coco_results``, mask2former_video/data_video/ytvis_eval.py:205)."""
        K = self.num_classes
        if class_names is not None and len(class_names) != K:
            raise ValueError(f"{len(class_names)} class names for {K} classes")
        acc = self.accumulate(stats)
        st = ap_summarize(acc, self.iou_thrs, self.max_dets)
        metrics = ("AP", "AP50", "AP75", "APs", "APm", "APl") + (("AR1", "AR10") if self.tubes else ())     # ytvis_eval.py:205
        out = {name: float(st[i] * 100 if st[i] >= 0 else "nan") for i, name in enumerate(metrics)}
        names = [str(i) for i in range(K)] if class_names is None else list(class_names)
        for k, name in enumerate(names):
            p = acc["precision"][:, :, k, 0, -1]
            p = p[p > -1]
            out[f"AP-{name}"] = float(np.mean(p) * 100) if p.size else float("nan")
        return out


class TubeAP(InstanceAP):
    """``InstanceAP(..., tubes=True)``: the YouTube-VIS evaluation of the reference (``YTVOSeval``) on packed mask tubes."""

    def __init__(self, num_classes, **options):
        super().__init__(num_classes, tubes=True, **options)


def _tubes_arg(bits, what):
    if not bits.is_cuda:
        raise RuntimeError(f"{what}: Not implemented on the CPU (device tensors only)")
    if bits.dim() != 3 or bits.dtype != torch.int64:
        raise ValueError(f"{what} must be packed tubes int64 [M, F, nwords], got {bits.dtype} {tuple(bits.shape)}")
    return bits.contiguous()


def tube_frame_areas(tubes):
    """Packed tubes int64 [M, F, nwords] -> their per-frame areas int32 [M, F]: ``mask_pair_counts`` on the M * F frame rows with the
    other side empty (one launch)."""
    tubes = _tubes_arg(tubes, "tubes")
    M, F, nwords = tubes.shape
    if M * F == 0:
        return torch.zeros((M, F), dtype=torch.int32, device=tubes.device)
    return mask_pair_counts(tubes.view(M * F, nwords), tubes.new_empty((0, nwords)))[1].view(M, F)


def tube_avg_areas(frame_area, M=None):
    """``avg_area`` of the reference's ``_toMask`` (ytvoseval.py:100-104) from frame areas int32 [M, F] on the device: the float64
    mean over the frames with a non-zero area, 0.0 without one."""
    if not frame_area.is_cuda:
        raise RuntimeError("tube_avg_areas: Not implemented on the CPU (device tensors only)")
    if frame_area.dim() != 2 or frame_area.dtype != torch.int32 or (M is not None and frame_area.shape[0] != M):
        raise ValueError(f"frame areas must be int32 [{'M' if M is None else M}, F], got {frame_area.dtype} {tuple(frame_area.shape)}")
    frame_area = frame_area.contiguous()
    dev = frame_area.device
    out = torch.empty(frame_area.shape[0], dtype=torch.float64, device=dev)
    if frame_area.shape[0]:
        _lib.call("mpf_seg_tube_areas", dev, frame_area.data_ptr(), frame_area.shape[0], frame_area.shape[1], out.data_ptr(),
                  _lib.stream_ptr(dev))
    return out


def ap_accumulate(stats, K, iou_thrs, rec_thrs, A, max_dets):
    """The reference's ``accumulate`` (ytvoseval.py:385-442) from detection records (``InstanceAP.stats``).  The records of a category
    in their stored order are the reference's concatenation of the images' evalImgs (image order, score order inside an image)."""
    Tn, R, M = len(iou_thrs), len(rec_thrs), len(max_dets)
    precision = -np.ones((Tn, R, K, A, M))
    recall = -np.ones((Tn, K, A, M))
    scores = -np.ones((Tn, R, K, A, M))
    cat, rank = np.asarray(stats["category"]), np.asarray(stats["rank"])
    sc = np.asarray(stats["scores"], dtype=np.float32).astype(np.float64)
    matched, ignored, npig_all = np.asarray(stats["matched"]), np.asarray(stats["ignored"]), np.asarray(stats["npig"])
    if npig_all.shape != (K, A) or matched.shape[1:] != (A, Tn) or ignored.shape != matched.shape:
        raise ValueError(f"stats do not fit {K} classes, {A} ranges, {Tn} thresholds")
    for k in range(K):
        of_k = cat == k
        for a in range(A):
            npig = int(npig_all[k, a])
            if npig == 0:
                continue
            for m, max_det in enumerate(max_dets):
                sel = np.nonzero(of_k & (rank < max_det))[0]
                dt_scores = sc[sel]
                inds = np.argsort(-dt_scores, kind="mergesort")
                dt_sorted = dt_scores[inds]
                dtm = matched[sel, a, :].T[:, inds]
                dt_ig = ignored[sel, a, :].T[:, inds]
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,)).tolist()
                    ss = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    pos = np.searchsorted(rc, rec_thrs, side="left")
                    for ri, pi in enumerate(pos):
                        if pi >= nd:                     # the reference's loop ends here in an IndexError: the rest stays 0
                            break
                        q[ri] = pr[pi]
                        ss[ri] = dt_sorted[pi]
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    return {"precision": precision, "recall": recall, "scores": scores}


def ap_summarize(acc, iou_thrs, max_dets):
    """The reference's ``_summarizeDets`` (ytvoseval.py:459-504) -> float64 [12].  As there, the area ranges are all / small / medium /
    large in that order, and the first statistic asks for ``maxDets == 100``: it is -1 where max_dets does not list 100."""
    precision, recall = acc["precision"], acc["recall"]
    iou_thrs = np.asarray(iou_thrs)
    if precision.shape[3] != 4 or len(max_dets) < 3:
        raise ValueError("the 12 statistics need the four area ranges (all, small, medium, large) and three max_dets")

    def one(ap=1, iou_thr=None, area=0, max_det=100):
        aind = [area]
        mind = [i for i, m in enumerate(max_dets) if m == max_det]
        s = precision if ap == 1 else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == iou_thrs)[0]]
        s = s[:, :, :, aind, mind] if ap == 1 else s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    st = np.zeros((12,))
    st[0] = one(1)
    st[1] = one(1, iou_thr=.5, max_det=max_dets[2])
    st[2] = one(1, iou_thr=.75, max_det=max_dets[2])
    st[3] = one(1, area=1, max_det=max_dets[2])
    st[4] = one(1, area=2, max_det=max_dets[2])
    st[5] = one(1, area=3, max_det=max_dets[2])
    st[6] = one(0, max_det=max_dets[0])
    st[7] = one(0, max_det=max_dets[1])
    st[8] = one(0, max_det=max_dets[2])
    st[9] = one(0, area=1, max_det=max_dets[2])
    st[10] = one(0, area=2, max_det=max_dets[2])
    st[11] = one(0, area=3, max_det=max_dets[2])
    return st
