"""Restatements of the reference's video eval branch, for the tests of csrc/seg_video.hip and the tube form of InstanceAP.

* ``inference_video``: torch restatement of ``VideoMaskFormer.forward``'s else branch and ``inference_video``
  (mask2former_video/video_maskformer_model.py:204-287): upsample every query to the padded size, select the top entries, crop,
  resize, threshold.  Entries come out sorted by score, descending and stable (the reference's ``topk(sorted=False)`` order is
  unspecified).  ``dtype`` float64 gives the margin reference of the tie band.
* ``avg_area`` / ``tube_iou``: numpy restatements of ``_toMask``'s avg_area (ytvoseval.py:100-104) and ``iou_seq`` (:203-217).
* ``tube_items`` / ``evaluate_tubes``: a tube as the items tests/_ap_restate.py takes, its frames stacked (a frame without annotation
  all zero) and its area the avg_area, so that ``evaluateVid`` / ``accumulate`` / ``summarize`` are the restatements there.
tests/test_video_cpu.py holds all of it to the goldens the reference's own code produced (tests/golden/make_golden_v*.py).

A tube is a dict {"id", "category", "frames": list of dense bool [H, W] or None, + "score" | "iscrowd"}."""
import numpy as np
import torch
import torch.nn.functional as F

import _ap_restate as A

YTVIS_AREA_RNGS = [[0 ** 2, 1e5 ** 2], [0 ** 2, 128 ** 2], [128 ** 2, 256 ** 2], [256 ** 2, 1e5 ** 2]]


def inference_video(pred_cls, pred_masks, img_size, padded_hw, height, width, topk=10, dtype=torch.float32):
    """pred_cls [Q, K+1], pred_masks [Q, F, h, w] -> {"scores" fp32 [T], "labels", "query" int64 [T], "masks" bool [T, F, H, W],
    "logits" [T, F, H, W] in ``dtype``: the resampled logits the threshold reads}"""
    K = pred_cls.shape[1] - 1
    if len(pred_cls) == 0:
        e = torch.zeros(0, dtype=torch.int64)
        z = torch.zeros((0, pred_masks.shape[1], height, width))
        return {"scores": torch.zeros(0), "labels": e, "query": e, "masks": z.bool(), "logits": z.to(dtype)}
    up = F.interpolate(pred_masks.to(dtype), size=(int(padded_hw[0]), int(padded_hw[1])), mode="bilinear", align_corners=False)
    scores = F.softmax(pred_cls.float(), dim=-1)[:, :-1]
    sc, idx = scores.flatten(0, 1).topk(min(topk, scores.numel()), sorted=True)
    sc, order = sc.sort(descending=True, stable=True)
    idx = idx[order]
    labels, query = idx % K, idx // K
    m = up[query][:, :, : img_size[0], : img_size[1]]
    m = F.interpolate(m, size=(height, width), mode="bilinear", align_corners=False)
    return {"scores": sc, "labels": labels, "query": query, "masks": m > 0., "logits": m}


def rle_counts(mask):
    """uncompressed COCO run lengths of a dense [H, W] mask: column-major, starting with the (possibly empty) run of zeros"""
    flat = np.asarray(mask).astype(bool).T.reshape(-1)
    edges = np.flatnonzero(np.diff(np.concatenate([[False], flat]).astype(np.int8)) != 0)
    return np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()


def rle_decode(rle):
    H, W = rle["size"]
    flat = np.zeros(H * W, dtype=bool)
    p, v = 0, False
    for c in rle["counts"]:
        flat[p:p + c] = v
        p += c
        v = not v
    assert p == H * W
    return flat.reshape(W, H).T


# ---- tubes ---------------------------------------------------------------------------------------------------------------------------
def frame_areas(frames):
    """what YTVOS.loadRes / the annotation carry as "areas": the pixel count per frame, None where the frame has no mask"""
    return [None if m is None else int(np.count_nonzero(m)) for m in frames]


def avg_area(areas):
    l = [a for a in areas if a]
    return 0 if len(l) == 0 else np.array(l).mean()


def tube_iou(d_seq, g_seq):
    i = .0
    u = .0
    for d, g in zip(d_seq, g_seq):
        if d is not None and g is not None:
            i += float(np.count_nonzero(d & g))
            u += float(np.count_nonzero(d | g))
        elif d is None and g is not None:
            u += float(np.count_nonzero(g))
        elif d is not None and g is None:
            u += float(np.count_nonzero(d))
    return i / u if u > .0 else .0


def stack_frames(frames, H, W):
    """dense bool [F, H, W], a frame without a mask all zero"""
    return np.stack([np.zeros((H, W), dtype=bool) if m is None else np.asarray(m, dtype=bool) for m in frames])


def tube_items(tubes, H, W):
    out = []
    for t in tubes:
        item = {k: v for k, v in t.items() if k != "frames"}
        item["mask"] = stack_frames(t["frames"], H, W)
        item["area"] = avg_area(frame_areas(t["frames"]))
        out.append(item)
    return out


def evaluate_tubes(videos, K, area_rngs, max_dets, iou_thrs=A.IOU_THRS):
    """videos: list of (dts, gts, (H, W)) of tubes -> evalImgs in the reference's (category, range, video) order; the reference
    file's own IoU takes the plain union for every pair (crowd_rule "union")"""
    return A.evaluate(video_items(videos), K, area_rngs, max_dets, iou_thrs, crowd_rule="union")


def video_items(videos):
    return [(tube_items(dts, *hw), tube_items(gts, *hw)) for dts, gts, hw in videos]
