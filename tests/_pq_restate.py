"""Numpy restatement of panopticapi's per-image PQ arithmetic (``pq_compute_single_core``; the reference carries the body as
``pq_compute_single_image``, tools/evaluate_pq_for_semantic_segmentation.py:41-136) for listed segments, crowd regions and VOID on
either side — the expected values of tests/test_pq_gpu.py and the parent side of ``tools/bench_infer.py --rows pq``.

It keeps the reference's own steps and their order (``np.unique`` of gt * OFFSET + pred, one walk over the pairs in ascending
order, python floats), so per-category ``iou`` comes out in the reference's bits.  Two things differ from panopticapi, as in the
device path: a gt segment's area is its pixel count, and the cases where the reference raises ``KeyError`` raise ``ValueError``.
"""
import numpy as np

OFFSET = 256 * 256 * 256


def rgb2id(rgb):
    rgb = np.asarray(rgb).astype(np.int64)
    return rgb[..., 0] + 256 * rgb[..., 1] + 256 * 256 * rgb[..., 2]


def id2rgb(ids):
    ids = np.asarray(ids).astype(np.int64)
    return np.stack([ids % 256, ids // 256 % 256, ids // 65536 % 256], axis=-1).astype(np.uint8)


def zero_stats(K):
    return {"tp": np.zeros(K, np.int64), "fp": np.zeros(K, np.int64), "fn": np.zeros(K, np.int64), "iou": np.zeros(K, np.float64)}


def pq_single(pan_gt, pan_pred, gt_segments, pred_segments, K, void_id=0):
    """One image -> {"tp", "fp", "fn"} int64 [K], "iou" float64 [K].  gt_segments: [{"id", "category_id", "iscrowd"}] in the
    annotation's order; pred_segments: [{"id", "category_id"}]."""
    pan_gt = np.asarray(pan_gt).astype(np.int64)
    pan_pred = np.asarray(pan_pred).astype(np.int64)
    st = zero_stats(K)
    iou_sum = [0.0] * K                                   # python floats, as PQStatCat.iou
    gt_segms = {int(s["id"]): {"category_id": int(s["category_id"]), "iscrowd": int(s.get("iscrowd", 0)), "area": 0} for s in gt_segments}
    pred_segms = {int(s["id"]): {"category_id": int(s["category_id"]), "area": 0} for s in pred_segments}
    for label, cnt in zip(*np.unique(pan_gt, return_counts=True)):
        if int(label) in gt_segms:
            gt_segms[int(label)]["area"] = int(cnt)
    left = set(pred_segms)
    for label, cnt in zip(*np.unique(pan_pred, return_counts=True)):
        label = int(label)
        if label not in pred_segms:
            if label == void_id:
                continue
            raise ValueError(f"segment {label} is in the map and not in segments_info")
        pred_segms[label]["area"] = int(cnt)
        left.remove(label)
        if not 0 <= pred_segms[label]["category_id"] < K:
            raise ValueError(f"segment {label} has an unknown category")
    if left:
        raise ValueError(f"segments {sorted(left)} are in segments_info and not in the map")

    gt_pred_map = {}
    labels, labels_cnt = np.unique(pan_gt.astype(np.uint64) * np.uint64(OFFSET) + pan_pred.astype(np.uint64), return_counts=True)
    for label, inter in zip(labels, labels_cnt):
        gt_pred_map[(int(label) // OFFSET, int(label) % OFFSET)] = int(inter)

    gt_matched, pred_matched = set(), set()
    for (g, p), inter in gt_pred_map.items():
        if g not in gt_segms or p not in pred_segms:
            continue
        if gt_segms[g]["iscrowd"] == 1:
            continue
        if gt_segms[g]["category_id"] != pred_segms[p]["category_id"]:
            continue
        union = pred_segms[p]["area"] + gt_segms[g]["area"] - inter - gt_pred_map.get((void_id, p), 0)
        iou = inter / union
        if iou > 0.5:
            c = gt_segms[g]["category_id"]
            st["tp"][c] += 1
            iou_sum[c] += iou
            gt_matched.add(g)
            pred_matched.add(p)

    crowd = {}
    for g, info in gt_segms.items():
        if g in gt_matched:
            continue
        if info["iscrowd"] == 1:
            crowd[info["category_id"]] = g
            continue
        st["fn"][info["category_id"]] += 1

    for p, info in pred_segms.items():
        if p in pred_matched:
            continue
        inter = gt_pred_map.get((void_id, p), 0)
        if info["category_id"] in crowd:
            inter += gt_pred_map.get((crowd[info["category_id"]], p), 0)
        if inter / info["area"] > 0.5:
            continue
        st["fp"][info["category_id"]] += 1
    st["iou"] = np.array(iou_sum, dtype=np.float64)
    return st


def pq_single_semantic(gt, pred, K, ignore_label):
    """The reference tool's own form (:49-60): every class with a pixel is one segment of its side."""
    gt = np.asarray(gt).astype(np.int64)
    pred = np.asarray(pred).astype(np.int64)
    bad = [int(v) for v in np.unique(pred) if not 0 <= v < K]
    if bad:
        raise ValueError(f"predicted labels {bad} are no category")
    gts = [{"id": int(c), "category_id": int(c), "iscrowd": 0} for c in np.unique(gt) if c != ignore_label and 0 <= c < K]
    preds = [{"id": int(c), "category_id": int(c)} for c in np.unique(pred)]
    return pq_single(gt, pred, gts, preds, K, void_id=ignore_label)


def add_stats(total, single):
    """pq_stat += single"""
    return {k: total[k] + single[k] for k in ("tp", "fp", "fn", "iou")}
