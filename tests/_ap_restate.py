"""Numpy restatement of the COCO mask evaluation as the reference carries it in
mask2former_video/data_video/datasets/ytvis_api/ytvoseval.py (an image is a one-frame video): ``compute_iou`` (:176-222, and
pycocotools' rleIou crowd rule), ``evaluate_image`` (evaluateVid, :267-345), ``accumulate`` (:347-442) and ``summarize`` (:454-504),
in the reference's loop form.  tests/test_ap_cpu.py holds it to the golden the reference's own code produced
(tests/golden/make_golden_ap.py); the GPU tests hold the device to it.

A detection is a dict {"id", "category", "score", "mask", "area"}, a ground truth {"id", "category", "mask", "area", "iscrowd"};
masks are dense bool [H, W]; ids are positive."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
COCO_AREA_RNGS = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]


def pack_columns(masks):
    """dense [M, H, W] -> uint64 [M, nwords]: position p = x * H + y, bit b of word j = position 64 j + b"""
    masks = np.asarray(masks) != 0
    M, H, W = masks.shape
    nwords = (H * W + 63) // 64
    flat = np.zeros((M, nwords * 64), dtype=np.uint8)
    flat[:, :H * W] = masks.transpose(0, 2, 1).reshape(M, H * W)
    return np.packbits(flat, axis=1, bitorder="little").view("<u8").reshape(M, nwords)


def unpack_columns(words, H, W):
    words = np.ascontiguousarray(words).view(np.uint64)
    M = words.shape[0]
    flat = np.unpackbits(words.astype("<u8").view(np.uint8).reshape(M, -1), axis=1, bitorder="little")
    return flat[:, :H * W].reshape(M, W, H).transpose(0, 2, 1).astype(bool), flat[:, H * W:]


def sort_dets(dt, max_det):
    inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
    return [dt[i] for i in inds[0:max_det]]


def compute_iou(dt, gt, max_det, crowd_rule):
    """ious [D, G] of the score-sorted, truncated detections against the ground truths in their given order"""
    if len(gt) == 0 and len(dt) == 0:
        return []
    dt = sort_dets(dt, max_det)
    ious = np.zeros([len(dt), len(gt)])
    for i, j in np.ndindex(ious.shape):
        d, g = dt[i]["mask"], gt[j]["mask"]
        inter = float(np.count_nonzero(d & g))
        if crowd_rule == "union":                       # ytvoseval.py:203-217
            u = float(np.count_nonzero(d | g))
            ious[i, j] = inter / u if u > .0 else .0
        elif crowd_rule == "coco":                      # pycocotools rleIou: crowd divides by the detection's area
            u = float(np.count_nonzero(d)) if int(gt[j]["iscrowd"]) else float(np.count_nonzero(d | g))
            ious[i, j] = inter / u if inter > 0 else .0
        else:
            raise ValueError(crowd_rule)
    return ious


def evaluate_image(dt, gt, a_rng, max_det, iou_thrs, crowd_rule):
    """one (image, category, area range): the dict of evaluateVid, or None"""
    if len(gt) == 0 and len(dt) == 0:
        return None
    ious_all = compute_iou(dt, gt, max_det, crowd_rule)
    ignore = [1 if (g["iscrowd"] or (g["area"] < a_rng[0] or g["area"] > a_rng[1])) else 0 for g in gt]
    gtind = np.argsort(ignore, kind="mergesort")
    gt = [gt[i] for i in gtind]
    dt = sort_dets(dt, max_det)
    iscrowd = [int(o["iscrowd"]) for o in gt]
    ious = ious_all[:, gtind] if len(ious_all) > 0 else ious_all
    T, G, D = len(iou_thrs), len(gt), len(dt)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    gt_ig = np.array([ignore[i] for i in gtind])
    dt_ig = np.zeros((T, D))
    if not len(ious) == 0:
        for tind, t in enumerate(iou_thrs):
            for dind, d in enumerate(dt):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind, g in enumerate(gt):
                    if gtm[tind, gind] > 0 and not iscrowd[gind]:
                        continue
                    if m > -1 and gt_ig[m] == 0 and gt_ig[gind] == 1:
                        break
                    if ious[dind, gind] < iou:
                        continue
                    iou = ious[dind, gind]
                    m = gind
                if m == -1:
                    continue
                dt_ig[tind, dind] = gt_ig[m]
                dtm[tind, dind] = gt[m]["id"]
                gtm[tind, m] = d["id"]
    a = np.array([d["area"] < a_rng[0] or d["area"] > a_rng[1] for d in dt]).reshape((1, len(dt)))
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm == 0, np.repeat(a, T, 0)))
    return {"dtIds": [d["id"] for d in dt], "gtIds": [g["id"] for g in gt], "dtMatches": dtm, "gtMatches": gtm,
            "dtScores": [d["score"] for d in dt], "gtIgnore": gt_ig, "dtIgnore": dt_ig}


def evaluate(images, K, area_rngs, max_dets, iou_thrs=IOU_THRS, crowd_rule="coco"):
    """images: list of (dts, gts) -> evalImgs in the reference's (category, range, image) order"""
    max_det = sorted(max_dets)[-1]
    return [evaluate_image([d for d in dts if d["category"] == k], [g for g in gts if g["category"] == k], rng, max_det, iou_thrs,
                           crowd_rule)
            for k in range(K) for rng in area_rngs for dts, gts in images]


def accumulate(eval_imgs, K, n_images, area_rngs, max_dets, iou_thrs=IOU_THRS, rec_thrs=REC_THRS):
    max_dets = sorted(max_dets)
    T, R, A, M = len(iou_thrs), len(rec_thrs), len(area_rngs), len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    scores = -np.ones((T, R, K, A, M))
    for k in range(K):
        Nk = k * A * n_images
        for a in range(A):
            Na = a * n_images
            for m, max_det in enumerate(max_dets):
                E = [eval_imgs[Nk + Na + i] for i in range(n_images)]
                E = [e for e in E if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([e["dtScores"][0:max_det] for e in E])
                inds = np.argsort(-dt_scores, kind="mergesort")
                dt_scores_sorted = dt_scores[inds]
                dtm = np.concatenate([e["dtMatches"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dtIgnore"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gtIgnore"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                if npig == 0:
                    continue
                tps = np.logical_and(dtm, np.logical_not(dt_ig))
                fps = np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=float)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=float)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    ss = np.zeros((R,))
                    if nd:
                        recall[t, k, a, m] = rc[-1]
                    else:
                        recall[t, k, a, m] = 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds = np.searchsorted(rc, rec_thrs, side="left")
                    try:
                        for ri, pi in enumerate(inds):
                            q[ri] = pr[pi]
                            ss[ri] = dt_scores_sorted[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
                    scores[t, :, k, a, m] = np.array(ss)
    return {"precision": precision, "recall": recall, "scores": scores}


def summarize(acc, max_dets, iou_thrs=IOU_THRS):
    """_summarizeDets; the area ranges are all / small / medium / large in that order"""
    max_dets = sorted(max_dets)
    labels = ["all", "small", "medium", "large"]

    def _summarize(ap=1, iouThr=None, areaRng="all", maxDets=100):
        aind = [i for i, lbl in enumerate(labels) if lbl == areaRng]
        mind = [i for i, m in enumerate(max_dets) if m == maxDets]
        if ap == 1:
            s = acc["precision"]
            if iouThr is not None:
                s = s[np.where(iouThr == iou_thrs)[0]]
            s = s[:, :, :, aind, mind]
        else:
            s = acc["recall"]
            if iouThr is not None:
                s = s[np.where(iouThr == iou_thrs)[0]]
            s = s[:, :, aind, mind]
        return -1 if len(s[s > -1]) == 0 else np.mean(s[s > -1])
    stats = np.zeros((12,))
    stats[0] = _summarize(1)
    stats[1] = _summarize(1, iouThr=.5, maxDets=max_dets[2])
    stats[2] = _summarize(1, iouThr=.75, maxDets=max_dets[2])
    stats[3] = _summarize(1, areaRng="small", maxDets=max_dets[2])
    stats[4] = _summarize(1, areaRng="medium", maxDets=max_dets[2])
    stats[5] = _summarize(1, areaRng="large", maxDets=max_dets[2])
    stats[6] = _summarize(0, maxDets=max_dets[0])
    stats[7] = _summarize(0, maxDets=max_dets[1])
    stats[8] = _summarize(0, maxDets=max_dets[2])
    stats[9] = _summarize(0, areaRng="small", maxDets=max_dets[2])
    stats[10] = _summarize(0, areaRng="medium", maxDets=max_dets[2])
    stats[11] = _summarize(0, areaRng="large", maxDets=max_dets[2])
    return stats


def expected_stats(images, K, area_rngs, max_dets, iou_thrs=IOU_THRS, crowd_rule="coco", eval_imgs=None):
    """What ``InstanceAP.stats`` must return for these images: one record per detection, images in order, score order (stable)
    inside an image; "rank" counts inside (image, category); a detection beyond the largest max_det has no bits."""
    A, T, n_images = len(area_rngs), len(iou_thrs), len(images)
    if eval_imgs is None:
        eval_imgs = evaluate(images, K, area_rngs, max_dets, iou_thrs, crowd_rule)
    npig = np.zeros((K, A), dtype=np.int64)
    rows = {}
    for k in range(K):
        for a in range(A):
            for i in range(n_images):
                e = eval_imgs[(k * A + a) * n_images + i]
                if e is None:
                    continue
                npig[k, a] += np.count_nonzero(e["gtIgnore"] == 0)
                for r, did in enumerate(e["dtIds"]):
                    row = rows.setdefault((i, did), {"rank": r, "matched": np.zeros((A, T), dtype=bool),
                                                     "ignored": np.zeros((A, T), dtype=bool)})
                    assert row["rank"] == r
                    row["matched"][a] = e["dtMatches"][:, r] != 0
                    row["ignored"][a] = np.asarray(e["dtIgnore"])[:, r].astype(bool)
    out = {k: [] for k in ("scores", "category", "rank", "image", "matched", "ignored")}
    for i, (dts, _) in enumerate(images):
        seen = {}
        for j in np.argsort([-d["score"] for d in dts], kind="mergesort"):
            d = dts[j]
            rank = seen.get(d["category"], 0)
            seen[d["category"]] = rank + 1
            row = rows.get((i, d["id"]))
            assert (row is None) == (rank >= sorted(max_dets)[-1]) and (row is None or row["rank"] == rank)
            out["scores"].append(np.float32(d["score"]))
            out["category"].append(d["category"])
            out["rank"].append(rank)
            out["image"].append(i)
            out["matched"].append(row["matched"] if row else np.zeros((A, T), dtype=bool))
            out["ignored"].append(row["ignored"] if row else np.zeros((A, T), dtype=bool))
    return {"scores": np.asarray(out["scores"], dtype=np.float32), "category": np.asarray(out["category"], dtype=np.int64),
            "rank": np.asarray(out["rank"], dtype=np.int64), "image": np.asarray(out["image"], dtype=np.int64),
            "matched": np.asarray(out["matched"], dtype=bool).reshape(-1, A, T),
            "ignored": np.asarray(out["ignored"], dtype=bool).reshape(-1, A, T), "npig": npig}
