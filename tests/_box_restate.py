"""Numpy restatement of the box side of the COCO evaluation: Detectron2's ``BitMasks.get_bounding_boxes`` (``boxes_of``),
pycocotools' ``bbIou`` (``bb_iou``, maskApi.c, in IEEE double and in its operation order) and ``evaluateImg`` driven by such an IoU
matrix (``evaluate_image``: the loop of tests/_ap_restate.py, whose matcher computes its IoUs from masks and takes no matrix).
``accumulate`` / ``summarize`` / ``expected_stats`` are those of tests/_ap_restate.py.

A detection is a dict {"id", "category", "score", "box", "area"}, a ground truth {"id", "category", "box", "area", "iscrowd"}; boxes
are XYWH floats; a detection's "area" is w * h, what COCO's ``loadRes`` gives a bbox result."""
import numpy as np

import _ap_restate as R


def boxes_of(dense):
    """dense [M, H, W] (non-zero = set) -> int32 [M, 4] (x0, y0, x1, y1): the first and last set column / row, the last + 1; an empty
    mask gives zeros (BitMasks.get_bounding_boxes)"""
    dense = np.asarray(dense) != 0
    out = np.zeros((dense.shape[0], 4), dtype=np.int32)
    for m, mask in enumerate(dense):
        xs, ys = np.nonzero(np.any(mask, axis=0))[0], np.nonzero(np.any(mask, axis=1))[0]
        if len(xs) and len(ys):
            out[m] = (xs[0], ys[0], xs[-1] + 1, ys[-1] + 1)
    return out


def xyxy_to_xywh(boxes):
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    return np.concatenate([b[:, :2], b[:, 2:] - b[:, :2]], axis=1)


def bb_iou(dt, gt, crowd, rule):
    """dt [D, 4], gt [G, 4] XYWH, crowd [G] -> float64 [D, G].  Python floats: every operation is one IEEE double rounding."""
    dt, gt = np.asarray(dt, dtype=np.float64).reshape(-1, 4), np.asarray(gt, dtype=np.float64).reshape(-1, 4)
    if rule not in ("coco", "union"):
        raise ValueError(rule)
    out = np.zeros((len(dt), len(gt)), dtype=np.float64)
    for d in range(len(dt)):
        dx, dy, dw, dh = (float(v) for v in dt[d])
        for g in range(len(gt)):
            gx, gy, gw, gh = (float(v) for v in gt[g])
            w = min(dx + dw, gx + gw) - max(dx, gx)
            h = min(dy + dh, gy + gh) - max(dy, gy)
            if w <= 0 or h <= 0:
                continue
            i = w * h
            da = dw * dh
            if crowd[g] and rule == "coco":
                u = da
            else:
                ga = gw * gh
                u = da + ga
                u = u - i
            out[d, g] = i / u
    return out


def bb_iou_contracted(d, g):
    """What a compiler that contracts a * b + c into a fused multiply-add makes of one non-crowd pair: ``u = fma(-w, h, fma(gw, gh,
    dw * dh))``, the products inside the two FMAs unrounded (exact rational arithmetic, then one rounding), over the same rounded
    ``i = w * h``.  Not the specification: the tests use it to pick thresholds at which such code decides differently."""
    from fractions import Fraction as Fr
    dx, dy, dw, dh = (float(v) for v in d)
    gx, gy, gw, gh = (float(v) for v in g)
    w = min(dx + dw, gx + gw) - max(dx, gx)
    h = min(dy + dh, gy + gh) - max(dy, gy)
    if w <= 0 or h <= 0:
        return 0.0
    i = w * h
    t = float(Fr(gw) * Fr(gh) + Fr(dw * dh))
    u = float(Fr(t) - Fr(w) * Fr(h))
    return i / u


# (detection, ground truth) XYWH pairs whose IoU differs in the last bit between bb_iou and bb_iou_contracted (a seeded search: about
# one random pair in three does)
CONTRACTION_PAIRS = [
    ([10.99187375346119, 0.5511822648613673, 27.6053932602442, 21.144299396578347],
     [9.970264052455743, 2.2817544854317933, 26.03095189457736, 20.77228251242356]),
    ([19.233143873275736, 14.495798815470673, 21.236805666423027, 13.306736121361125],
     [17.1970559259265, 17.315351294767467, 21.365354350806058, 10.233661021127286]),
    ([16.711384330005483, 5.637556547290843, 11.456545014889208, 24.179941401997635],
     [18.54171332887554, 8.419581784360668, 8.660743658258628, 24.03764050759233]),
    ([2.118424734146489, 12.663198920731155, 16.41272809659597, 26.758818142287165],
     [3.0416208005568555, 12.250559413395592, 19.351292141733563, 27.815899082288503]),
    ([16.20548704212598, 6.83589447880226, 21.31007869005367, 10.888906553442602],
     [19.18233418283775, 5.295187264640223, 19.36501842787049, 7.47442713257033]),
    ([5.676129778882622, 6.282677912046044, 14.39143576459813, 22.30099148758856],
     [8.50626963260115, 7.930662721588435, 16.720507349980572, 24.375139491905202]),
    ([5.904685113253915, 16.93996741267459, 8.733809975464395, 27.007713832211103],
     [4.0316335686467255, 16.294918068750086, 6.589009003161502, 29.737537773750198]),
    ([4.024064014493289, 19.764378024404245, 27.749175860114555, 15.793607794778307],
     [4.8731455515269095, 19.05026726016277, 26.801119321233916, 15.824031396334544]),
    ([0.3365456936042599, 6.070178531990214, 34.970776469718125, 12.864403885699684],
     [2.4308128247598924, 6.70427742392444, 37.419062129935114, 13.90694592924751]),
    ([0.6778450103301248, 3.7358735870761706, 25.240681863043324, 22.11693793857495],
     [-1.3708247857495994, 6.448049199433279, 22.475510923422558, 22.19936393648443]),
]


def contraction_scene():
    """-> (dts, gts, thresholds): pair k is the only detection and ground truth of category k, and threshold k is the larger of its
    two IoUs, so that at (pair k, threshold k) separately rounded operations and contracted ones decide differently"""
    dts = [{"id": k + 1, "category": k, "score": 0.5, "box": np.array(d), "area": d[2] * d[3]} for k, (d, _) in enumerate(CONTRACTION_PAIRS)]
    gts = [{"id": k + 1, "category": k, "iscrowd": 0, "box": np.array(g), "area": g[2] * g[3]} for k, (_, g) in enumerate(CONTRACTION_PAIRS)]
    thrs = np.array([max(float(bb_iou([d], [g], [0], "coco")[0, 0]), bb_iou_contracted(d, g)) for d, g in CONTRACTION_PAIRS])
    return dts, gts, thrs


def evaluate_image(dt, gt, a_rng, max_det, iou_thrs, crowd_rule):
    """one (image, category, area range) of evaluateImg with bbIou: the dict of tests/_ap_restate.py's evaluate_image, or None"""
    if len(gt) == 0 and len(dt) == 0:
        return None
    dt = R.sort_dets(dt, max_det)
    ious_all = bb_iou([d["box"] for d in dt], [g["box"] for g in gt], [int(g["iscrowd"]) for g in gt], crowd_rule)
    ignore = [1 if (g["iscrowd"] or (g["area"] < a_rng[0] or g["area"] > a_rng[1])) else 0 for g in gt]
    gtind = np.argsort(ignore, kind="mergesort")
    gt = [gt[i] for i in gtind]
    iscrowd = [int(o["iscrowd"]) for o in gt]
    ious = ious_all[:, gtind]
    T, G, D = len(iou_thrs), len(gt), len(dt)
    gtm = np.zeros((T, G))
    dtm = np.zeros((T, D))
    gt_ig = np.array([ignore[i] for i in gtind])
    dt_ig = np.zeros((T, D))
    if D and G:
        for tind, t in enumerate(iou_thrs):
            for dind, d in enumerate(dt):
                iou = min([t, 1 - 1e-10])
                m = -1
                for gind in range(G):
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


def evaluate(images, K, area_rngs, max_dets, iou_thrs=R.IOU_THRS, crowd_rule="coco"):
    """images: list of (dts, gts) -> evalImgs in the (category, range, image) order of tests/_ap_restate.py"""
    max_det = sorted(max_dets)[-1]
    return [evaluate_image([d for d in dts if d["category"] == k], [g for g in gts if g["category"] == k], rng, max_det, iou_thrs,
                           crowd_rule)
            for k in range(K) for rng in area_rngs for dts, gts in images]


def expected(images, K, area_rngs, max_dets, iou_thrs=R.IOU_THRS, crowd_rule="coco"):
    """-> (the records ``InstanceAP(iou_type="bbox").stats`` must return, the 12 statistics of summarize)"""
    ev = evaluate(images, K, area_rngs, max_dets, iou_thrs, crowd_rule)
    stats = R.expected_stats(images, K, area_rngs, max_dets, iou_thrs, crowd_rule, eval_imgs=ev)
    acc = R.accumulate(ev, K, len(images), area_rngs, max_dets, iou_thrs)
    return stats, R.summarize(acc, max_dets, iou_thrs)
