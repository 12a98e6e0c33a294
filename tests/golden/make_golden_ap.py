"""Generates tests/golden/ap_instances.npz from the reference's own COCO evaluation body (needs the reference tree, see
_ref_import.REF).

mask2former_video/data_video/datasets/ytvis_api/ytvoseval.py is loaded by path and its ``evaluate`` / ``accumulate`` /
``summarize`` run unmodified; its ``evaluateVid`` is the body of ``COCOeval.evaluateImg`` and an image is a one-frame video.
``pycocotools.mask`` is not installed: it is stubbed with ``area`` and ``merge`` on a small wrapper around a dense mask (truthy,
because ``_toMask`` tests ``if a:``), and ``np.float = float`` is set in this process only (the file predates numpy 1.24).  Two
tiny dataset stand-ins provide getVidIds / getCatIds / getAnnIds / loadAnns / annToRLE.

The unmodified class gives the golden of ``crowd_rule="union"`` (its own computeIoU takes the plain union for every pair); a
subclass that overrides ONLY ``computeIoU`` with pycocotools' rleIou crowd rule (a crowd ground truth divides by the detection's
area) gives the golden of ``crowd_rule="coco"``.  Two settings: COCO's default ranges and max_dets, and scaled-down ranges with
max_dets (1, 3, 5) so that all four ranges are populated and the truncation happens.

Stored: the masks (np.packbits), ids, categories, float32 scores, crowd flags, areas; per (rule, setting) every evalImgs entry's
dtMatches != 0, dtIgnore, gtIgnore, dtIds and gtIds (flattened, with a shape table), and precision, recall, scores, stats.

    python tests/golden/make_golden_ap.py
"""
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REF  # noqa: E402

K = 4
SIZES = ((37, 50), (33, 56), (61, 83))
SETTINGS = {
    "coco": {"area_rngs": [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], "max_dets": [1, 10, 100]},
    "small": {"area_rngs": [[0, 1e10], [0, 64], [64, 400], [400, 1e10]], "max_dets": [1, 3, 5]},
}
RULES = ("union", "coco")


class Mask:
    """the stand-in for an RLE: a dense bool mask; truthy whatever it holds"""

    def __init__(self, a):
        self.a = a

    def __bool__(self):
        return True


def _area(m):
    return int(m.a.sum())


def _merge(ms, intersect=False):
    a, b = ms
    return Mask(a.a & b.a) if intersect else Mask(a.a | b.a)


def load_eval():
    pkg = types.ModuleType("pycocotools")
    mask = types.ModuleType("pycocotools.mask")
    mask.area, mask.merge = _area, _merge
    pkg.mask = mask
    sys.modules["pycocotools"], sys.modules["pycocotools.mask"] = pkg, mask
    np.float = float
    path = os.path.join(REF, "mask2former_video", "data_video", "datasets", "ytvis_api", "ytvoseval.py")
    spec = importlib.util.spec_from_file_location("_mpf_ref_ytvoseval", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Dataset:
    """what YTVOSeval asks of its cocoGt / cocoDt"""

    def __init__(self, anns):
        self.anns = {a["id"]: a for a in anns}

    def getVidIds(self):
        return list(range(1, len(SIZES) + 1))

    def getCatIds(self):
        return list(range(K))

    def getAnnIds(self, vidIds=(), catIds=()):
        vids, cats = set(int(v) for v in vidIds), set(int(c) for c in catIds)
        return [i for i, a in self.anns.items() if a["video_id"] in vids and a["category_id"] in cats]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]

    def annToRLE(self, ann, i):
        return ann["segmentations"][i]


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def rect(img, y, x, h, w, drop=0):
    """a rectangle with its first `drop` pixels (row-major) cleared"""
    H, W = SIZES[img]
    assert 0 <= y and y + h <= H and 0 <= x and x + w <= W, (img, y, x, h, w)
    m = np.zeros((H, W), dtype=bool)
    m[y:y + h, x:x + w] = True
    ys, xs = np.nonzero(m)
    m[ys[:drop], xs[:drop]] = False
    return m


def scenes():
    """-> (gts, dts): lists of (image, category, mask, iscrowd) and (image, category, mask, score), in annotation order"""
    gts = [
        (0, 0, rect(0, 2, 2, 10, 10), 0),        # 1: area 100
        (0, 0, rect(0, 2, 20, 3, 2), 0),         # 2: area 6; detection 2 has IoU 3/6 = the first threshold exactly
        (0, 0, rect(0, 15, 0, 20, 30), 1),       # 3: crowd
        (0, 1, rect(0, 0, 35, 30, 14), 0),       # 4: area 420
        (0, 3, rect(0, 32, 40, 4, 8), 0),        # 5: category 3 has no detection anywhere
        (0, 0, rect(0, 2, 26, 2, 2), 0),         # 6: area 4; detection 3 has IoU 3/4
        (0, 0, rect(0, 28, 10, 8, 10), 0),       # 7: area 80, partly under the crowd: the break rule (detection 7)
        (1, 0, rect(1, 1, 1, 20, 25), 0),        # 8: area 500
        (1, 1, rect(1, 3, 30, 8, 8), 0),         # 9: area 64, on the edge of two of the small ranges
        (1, 1, rect(1, 15, 28, 15, 25), 1),      # 10: crowd
        (2, 0, rect(2, 5, 5, 40, 40), 0),        # 11: area 1600, "medium" under the COCO ranges
        (2, 1, rect(2, 0, 50, 50, 30), 0),       # 12: area 1500
        (2, 0, rect(2, 50, 0, 10, 12), 0),       # 13: area 120
        (2, 3, rect(2, 50, 60, 8, 8), 0),        # 14
        (2, 1, rect(2, 55, 40, 4, 5), 0),        # 15: area 20; detection 22 has IoU 17/20 = the 0.85 threshold as linspace gives it
        (2, 0, rect(2, 50, 0, 10, 12), 0),       # 16: the same pixels as 13: detection 18 has IoU 1 with both, the later one wins
    ]
    dts = [
        (0, 0, rect(0, 2, 2, 10, 10), .9),       # 1: IoU 1 with gt 1
        (0, 0, rect(0, 2, 20, 3, 1), .8),        # 2: IoU 1/2 with gt 2
        (0, 0, rect(0, 2, 26, 2, 2, drop=1), .8),    # 3: IoU 3/4 with gt 6; the score ties with 2 and, across images, with 18
        (0, 0, rect(0, 16, 1, 5, 5), .7),        # 4: inside the crowd
        (0, 0, rect(0, 22, 8, 6, 6), .6),        # 5: inside the same crowd
        (0, 0, rect(0, 30, 35, 5, 5), .5),       # 6: on a ground truth of another category: a false positive
        (0, 0, rect(0, 28, 10, 8, 8), .4),       # 7: IoU 0.8 with gt 7 and 0.875 with the crowd under the "coco" rule
        (0, 1, rect(0, 0, 35, 30, 13), .95),     # 8: IoU 390/420
        (0, 2, rect(0, 5, 5, 4, 4), .3),         # 9: category 2 has no ground truth anywhere
        (1, 0, rect(1, 1, 1, 20, 24), .9),       # 10: IoU 0.96; the score ties with 1 across images
        (1, 0, rect(1, 25, 40, 3, 3), .2),       # 11
        (1, 1, rect(1, 3, 30, 8, 7), .8),        # 12: IoU 0.875
        (1, 1, rect(1, 16, 30, 5, 5), .5),       # 13: inside the crowd
        (1, 1, rect(1, 0, 50, 2, 2), .45),       # 14: area 4, unmatched: ignored outside the range that holds it
        (2, 0, rect(2, 5, 5, 40, 36), .85),      # 15: IoU 0.9
        (2, 1, rect(2, 0, 50, 50, 27), .7),      # 16: IoU 0.9
        (2, 1, rect(2, 55, 30, 5, 5), .1),       # 17
        (2, 0, rect(2, 50, 0, 10, 12), .8),      # 18: gt 13 and gt 16 exactly: equal IoU
        (2, 2, rect(2, 20, 60, 5, 5), .6),       # 19
        (2, 1, rect(2, 30, 0, 3, 3), .3),        # 20
        (2, 1, rect(2, 40, 0, 3, 3), .3),        # 21: ties with 20 inside the category
        (2, 1, rect(2, 55, 40, 4, 5, drop=3), .65),  # 22: IoU 17/20 with gt 15
    ]
    return gts, dts


def datasets(gts, dts):
    """fresh annotation dicts: evaluate() writes into them"""
    g = [{"id": n + 1, "video_id": img + 1, "category_id": c, "segmentations": [Mask(m)], "areas": [int(m.sum())], "iscrowd": cr}
         for n, (img, c, m, cr) in enumerate(gts)]
    d = [{"id": n + 1, "video_id": img + 1, "category_id": c, "segmentations": [Mask(m)], "areas": [int(m.sum())], "iscrowd": 0,
          "score": float(np.float32(s))} for n, (img, c, m, s) in enumerate(dts)]
    return Dataset(g), Dataset(d)


def coco_rule_class(base):
    class CocoCrowdEval(base):
        """only computeIoU differs: pycocotools' rleIou, where a crowd ground truth divides by the detection's area"""

        def computeIoU(self, vidId, catId):
            p = self.params
            gt, dt = self._gts[vidId, catId], self._dts[vidId, catId]
            if len(gt) == 0 and len(dt) == 0:
                return []
            inds = np.argsort([-d["score"] for d in dt], kind="mergesort")
            dt = [dt[i] for i in inds][:p.maxDets[-1]]
            ious = np.zeros([len(dt), len(gt)])
            for i, j in np.ndindex(ious.shape):
                d, g = dt[i]["segmentations"][0], gt[j]["segmentations"][0]
                inter = _area(_merge([d, g], True))
                union = _area(d) if int(gt[j]["iscrowd"]) else _area(_merge([d, g], False))
                ious[i, j] = inter / union if inter > 0 else .0
            return ious
    return CocoCrowdEval


def run(cls, gts, dts, setting):
    gt_set, dt_set = datasets(gts, dts)
    with contextlib.redirect_stdout(io.StringIO()):
        e = cls(gt_set, dt_set, "segm")
        e.params.areaRng = [list(r) for r in setting["area_rngs"]]
        e.params.maxDets = list(setting["max_dets"])
        e.evaluate()
        e.accumulate()
        e.summarize()
    return e


def flatten(e):
    """every evalImgs entry in its stored (category, range, image) order -> the flat arrays and the [entries, 3] table (D, G, exists)"""
    table, dtm, dtig, gtig, dtids, gtids = [], [], [], [], [], []
    for x in e.evalImgs:
        if x is None:
            table.append((0, 0, 0))
            continue
        table.append((len(x["dtIds"]), len(x["gtIds"]), 1))
        dtm.append((np.asarray(x["dtMatches"]) != 0).ravel())
        dtig.append(np.asarray(x["dtIgnore"]).astype(bool).ravel())
        gtig.append(np.asarray(x["gtIgnore"]).astype(bool).ravel())
        dtids.append(np.asarray(x["dtIds"], dtype=np.int64))
        gtids.append(np.asarray(x["gtIds"], dtype=np.int64))
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)     # noqa: E731
    return {"table": np.asarray(table, dtype=np.int64), "dtm": cat(dtm, bool), "dtig": cat(dtig, bool), "gtig": cat(gtig, bool),
            "dtids": cat(dtids, np.int64), "gtids": cat(gtids, np.int64)}


def coverage(evals, gts, dts):
    """the data covers what the kernels can get wrong"""
    e = evals["coco", "coco"]
    thr = e.params.iouThrs
    ents = [x for x in e.evalImgs if x is not None]
    all_rng = [x for x in ents if x["aRng"] == [0, 1e10]]
    crowd_ids = {n + 1 for n, g in enumerate(gts) if g[3]}
    hits = [int(v) for x in all_rng for v in x["dtMatches"][0] if int(v) in crowd_ids]
    assert hits, "no match on a crowd ground truth"
    assert any(hits.count(c) >= 2 for c in crowd_ids), "no crowd matched by two detections"
    assert any((np.asarray(x["dtIgnore"]).astype(bool) & (x["dtMatches"] == 0)).any() for x in ents), "no detection ignored by its area"
    # the break rule: detection 7 prefers the crowd by IoU and still takes the plain ground truth 7 at the first threshold
    x = [x for x in all_rng if x["video_id"] == 1 and x["category_id"] == 0][0]
    ious = e.ious[1, 0]
    row = x["dtIds"].index(7)
    g_order = [g["id"] for g in e._gts[1, 0]]
    assert ious[row, g_order.index(3)] > ious[row, g_order.index(7)] >= thr[0]
    assert x["dtMatches"][0][row] == 7 and not x["dtIgnore"][0][row], "the break rule did not decide detection 7"
    assert x["dtMatches"][7][row] == 3, "above its plain IoU detection 7 goes to the crowd"
    # equal IoU: the later ground truth wins
    x2 = [x for x in all_rng if x["video_id"] == 3 and x["category_id"] == 0][0]
    i2 = e.ious[3, 0]
    r2 = x2["dtIds"].index(18)
    o2 = [g["id"] for g in e._gts[3, 0]]
    assert i2[r2, o2.index(13)] == i2[r2, o2.index(16)] and x2["dtMatches"][0][r2] == 16
    sc = [(d[0], d[1], float(np.float32(d[3]))) for d in dts]
    assert any(a[:2] == b[:2] and a[2] == b[2] for i, a in enumerate(sc) for b in sc[i + 1:]), "no score tie inside a category"
    assert any(a[0] != b[0] and a[1] == b[1] and a[2] == b[2] for i, a in enumerate(sc) for b in sc[i + 1:]), "no tie across images"
    on_thr = [(t, float(v)) for m in e.ious.values() if len(m) for v in np.asarray(m).ravel() for t in range(len(thr)) if v == thr[t]]
    assert {t for t, _ in on_thr} >= {0, 5, 7}, on_thr              # 1/2, 3/4 and 17/20 sit exactly on their thresholds ...
    x3 = [x for x in all_rng if x["video_id"] == 3 and x["category_id"] == 1][0]
    assert x3["dtMatches"][7][x3["dtIds"].index(22)] == 15            # ... and match there
    for name in ("coco", "small"):
        for rule in RULES:
            ev = evals[rule, name]
            rngs = {tuple(x["aRng"]) for x in ev.evalImgs if x is not None}
            assert len(rngs) == 4
            tp = np.zeros(len(thr), dtype=bool)
            fp = np.zeros(len(thr), dtype=bool)
            for x in ev.evalImgs:
                if x is None or x["aRng"] != [0, 1e10]:
                    continue
                m, ig = x["dtMatches"] != 0, np.asarray(x["dtIgnore"]).astype(bool)
                tp |= (m & ~ig).any(1)
                fp |= (~m & ~ig).any(1)
            assert tp.all() and fp.all(), (rule, name, tp, fp)
    small = evals["coco", "small"]
    assert all(any(not bool(i) for x in small.evalImgs if x is not None and list(x["aRng"]) == list(r) for i in x["gtIgnore"])
               for r in SETTINGS["small"]["area_rngs"]), "a range of the small setting holds no ground truth"
    per = {}
    for d in dts:
        per[d[0], d[1]] = per.get((d[0], d[1]), 0) + 1
    assert max(per.values()) > SETTINGS["small"]["max_dets"][-1], "no truncation"
    assert not any(g[1] == 2 for g in gts) and any(d[1] == 2 for d in dts), "category 2: detections, no ground truth"
    assert not any(d[1] == 3 for d in dts) and any(g[1] == 3 for g in gts), "category 3: ground truth, no detection"


def main():
    mod = load_eval()
    gts, dts = scenes()
    classes = {"union": mod.YTVOSeval, "coco": coco_rule_class(mod.YTVOSeval)}
    evals = {(rule, name): run(classes[rule], gts, dts, s) for rule in RULES for name, s in SETTINGS.items()}
    coverage(evals, gts, dts)
    out = {"num_classes": np.int64(K), "sizes": np.asarray(SIZES, dtype=np.int64),
           "gt_image": np.asarray([g[0] for g in gts], dtype=np.int64), "gt_category": np.asarray([g[1] for g in gts], dtype=np.int64),
           "gt_crowd": np.asarray([g[3] for g in gts], dtype=np.int64), "gt_area": np.asarray([g[2].sum() for g in gts], dtype=np.float64),
           "gt_id": np.arange(1, len(gts) + 1), "dt_image": np.asarray([d[0] for d in dts], dtype=np.int64),
           "dt_category": np.asarray([d[1] for d in dts], dtype=np.int64), "dt_score": np.asarray([d[3] for d in dts], dtype=np.float32),
           "dt_area": np.asarray([d[2].sum() for d in dts], dtype=np.float64), "dt_id": np.arange(1, len(dts) + 1),
           "gt_masks": np.packbits(np.concatenate([g[2].ravel() for g in gts])),
           "dt_masks": np.packbits(np.concatenate([d[2].ravel() for d in dts])),
           "iou_thrs": np.asarray(evals["coco", "coco"].params.iouThrs, dtype=np.float64),
           "rec_thrs": np.asarray(evals["coco", "coco"].params.recThrs, dtype=np.float64)}
    for name, s in SETTINGS.items():
        out[f"{name}_area_rngs"] = np.asarray(s["area_rngs"], dtype=np.float64)
        out[f"{name}_max_dets"] = np.asarray(s["max_dets"], dtype=np.int64)
    for (rule, name), e in evals.items():
        for k, v in flatten(e).items():
            out[f"{rule}_{name}_{k}"] = v
        for k in ("precision", "recall", "scores"):
            out[f"{rule}_{name}_{k}"] = np.asarray(e.eval[k], dtype=np.float64)
        out[f"{rule}_{name}_stats"] = np.asarray(e.stats, dtype=np.float64)
        print(rule, name, np.round(e.stats, 4))
    path = os.path.join(HERE, "ap_instances.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
