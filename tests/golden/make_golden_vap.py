"""Generates tests/golden/vap_small.npz from the reference's own YouTube-VIS evaluation (needs the reference tree, see
_ref_import.REF).

mask2former_video/data_video/datasets/ytvis_api/ytvoseval.py is loaded by path, with the ``pycocotools.mask`` stand-in of
make_golden_ap.py (a truthy wrapper around a dense mask, ``area`` and ``merge``), and its ``evaluate`` / ``accumulate`` /
``summarize`` run unmodified on videos of several frames: ``iou_seq`` over the frames, ``avg_area`` in the area ranges.  An
annotation carries "segmentations" (one stand-in mask or None per frame) and "areas" (the pixel count or None per frame), as
``YTVOS.loadRes`` builds them.

4 videos of F = 1, 3, 4, 4 frames of 23 x 37 pixels (851 positions: 14 words with a 19-bit tail), 3 categories.  Two settings: the
file's own ranges and max_dets, and small ranges (with max_dets (1, 2, 3), so the truncation happens) that every kind of tube here
populates.

Stored: per tube its video, category, score / crowd flag, id, the frames' "present" flags and masks (np.packbits); per setting every
evalImgs entry's dtMatches != 0, dtIgnore, gtIgnore, dtIds, gtIds (flattened, with a shape table), precision, recall, scores, stats.

    python tests/golden/make_golden_vap.py
"""
import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_ap import Mask, flatten, load_eval  # noqa: E402

K = 3
H, W = 23, 37
FRAMES = (1, 3, 4, 4)
SETTINGS = {
    "ytvis": {"area_rngs": [[0 ** 2, 1e5 ** 2], [0 ** 2, 128 ** 2], [128 ** 2, 256 ** 2], [256 ** 2, 1e5 ** 2]], "max_dets": [1, 10, 100]},
    "small": {"area_rngs": [[0, 1e10], [0, 40], [40, 150], [150, 1e10]], "max_dets": [1, 2, 3]},
}


def rect(y, x, h, w):
    assert 0 <= y and y + h <= H and 0 <= x and x + w <= W, (y, x, h, w)
    m = np.zeros((H, W), dtype=bool)
    m[y:y + h, x:x + w] = True
    return m


EMPTY = np.zeros((H, W), dtype=bool)


def scenes():
    """-> (gts, dts): (video, category, frames, iscrowd) and (video, category, frames, score); a frame is a mask or None"""
    gts = [
        (0, 0, [rect(2, 2, 8, 8)], 0),                                              # 1: area 64
        (0, 1, [rect(10, 10, 13, 13)], 0),                                          # 2: area 169, "large" in the small setting
        (1, 0, [rect(1, 1, 10, 10), None, rect(2, 2, 10, 10)], 0),                  # 3: a frame without annotation; avg_area 100
        (1, 0, [rect(12, 0, 10, 20)] * 3, 1),                                       # 4: crowd
        (1, 1, [None, None, None], 0),                                              # 5: no frame at all: avg_area 0
        (1, 1, [rect(0, 25, 6, 6), rect(0, 25, 6, 5), None], 0),                    # 6: avg_area 33
        (1, 0, [rect(12, 22, 6, 6), rect(12, 22, 6, 6), rect(12, 22, 6, 6)], 0),    # 7: area 36, reached by detection 12 in one frame only
        (3, 0, [rect(0, 0, 15, 15)] * 4, 0),                                        # 8: video 3 has ground truth and no detection
        (3, 1, [rect(5, 5, 8, 10)] * 4, 0),                                         # 9: area 80
        (3, 2, [rect(10, 20, 4, 4)] * 4, 0),                                        # 10: area 16
        (3, 1, [rect(16, 20, 5, 16)] * 4, 1),                                       # 11: a crowd nobody reaches
    ]
    dts = [
        (0, 0, [rect(2, 2, 8, 7)], .9),                                             # 1: IoU 56 / 64
        (0, 1, [rect(10, 10, 13, 12)], .75),                                        # 2: IoU 156 / 169
        (0, 1, [rect(0, 30, 3, 3)], .5),                                            # 3: unmatched, area 9
        (1, 0, [rect(1, 1, 10, 10), rect(1, 1, 10, 10), rect(2, 2, 10, 9)], .9),    # 4: 190 / 300 with gt 3: its frame 1 meets no mask
        (1, 0, [rect(13, 1, 4, 4)] * 3, .8),                                        # 5: inside the crowd (IoU 48 / 600: unmatched)
        (1, 0, [rect(14, 8, 5, 5), EMPTY, rect(14, 8, 5, 5)], .7),                  # 6: an empty frame: avg_area 25 over two frames
        (1, 1, [rect(0, 25, 6, 6), rect(0, 25, 6, 5), None], .6),                   # 7: gt 6 exactly
        (1, 1, [None, None, rect(15, 30, 3, 3)], .4),                               # 8: one frame, unmatched, avg_area 9
        (1, 2, [rect(5, 15, 4, 4)] * 3, .3),                                        # 9: category 2 has no ground truth in this video
        (1, 0, [rect(12, 0, 10, 20), rect(12, 0, 10, 19), rect(12, 0, 10, 20)], .85),   # 10: the crowd itself, IoU 590 / 600
        (1, 0, [rect(1, 1, 10, 9), None, rect(2, 2, 10, 10)], .6),                  # 11: gt 3 again, 190 / 200: gt 3 is taken
        (1, 0, [rect(12, 22, 6, 6), None, None], .55),                              # 12: gt 7 in one of three frames: 36 / 108
        (2, 0, [rect(3, 3, 12, 14)] * 4, .85),                                      # 13: video 2 has detections and no ground truth
        (2, 1, [rect(0, 0, 5, 5), rect(0, 0, 5, 5), None, None], .2),               # 14: avg_area 25, the frames' sum 50
        (2, 1, [rect(10, 0, 9, 9)] * 4, .35),                                       # 15: avg_area 81, the frames' sum 324
        (2, 1, [rect(0, 10, 4, 4)] * 4, .3),                                        # 16
        (2, 1, [rect(0, 20, 4, 4)] * 4, .25),                                       # 17: four of category 1 here: max_dets 3 truncates
    ]
    return gts, dts


def annotations(rows, dt):
    out = []
    for n, (vid, c, frames, x) in enumerate(rows):
        assert len(frames) == FRAMES[vid]
        a = {"id": n + 1, "video_id": vid + 1, "category_id": c, "segmentations": [None if m is None else Mask(m) for m in frames],
             "areas": [None if m is None else int(m.sum()) for m in frames], "iscrowd": 0 if dt else x}
        if dt:
            a["score"] = float(np.float32(x))
        out.append(a)
    return out


class Dataset:
    """what YTVOSeval asks of its cocoGt / cocoDt"""

    def __init__(self, anns):
        self.anns = {a["id"]: a for a in anns}

    def getVidIds(self):
        return list(range(1, len(FRAMES) + 1))

    def getCatIds(self):
        return list(range(K))

    def getAnnIds(self, vidIds=(), catIds=()):
        vids, cats = set(int(v) for v in vidIds), set(int(c) for c in catIds)
        return [i for i, a in self.anns.items() if a["video_id"] in vids and a["category_id"] in cats]

    def loadAnns(self, ids):
        return [self.anns[i] for i in ids]

    def annToRLE(self, ann, i):
        return ann["segmentations"][i]


def run(mod, gts, dts, setting):
    with contextlib.redirect_stdout(io.StringIO()):
        e = mod.YTVOSeval(Dataset(annotations(gts, False)), Dataset(annotations(dts, True)), "segm")
        e.params.areaRng = [list(r) for r in setting["area_rngs"]]
        e.params.maxDets = list(setting["max_dets"])
        e.evaluate()
        e.accumulate()
        e.summarize()
    return e


def coverage(evals, gts, dts):
    """the data covers what the tube route can get wrong"""
    small = evals["small"]
    ents = [x for x in small.evalImgs if x is not None]
    rngs = SETTINGS["small"]["area_rngs"]
    for r in rngs:
        assert any(not bool(i) for x in ents if list(x["aRng"]) == list(r) for i in x["gtIgnore"]), f"range {r} holds no ground truth"
    all_rng = [x for x in ents if list(x["aRng"]) == list(rngs[0])]
    crowd_ids = {n + 1 for n, g in enumerate(gts) if g[3]}
    assert any(int(v) in crowd_ids for x in all_rng for v in x["dtMatches"][0]), "no match on a crowd ground truth"
    # an unmatched detection whose avg_area lies in another range than the sum of its frames would
    def rng_of(v):
        return [i for i, r in enumerate(rngs) if r[0] <= v <= r[1]]
    unmatched = {int(i) for x in all_rng for i, m in zip(x["dtIds"], x["dtMatches"][0]) if m == 0}
    differs = [n + 1 for n, d in enumerate(dts)
               if rng_of(np.mean([m.sum() for m in d[2] if m is not None and m.any()])) != rng_of(sum(m.sum() for m in d[2] if m is not None))]
    assert unmatched & set(differs), "no unmatched detection separates avg_area from the summed area"
    assert any(a["avg_area"] == 0 for a in small.cocoGt.anns.values()), "no ground truth without any frame"
    assert any(None in [None if m is None else 1 for m in g[2]] and any(m is not None for m in g[2]) for g in gts)
    assert any(m is not None and not m.any() for d in dts for m in d[2]), "no detection with an empty frame"
    vids_gt, vids_dt = {g[0] for g in gts}, {d[0] for d in dts}
    assert vids_dt - vids_gt and vids_gt - vids_dt, "need a video with detections only and one with ground truth only"
    per = {}
    for d in dts:
        per[d[0], d[1]] = per.get((d[0], d[1]), 0) + 1
    assert max(per.values()) > SETTINGS["small"]["max_dets"][-1], "no truncation"
    thr = small.params.iouThrs
    tp = np.zeros(len(thr), dtype=bool)
    fp = np.zeros(len(thr), dtype=bool)
    for x in all_rng:
        m, ig = x["dtMatches"] != 0, np.asarray(x["dtIgnore"]).astype(bool)
        tp |= (m & ~ig).any(1)
        fp |= (~m & ~ig).any(1)
    assert tp[0] and fp.all(), (tp, fp)


def pack_rows(rows):
    present = np.asarray([m is not None for r in rows for m in r[2]], dtype=bool)
    masks = np.concatenate([(EMPTY if m is None else m).ravel() for r in rows for m in r[2]])
    return present, np.packbits(masks)


def main():
    mod = load_eval()
    gts, dts = scenes()
    evals = {name: run(mod, gts, dts, s) for name, s in SETTINGS.items()}
    coverage(evals, gts, dts)
    gp, gm = pack_rows(gts)
    dp, dm = pack_rows(dts)
    out = {"num_classes": np.int64(K), "size": np.asarray([H, W], dtype=np.int64), "frames": np.asarray(FRAMES, dtype=np.int64),
           "gt_video": np.asarray([g[0] for g in gts], dtype=np.int64), "gt_category": np.asarray([g[1] for g in gts], dtype=np.int64),
           "gt_crowd": np.asarray([g[3] for g in gts], dtype=np.int64), "gt_id": np.arange(1, len(gts) + 1),
           "gt_present": gp, "gt_masks": gm,
           "gt_avg_area": np.asarray([evals["small"].cocoGt.anns[n + 1]["avg_area"] for n in range(len(gts))], dtype=np.float64),
           "dt_video": np.asarray([d[0] for d in dts], dtype=np.int64), "dt_category": np.asarray([d[1] for d in dts], dtype=np.int64),
           "dt_score": np.asarray([d[3] for d in dts], dtype=np.float32), "dt_id": np.arange(1, len(dts) + 1),
           "dt_present": dp, "dt_masks": dm,
           "dt_avg_area": np.asarray([evals["small"].cocoDt.anns[n + 1]["avg_area"] for n in range(len(dts))], dtype=np.float64),
           "iou_thrs": np.asarray(evals["small"].params.iouThrs, dtype=np.float64),
           "rec_thrs": np.asarray(evals["small"].params.recThrs, dtype=np.float64)}
    for name, s in SETTINGS.items():
        out[f"{name}_area_rngs"] = np.asarray(s["area_rngs"], dtype=np.float64)
        out[f"{name}_max_dets"] = np.asarray(s["max_dets"], dtype=np.int64)
    for name, e in evals.items():
        for k, v in flatten(e).items():
            out[f"{name}_{k}"] = v
        for k in ("precision", "recall", "scores"):
            out[f"{name}_{k}"] = np.asarray(e.eval[k], dtype=np.float64)
        out[f"{name}_stats"] = np.asarray(e.stats, dtype=np.float64)
        print(name, np.round(e.stats, 4))
    path = os.path.join(HERE, "vap_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
