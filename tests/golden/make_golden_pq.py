"""Generates tests/golden/pq_semantic.npz from the reference's own PQ arithmetic (needs the reference tree, see _ref_import.REF).

``pq_compute_single_image`` of tools/evaluate_pq_for_semantic_segmentation.py is loaded by path and run unmodified on three
label-map pairs.  The file's imports that are not installed are stubbed as _ref_import.py stubs detectron2: ``tqdm``,
``detectron2.data*``, ``detectron2.utils.file_io`` and ``pycocotools`` are not touched by the function; ``panopticapi.evaluation.
PQStat`` is restated with its documented semantics (per-category tp / fp / fn / iou, ``+=`` adds category by category).

Stored: the maps, the per-image tp / fp / fn / iou and their running sum (``pq_stat += single``, as the tool's main loop).

    python tests/golden/make_golden_pq.py
"""
import importlib.util
import os
import sys
import types
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import REF  # noqa: E402

K, IGNORE = 6, 255
SIZES = ((37, 50), (33, 56), (61, 83))


# ---- panopticapi.evaluation.PQStat (third-party, restated) ---------------------------------------------------------------------
class PQStatCat:
    def __init__(self):
        self.iou = 0.0
        self.tp = 0
        self.fp = 0
        self.fn = 0

    def __iadd__(self, other):
        self.iou += other.iou
        self.tp += other.tp
        self.fp += other.fp
        self.fn += other.fn
        return self


class PQStat:
    def __init__(self):
        self.pq_per_cat = defaultdict(PQStatCat)

    def __getitem__(self, i):
        return self.pq_per_cat[i]

    def __iadd__(self, other):
        for label, cat in other.pq_per_cat.items():
            self.pq_per_cat[label] += cat
        return self


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def load_tool():
    _stub("tqdm", tqdm=lambda x, *a, **k: x)
    _stub("detectron2")
    _stub("detectron2.data", MetadataCatalog=None)
    _stub("detectron2.data.detection_utils", read_image=None)
    _stub("detectron2.utils")
    _stub("detectron2.utils.file_io", PathManager=None)
    _stub("pycocotools", mask=None)
    _stub("panopticapi")
    _stub("panopticapi.evaluation", PQStat=PQStat)
    path = os.path.join(REF, "tools", "evaluate_pq_for_semantic_segmentation.py")
    spec = importlib.util.spec_from_file_location("_mpf_ref_pq_tool", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def blocky(g, hw, classes, cell):
    """Piecewise constant map: one draw per cell x cell block."""
    H, W = hw
    small = g.choice(classes, size=((H + cell - 1) // cell, (W + cell - 1) // cell))
    return np.kron(small, np.ones((cell, cell), dtype=np.int64))[:H, :W]


def make_pair(g, hw):
    """gt: blocky classes with ~15 % ignore; prediction: the gt with some blocks redrawn (it agrees on most pixels) and most of ONE
    class painted as another, so that this class misses IoU 0.5: a false negative and a false positive."""
    gt = blocky(g, hw, np.arange(K), 9)
    pred = gt.copy()
    redraw = blocky(g, hw, np.arange(K), 5)
    where = blocky(g, hw, np.array([0] * 7 + [1]), 5).astype(bool)
    pred[where] = redraw[where]
    a, b = g.choice(K, size=2, replace=False)
    pred[(gt == a) & blocky(g, hw, np.array([0, 1, 1, 1]), 3).astype(bool)] = b
    ignore = blocky(g, hw, np.array([0] * 17 + [1] * 3), 4).astype(bool)
    gt[ignore] = IGNORE
    return gt, pred


def as_arrays(stat):
    tp, fp, fn = (np.array([getattr(stat[c], k) for c in range(K)], dtype=np.int64) for k in ("tp", "fp", "fn"))
    return tp, fp, fn, np.array([stat[c].iou for c in range(K)], dtype=np.float64)


def main():
    tool = load_tool()
    categories = {i: {"id": i, "name": str(i), "isthing": 0} for i in range(K)}
    g = np.random.default_rng(20)
    out = {"num_classes": np.int64(K), "ignore_label": np.int64(IGNORE), "num_images": np.int64(len(SIZES))}
    total = PQStat()
    for n, hw in enumerate(SIZES):
        gt, pred = make_pair(g, hw)
        single = tool.pq_compute_single_image(gt, pred, categories, IGNORE)
        total += single
        out[f"gt_{n}"] = gt.astype(np.int32)
        out[f"pred_{n}"] = pred.astype(np.int32)
        for k, v in zip(("tp", "fp", "fn", "iou"), as_arrays(single)):
            out[f"{k}_{n}"] = v
        for k, v in zip(("tp", "fp", "fn", "iou"), as_arrays(total)):
            out[f"sum_{k}_{n}"] = v
        print(n, hw, "ignore share %.3f" % (gt == IGNORE).mean(), "agree %.3f" % (gt == pred).mean(), *as_arrays(single)[:3])
    tp, fp, fn, _ = as_arrays(total)
    assert tp.sum() > 0 and fp.sum() > 0 and fn.sum() > 0, (tp, fp, fn)
    path = os.path.join(HERE, "pq_semantic.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
