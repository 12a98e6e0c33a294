"""Numpy restatement of boundary-iou-api as the reference's tools/evaluate_coco_boundary_ap.py uses it
(``boundary_iou.coco_instance_api`` with ``iouType="boundary"``, ``dilation_ratio=0.020``): ``mask_to_boundary`` and the pair IoU of
``COCOeval.computeBoundaryIoU``, in the package's own loop form.  Neither boundary_iou, cv2 nor pycocotools is installed where these
tests run: this file IS the specification, and tests/test_boundary_ap_cpu.py holds its erosion to scipy.ndimage.binary_erosion as
an independent second formulation.  The rest of the evaluation (matching, accumulate, summarize) is tests/_ap_restate.py, driven
with this file's ``compute_iou`` in place of its own (``patched``)."""
import contextlib

import numpy as np

import _ap_restate as R


def boundary_dilation(H, W, dilation_ratio=0.02):
    """the package's ``dilation = int(round(dilation_ratio * img_diag))``, ``if dilation < 1: dilation = 1``"""
    img_diag = np.sqrt(H ** 2 + W ** 2)
    dilation = int(round(dilation_ratio * img_diag))
    if dilation < 1:
        dilation = 1
    return dilation


def _erode3x3(m):
    """cv2.erode with a 3 x 3 all-ones element, one iteration, on an already padded image (the pad absorbs the border)"""
    out = np.zeros_like(m)
    out[1:-1, 1:-1] = (m[:-2, :-2] & m[:-2, 1:-1] & m[:-2, 2:] & m[1:-1, :-2] & m[1:-1, 1:-1] & m[1:-1, 2:]
                       & m[2:, :-2] & m[2:, 1:-1] & m[2:, 2:])
    return out


def erode(mask, d):
    """copyMakeBorder(mask, 1, 1, 1, 1, BORDER_CONSTANT, value=0), erode(..., iterations=d), crop"""
    mask = np.asarray(mask) != 0
    h, w = mask.shape
    padded = np.zeros((h + 2, w + 2), dtype=bool)
    padded[1:-1, 1:-1] = mask
    for _ in range(d):
        padded = _erode3x3(padded)
    return padded[1:h + 1, 1:w + 1]


def mask_to_boundary(mask, d):
    """``mask - mask_erode``: the pixels of the mask within ``d`` of its outside"""
    mask = np.asarray(mask) != 0
    return mask & ~erode(mask, d)


def compute_iou(dilation_ratio=0.02, d=None):
    """-> a ``compute_iou(dt, gt, max_det, crowd_rule)`` for tests/_ap_restate.py: computeBoundaryIoU's
    ``min(mask IoU, boundary IoU)``, each of the two by _ap_restate.compute_iou (the crowd rule applies to both)"""
    def to_boundaries(items):
        out = []
        for o in items:
            m = o["mask"]
            dd = boundary_dilation(m.shape[0], m.shape[1], dilation_ratio) if d is None else d
            out.append({**o, "mask": mask_to_boundary(m, dd)})
        return out

    def fn(dt, gt, max_det, crowd_rule):
        mask_iou = _MASK_IOU(dt, gt, max_det, crowd_rule)
        if len(gt) == 0 and len(dt) == 0:
            return mask_iou
        return np.minimum(mask_iou, _MASK_IOU(to_boundaries(dt), to_boundaries(gt), max_det, crowd_rule))
    return fn


_MASK_IOU = R.compute_iou          # the module's own, whatever ``patched`` puts in its place


@contextlib.contextmanager
def patched(dilation_ratio=0.02, d=None):
    """inside the block, _ap_restate's evaluate / expected_stats compute Boundary IoUs; the file itself is not edited"""
    R.compute_iou = compute_iou(dilation_ratio, d)
    try:
        yield R
    finally:
        R.compute_iou = _MASK_IOU
