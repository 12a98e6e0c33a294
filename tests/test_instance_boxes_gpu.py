"""GPU: ``InferenceConfig.instance_boxes`` — the ``pred_boxes`` of ``postprocess`` and the "boxes" of ``instance_bits`` are the
bounding boxes of the very masks the call returns (``np.any`` over each axis, tests/_box_restate.py), the default keeps the
reference's zeros, and ``d2_plugin.InstanceAPEvaluator(iou_types=("bbox", "segm"))`` scores what a direct ``InstanceAP`` run scores.
Q = 8 queries of 16 x 20 logits on a 64 x 80 padded grid, resampled to 37 x 50 outputs."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _ap_restate as R
import _box_restate as X
from test_ap_cpu import assert_stats_equal

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
Q, K, LOW, PADDED, OUT = 8, 3, (16, 20), (64, 80), (37, 50)
IMAGE_SIZES = [(60, 75), (64, 80)]


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case():
    """two images: smooth blobs of random sign per query; query 0 of the first image is negative everywhere (an empty mask)"""
    from mp_former_amd.inference import InferenceConfig
    g = torch.Generator().manual_seed(7)
    coarse = torch.randn(2, Q, 4, 5, generator=g)
    masks = torch.nn.functional.interpolate(coarse, size=LOW, mode="bilinear", align_corners=False) * 4 - 1
    masks[0, 0] = -5.0
    logits = torch.randn(2, Q, K + 1, generator=g) * 2
    logits[0, 0] = torch.tensor([6.0, 0.0, 0.0, 0.0])   # ... and is selected
    cfg = InferenceConfig(num_classes=K, num_queries=Q, test_topk_per_image=12, instance_on=True)
    return logits.to(DEV), masks.contiguous().to(DEV), cfg


def _run(fn, **options):
    logits, masks, cfg = _case()
    return fn(logits, masks, IMAGE_SIZES, PADDED, [OUT, OUT], dataclasses.replace(cfg, **options))


def test_pred_boxes_are_the_boxes_of_pred_masks():
    from mp_former_amd.inference import instance_bits, postprocess
    with_boxes = _run(postprocess, instance_boxes=True)
    plain = _run(postprocess)
    packed = _run(instance_bits, instance_boxes=True)
    rle = _run(postprocess, instance_boxes=True, instance_masks="rle")
    n_empty = 0
    for a, b, p, r in zip(with_boxes, plain, packed, rle):
        ia, ib = a["instances"], b["instances"]
        assert torch.equal(ia.pred_masks, ib.pred_masks) and torch.equal(ia.scores, ib.scores) and torch.equal(ia.pred_classes, ib.pred_classes)
        dense = _np(ia.pred_masks) > 0
        want = X.boxes_of(dense)
        T = len(want)
        assert T == 12 and dense.any() and tuple(ia.image_size) == OUT
        n_empty += int((~dense.any((1, 2))).sum())
        got = ia.pred_boxes.tensor
        assert got.dtype == torch.float32 and got.device == DEV and tuple(got.shape) == (T, 4)
        np.testing.assert_array_equal(_np(got), want.astype(np.float32))
        assert (want[:, 2] <= OUT[1]).all() and (want[:, 3] <= OUT[0]).all()
        # the default: the reference's zeros
        zeros = ib.pred_boxes.tensor
        assert tuple(zeros.shape) == (T, 4) and not zeros.any() and zeros.dtype == torch.float32
        # the packed route: the same masks, the same boxes, as int32
        assert set(p) == {"bits", "size", "scores", "pred_classes", "boxes"}
        assert p["boxes"].dtype == torch.int32 and p["boxes"].device == DEV
        np.testing.assert_array_equal(_np(p["boxes"]), want)
        np.testing.assert_array_equal(R.unpack_columns(_np(p["bits"]), *OUT)[0], dense)
        # the run-length route carries the same boxes
        np.testing.assert_array_equal(_np(r["instances"].pred_boxes.tensor), want.astype(np.float32))
    assert n_empty > 0, "no empty mask among the selected entries"
    for p in _run(instance_bits):
        assert set(p) == {"bits", "size", "scores", "pred_classes"}, "the default keeps today's keys"


def test_no_instance_gives_empty_boxes():
    """panoptic and instance inference together keep thing classes only: without thing classes nothing is selected"""
    from mp_former_amd.inference import instance_bits, postprocess
    for res in _run(postprocess, instance_boxes=True, panoptic_on=True, thing_ids=frozenset()):
        b = res["instances"].pred_boxes.tensor
        assert tuple(b.shape) == (0, 4) and b.dtype == torch.float32
    for p in _run(instance_bits, instance_boxes=True, panoptic_on=True, thing_ids=frozenset()):
        assert tuple(p["boxes"].shape) == (0, 4) and p["boxes"].dtype == torch.int32


def test_evaluator_scores_bbox_like_a_direct_run():
    from mp_former_amd.d2_plugin import InstanceAPEvaluator
    from mp_former_amd.inference import InstanceAP, boxes_xyxy_to_xywh, instance_bits, pack_masks, postprocess
    dense = _run(postprocess, instance_boxes=True)
    packed = _run(instance_bits, instance_boxes=True)
    gts = []
    for n, d in enumerate(dense):
        pm = _np(d["instances"].pred_masks) > 0
        pick = [i for i in range(len(pm)) if pm[i].any()][:5]
        gm = np.stack([np.roll(pm[i], (j % 3, 2 * (j % 2)), (0, 1)) for j, i in enumerate(pick)])       # the first: a copy
        gt = SimpleNamespace(gt_masks=SimpleNamespace(tensor=torch.from_numpy(gm).to(DEV)),
                             gt_classes=_np(d["instances"].pred_classes)[pick].tolist(), gt_iscrowd=[int(j == 1) for j in range(len(pick))])
        if n == 0:                                       # this image's annotation carries boxes of its own, a little larger
            gt.gt_boxes = SimpleNamespace(tensor=torch.from_numpy(X.boxes_of(gm).astype(np.float32) + np.float32([-0.5, -0.25, 0.5, 0.75])))
        gts.append(gt)
    inputs = [{"instances": gt} for gt in gts]
    outputs = [dense[0], {"instances": packed[1]}]      # Instances with pred_boxes, and the dict with "boxes"
    ev = InstanceAPEvaluator(K, device=DEV, iou_types=("bbox", "segm"))
    ev.reset()
    ev.process(inputs, outputs)
    got = ev.evaluate()
    assert list(got) == ["bbox", "segm"]
    direct = {t: InstanceAP(K, device=DEV, iou_type=t) for t in ("bbox", "segm")}
    for n, (p, gt) in enumerate(zip(packed, gts)):
        gt_bits = pack_masks(gt.gt_masks.tensor)
        args = (p["bits"], p["scores"], p["pred_classes"], gt_bits, gt.gt_classes, gt.gt_iscrowd)
        direct["segm"].update(*args)
        direct["bbox"].update(*args, size=OUT, dt_boxes=boxes_xyxy_to_xywh(p["boxes"]),
                              gt_boxes=boxes_xyxy_to_xywh(gt.gt_boxes.tensor.to(DEV)) if n == 0 else None)
    for t in ("bbox", "segm"):
        assert_stats_equal(ev.aps[t].stats(), direct[t].stats(), t)
        want = direct[t].results()
        assert got[t].keys() == want.keys()
        for k, v in want.items():
            assert got[t][k] == v or (np.isnan(v) and np.isnan(got[t][k])), (t, k)
    assert got["bbox"]["AP"] > 0
    # and against the restatement: the boxes of the masks, the first image's ground truth with its own boxes
    images = []
    for n, (p, gt) in enumerate(zip(packed, gts)):
        db = X.xyxy_to_xywh(X.boxes_of(R.unpack_columns(_np(p["bits"]), *OUT)[0]))
        gm = _np(gt.gt_masks.tensor)
        gb = X.xyxy_to_xywh(_np(gt.gt_boxes.tensor) if n == 0 else X.boxes_of(gm))
        sc, cl = _np(p["scores"]), _np(p["pred_classes"])
        dts = [{"id": i + 1, "category": int(cl[i]), "score": float(sc[i]), "box": db[i], "area": float(db[i][2]) * float(db[i][3])}
               for i in range(len(sc))]
        images.append((dts, [{"id": j + 1, "category": int(gt.gt_classes[j]), "iscrowd": gt.gt_iscrowd[j], "box": gb[j],
                              "area": float(gm[j].sum())} for j in range(len(gb))]))
    assert_stats_equal(ev.aps["bbox"].stats(), X.expected(images, K, R.COCO_AREA_RNGS, (1, 10, 100))[0], "restatement")
    # the reference's placeholder (zeros on the host, the default route) counts as no boxes: the masks' boxes are scored
    with_zeros, with_boxes = InstanceAPEvaluator(K, device=DEV, iou_types=("bbox",)), InstanceAPEvaluator(K, device=DEV, iou_types=("bbox",))
    plain = _run(postprocess)
    assert not plain[0]["instances"].pred_boxes.tensor.is_cuda and not plain[0]["instances"].pred_boxes.tensor.any()
    with_zeros.process(inputs, plain)
    with_boxes.process(inputs, dense)
    assert_stats_equal(with_zeros.ap.stats(), with_boxes.ap.stats(), "placeholder")
    assert with_zeros.evaluate()["bbox"]["AP"] == got["bbox"]["AP"] > 0
    # install_native_inference passes the option through
    import inspect
    from mp_former_amd import d2_plugin
    assert inspect.signature(d2_plugin.install_native_inference).parameters["instance_boxes"].default is False
