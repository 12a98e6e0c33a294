"""GPU: a large-scale-jitter batch formed on the device (mp_former_amd.augment.lsj_batch / lsj_targets and
d2_plugin.install_native_lsj) against the restatements: the images against tests/_resample_restate.py, the masks against
tests/_codec_restate.py's rasterisation of the restatement's transformed polygons, labels and boxes against the restatement.
Integer (and float64 / float32 bit) equality."""
import functools

import numpy as np
import pytest
import torch

import _codec_restate as C
import _resample_restate as R
from test_lsj_cpu import source

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S = 32


def _np(t):
    return t.detach().cpu().numpy()


def _samples():
    """two samples of S = 32: 37 x 53 flipped and upscaled (a crop window inside the resized image), 48 x 64 downscaled (padding)"""
    from mp_former_amd.augment import lsj_params
    a = {"image_raw": torch.from_numpy(source(37, 53)), "lsj": lsj_params(37, 53, True, 2.0, 0.5, S), "annotations": [
        {"category_id": 5, "iscrowd": 0, "segmentation": [[20.0, 10.0, 36.5, 11.0, 30.0, 27.5], [24.0, 20.0, 33.0, 21.0, 27.0, 30.25, 22.5, 26.0]]},
        {"category_id": 2, "iscrowd": 0, "segmentation": [[1.0, 1.0, 6.0, 1.5, 3.0, 5.0]]},                 # wholly outside the crop: kept, empty
        {"category_id": 9, "iscrowd": 1, "segmentation": [[20.0, 10.0, 36.0, 11.0, 30.0, 27.0]]},           # crowd: dropped
        {"category_id": 7, "iscrowd": 0, "segmentation": [[15.0, 8.0, 45.0, 8.0, 45.0, 30.0, 15.0, 30.0]]}]}
    b = {"image_raw": torch.from_numpy(source(48, 64)), "lsj": lsj_params(48, 64, False, 0.4, 0.3, S), "annotations": [
        {"category_id": 1, "segmentation": [[5.0, 5.0, 60.0, 7.0, 33.0, 44.0]]},
        {"category_id": 3, "iscrowd": 0, "segmentation": [[10.5, 30.0, 20.0, 30.0, 20.0, 40.0]]}]}
    return [a, b]


@functools.lru_cache(maxsize=None)
def _expected():
    """per sample (image uint8 [3, S, S], labels, masks bool [T, S, S], boxes float32 [T, 4]) from the restatements, made once"""
    out = []
    for s in _samples():
        p = s["lsj"]
        image = R.lsj_image(_np(s["image_raw"]), p.flip, p.resized, p.offset, p.crop)
        labels, polys, boxes = R.lsj_annotations(s["annotations"], p.flip, p.src, p.resized, p.offset)
        masks = np.stack([C.poly_mask([r.tolist() for r in rings], S, S) for rings in polys]) if polys else np.zeros((0, S, S), dtype=bool)
        out.append((image, labels, masks, boxes))
    return out


def test_the_samples_are_the_cases_they_claim_to_be():
    pa, pb = (s["lsj"] for s in _samples())
    assert pa.flip and pa.resized == (45, 64) and pa.offset == (6, 16) and pa.valid == (S, S)
    assert not pb.flip and pb.resized == (10, 13) and pb.offset == (0, 0) and pb.valid == (10, 13)
    (_, la, ma, _), (_, lb, mb, _) = _expected()
    assert la.tolist() == [5, 2, 7] and lb.tolist() == [1, 3]
    assert ma[0].any() and not ma[1].any() and ma[2].any() and mb.any(axis=(1, 2)).all()
    one = C.poly_mask([R.transform_ring(_samples()[0]["annotations"][0]["segmentation"][0], True, (37, 53), (45, 64), (6, 16)).tolist()], S, S)
    assert (ma[0] & ~one).any(), "the second ring adds pixels"


def _check(t, want):
    image, labels, masks, boxes = want
    assert t["labels"].dtype == torch.int64 and t["labels"].device == DEV
    np.testing.assert_array_equal(_np(t["labels"]), labels)
    assert t["masks"].dtype == torch.bool and tuple(t["masks"].shape) == (len(labels), S, S)
    np.testing.assert_array_equal(_np(t["masks"]), masks)
    assert t["boxes"].dtype == torch.float32 and tuple(t["boxes"].shape) == (len(labels), 4)
    np.testing.assert_array_equal(_np(t["boxes"]), boxes)
    assert t["bits"].dtype == torch.int64 and tuple(t["bits"].shape) == (len(labels), (S * S + 63) // 64)


def test_lsj_batch_equals_the_restatements():
    from mp_former_amd.augment import lsj_batch, lsj_targets
    from mp_former_amd.inference import unpack_masks
    samples = _samples()
    images, targets = lsj_batch(samples)
    assert images.dtype == torch.uint8 and tuple(images.shape) == (2, 3, S, S) and images.device == DEV
    for b, want in enumerate(_expected()):
        np.testing.assert_array_equal(_np(images[b]), want[0], err_msg=str(b))
        _check(targets[b], want)
        np.testing.assert_array_equal(_np(unpack_masks(targets[b]["bits"], (S, S))), want[2])
        _check(lsj_targets(samples[b]["annotations"], samples[b]["lsj"], device=DEV), want)
    assert (_np(images[1])[:, 10:, :] == 128).all() and (_np(images[1])[:, :, 13:] == 128).all()


def test_a_sample_without_annotation_has_empty_targets():
    from mp_former_amd.augment import lsj_batch
    samples = _samples()
    samples[0] = {k: v for k, v in samples[0].items() if k != "annotations"}
    samples[1]["annotations"] = []
    images, targets = lsj_batch(samples)
    for b in (0, 1):
        np.testing.assert_array_equal(_np(images[b]), _expected()[b][0])
        assert tuple(targets[b]["masks"].shape) == (0, S, S) and targets[b]["masks"].dtype == torch.bool
        assert tuple(targets[b]["labels"].shape) == (0,) and tuple(targets[b]["boxes"].shape) == (0, 4)
    # and next to a sample that has some
    samples = _samples()
    samples[0]["annotations"] = []
    images, targets = lsj_batch(samples)
    assert tuple(targets[0]["masks"].shape) == (0, S, S)
    np.testing.assert_array_equal(_np(targets[1]["masks"]), _expected()[1][2])


def test_lsj_batch_normalised_on_a_divisible_canvas():
    from mp_former_amd.augment import lsj_batch
    mean, std = [123.675, 116.280, 103.530], [58.395, 57.120, 57.375]
    images, _ = lsj_batch(_samples(), dtype=torch.float32, mean=mean, std=std, canvas=(64, 64))
    for b, want in enumerate(_expected()):
        u8 = torch.from_numpy(want[0]).to(DEV)
        ref = torch.zeros(3, 64, 64, device=DEV)
        ref[:, :S, :S] = (u8.float() - torch.tensor(mean, device=DEV)[:, None, None]) / torch.tensor(std, device=DEV)[:, None, None]
        assert torch.equal(images[b].view(torch.int32), ref.view(torch.int32)), b


class _StubModel:
    """what install_native_lsj touches of a reference MaskFormer: ``training``, ``device`` and ``forward``"""

    def __init__(self):
        self.training, self.device, self.seen = True, DEV, []

    def forward(self, batched_inputs):
        self.seen.append(batched_inputs)
        return {"n": len(batched_inputs)}


def test_install_native_lsj_hands_the_usual_dicts_on():
    from mp_former_amd import d2_plugin
    model = _StubModel()
    d2_plugin.install_native_lsj(model)
    samples = _samples()
    samples[0]["image_id"] = 41
    assert model.forward(samples) == {"n": 2}
    (got,) = model.seen
    assert len(got) == 2 and got[0]["image_id"] == 41 and "image_raw" not in got[0] and "annotations" not in got[0]
    assert "image_raw" in samples[0], "the input was modified"
    for d, (image, labels, masks, boxes) in zip(got, _expected()):
        assert d["image"].dtype == torch.uint8 and tuple(d["image"].shape) == (3, S, S) and d["image"].device == DEV
        np.testing.assert_array_equal(_np(d["image"]), image)
        inst = d["instances"]
        assert tuple(inst.image_size) == (S, S) and len(inst) == len(labels)
        assert inst.gt_masks.dtype == torch.bool and tuple(inst.gt_masks.shape) == (len(labels), S, S)
        np.testing.assert_array_equal(_np(inst.gt_masks), masks)
        np.testing.assert_array_equal(_np(inst.gt_classes), labels)
        np.testing.assert_array_equal(_np(inst.gt_boxes.tensor), boxes)
    # eval mode is passed through untouched
    model.training = False
    marker = [{"image": "anything"}]
    assert model.forward(marker) == {"n": 1} and model.seen[-1] is marker
