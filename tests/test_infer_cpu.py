"""CPU: inference post-processing (mp_former_amd/inference.py, csrc/seg_infer.hip) without a GPU — the bilinear index rule
of the kernels against F.interpolate, the host segment table and the torch restatement against the reference's own eval
branch (tests/golden/infer_*.npz), and argument checks of the new C entry points."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from _infer_restate import restate

INFER_FIXTURES = ["infer_instance", "infer_all", "infer_semantic"]


def load_infer(name):
    from mp_former_amd.inference import InferenceConfig
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    c = json.loads(str(z["config"]))
    c.pop("size_divisibility")
    d = 8
    hp = max(s[0] for s in z["image_sizes"])
    wp = max(s[1] for s in z["image_sizes"])
    padded = ((hp + d - 1) // d * d, (wp + d - 1) // d * d)
    cfg = InferenceConfig(**{**c, "thing_ids": frozenset(c["thing_ids"])})
    return z, cfg, padded


def taps(n_in, n_out):
    """The kernels' index rule (seg_infer.hip tap()): fp32 scale = in / out, src = max(scale * (dst + 0.5) - 0.5, 0),
    i0 = trunc(src), i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1 — every step rounded to fp32."""
    f = np.float32
    scale = f(n_in) / f(n_out)
    dst = np.arange(n_out, dtype=np.float32)
    src = np.maximum((scale * (dst + f(0.5))).astype(f) - f(0.5), f(0)).astype(f)
    i0 = src.astype(np.int64)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(f)).astype(f)
    return i0, i1, (f(1) - l1).astype(f), l1


def resample_np(x, out_hw):
    """[h, w] fp32 -> [H, W] with taps() and torch's weight order h0 * (w0 * x00 + w1 * x01) + h1 * (w0 * x10 + w1 * x11)."""
    y0, y1, hy0, hy1 = taps(x.shape[0], out_hw[0])
    x0, x1, wx0, wx1 = taps(x.shape[1], out_hw[1])
    f = np.float32
    r0 = (wx0[None] * x[y0][:, x0]).astype(f) + (wx1[None] * x[y0][:, x1]).astype(f)
    r1 = (wx0[None] * x[y1][:, x0]).astype(f) + (wx1[None] * x[y1][:, x1]).astype(f)
    return ((hy0[:, None] * r0).astype(f) + (hy1[:, None] * r1).astype(f)).astype(f)


@pytest.mark.parametrize("shape", [((10, 14), (40, 56)), ((40, 56), (29, 41)), ((37, 50), (37, 50)), ((13, 17), (61, 83)),
                                   ((200, 304), (800, 1216)), ((800, 1199), (480, 719)), ((7, 9), (3, 5)), ((1, 1), (4, 3))])
def test_bilinear_index_rule_matches_interpolate(shape):
    (h, w), out = shape
    g = torch.Generator().manual_seed(h * 1000 + w)
    x = torch.randn(h, w, generator=g) * 4
    ref = F.interpolate(x[None, None], size=out, mode="bilinear", align_corners=False)[0, 0].numpy()
    got = resample_np(x.numpy(), out)
    # same indices and weights: agreement to fp32 rounding of the weighted sum (the CPU kernel may fuse the products)
    np.testing.assert_allclose(got, ref, rtol=0, atol=4e-6 * max(1.0, float(np.abs(ref).max())))
    i0, i1, l0, l1 = taps(h, out[0])
    assert i0.min() >= 0 and i1.max() <= h - 1 and (l0 >= 0).all() and (l1 >= 0).all() and (l1 < 1).all()


def _ref_masks(z, key, n):
    return z[key][n] if key in z else None


@pytest.mark.parametrize("name", INFER_FIXTURES)
@pytest.mark.parametrize("variant", ["f32", "bf16"])
def test_restatement_reproduces_the_reference(name, variant):
    z, cfg, padded = load_infer(name)
    masks = torch.from_numpy(z["pred_masks" if variant == "f32" else "pred_masks_bf16"])
    res = restate(torch.from_numpy(z["pred_logits"]), masks, z["image_sizes"], padded, z["output_sizes"], cfg)
    for n, r in enumerate(res):
        p = f"{variant}_{n}_"
        if cfg.semantic_on:
            np.testing.assert_allclose(r["sem_seg"].numpy(), z[p + "sem_seg"], rtol=1e-5, atol=1e-6)
        if cfg.panoptic_on:
            ids, info = r["panoptic_seg"]
            np.testing.assert_array_equal(ids.numpy(), z[p + "pan_ids"])
            assert [[s["id"], int(s["isthing"]), s["category_id"]] for s in info] == z[p + "pan_segments"].tolist()
        if cfg.instance_on:
            ins = r["instances"]
            ref_order = np.lexsort((-z[p + "inst_scores"], z[p + "inst_classes"]))
            got_order = np.lexsort((-ins["scores"].numpy(), ins["pred_classes"].numpy()))
            np.testing.assert_array_equal(ins["pred_classes"].numpy()[got_order], z[p + "inst_classes"][ref_order])
            np.testing.assert_allclose(ins["scores"].numpy()[got_order], z[p + "inst_scores"][ref_order], rtol=1e-5)
            np.testing.assert_array_equal(ins["pred_masks"].numpy()[got_order].astype(np.uint8), z[p + "inst_masks"][ref_order])


def test_segment_table_from_the_counters():
    """The host half of panoptic inference on the per-query areas reproduces the reference's segments_info — and the fixture
    covers the engineered cases: a stuff merge, an overlap rejection, a no-object query, an image with nothing kept."""
    from mp_former_amd.inference import segment_table
    z, cfg, padded = load_infer("infer_all")
    res = restate(torch.from_numpy(z["pred_logits"]), torch.from_numpy(z["pred_masks"]), z["image_sizes"], padded, z["output_sizes"],
                  cfg, keep_margins=True)
    labels, ma, oa, inter = res[0]["areas"]
    lut, info = segment_table(labels, ma, oa, inter, cfg.thing_ids, cfg.overlap_threshold)
    assert [[s["id"], int(s["isthing"]), s["category_id"]] for s in info] == z["f32_0_pan_segments"].tolist()
    stuff = [k for k, c in enumerate(labels) if c not in cfg.thing_ids and lut[k]]
    assert any(lut[a] == lut[b] for a in stuff for b in stuff if a < b), "no stuff merge"
    assert any(lut[k] == 0 and ma[k] > 0 and oa[k] > 0 and inter[k] > 0 for k in range(len(labels))), "no overlap rejection"
    prob = torch.from_numpy(z["pred_logits"][0]).softmax(-1)
    assert (prob.argmax(-1) == cfg.num_classes).any(), "no no-object query"
    assert res[1]["panoptic_seg"][1] == [] and z["f32_1_pan_ids"].max() == 0, "image 1 should keep nothing"
    assert res[1]["areas"] == ([], [], [], [])


def test_config_rules():
    from mp_former_amd.inference import InferenceConfig
    with pytest.raises(ValueError):
        InferenceConfig(num_classes=3, semantic_on=False, instance_on=True, sem_seg_postprocess_before_inference=False)
    with pytest.raises(ValueError):
        InferenceConfig(num_classes=3, semantic_on=True, instance_on=True, sem_seg_postprocess_before_inference=False)


def test_postprocess_rejects_cpu_tensors():
    from mp_former_amd.inference import InferenceConfig, postprocess
    cfg = InferenceConfig(num_classes=3)
    with pytest.raises(RuntimeError, match="CPU"):
        postprocess(torch.zeros(1, 4, 4), torch.zeros(1, 4, 5, 5), [(8, 8)], (8, 8), [(8, 8)], cfg)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib.lib()


def test_seg_entry_points_reject_bad_arguments(lib):
    one = ctypes.c_void_p(16)       # never dereferenced: the checks come first
    geom = [10, 14, 40, 56, 37, 50, 29, 41]
    assert lib.mpf_seg_semantic(one, 140, 99, 4, *geom, one, 3, one, None) == -1 and b"dtype" in lib.mpf_last_error()
    assert lib.mpf_seg_semantic(None, 140, 0, 4, *geom, one, 3, one, None) == -3
    assert lib.mpf_seg_semantic(one, 140, 0, 4, *geom, one, 0, one, None) == -2
    assert lib.mpf_seg_semantic(one, 100, 0, 4, *geom, one, 3, one, None) == -2                       # stride_q < h * w
    assert lib.mpf_seg_semantic(one, 140, 0, 4, 10, 14, 40, 56, 41, 50, 29, 41, one, 3, one, None) == -2   # image > padded
    assert lib.mpf_seg_softmax(one, 0, 4, 0.8, one, one, one, one, one, None) == -2
    assert lib.mpf_seg_softmax(one, 2000, 4, 0.8, one, one, one, one, one, None) == -2
    assert lib.mpf_seg_softmax(one, 4, 4, 0.8, None, one, one, one, one, None) == -3
    assert lib.mpf_seg_instance_workspace_bytes(3, 29, 41) == 3 * 2 * 8
    assert lib.mpf_seg_instance_scores(one, 140, 0, 4, *geom, one, one, 3, one, one, 8, None) == -2 and b"workspace" in lib.mpf_last_error()
    assert lib.mpf_seg_instance_scores(one, 140, 0, 4, *geom, None, one, 3, one, one, 48, None) == -3
    assert lib.mpf_seg_instance_masks(one, 140, 2, 4, *geom, one, 0, one, None) == -2
    assert lib.mpf_seg_panoptic_areas(one, 140, 0, 2000, *geom, one, one, one, one, None) == -2
    assert lib.mpf_seg_panoptic_areas(one, 140, 0, 4, *geom, one, None, one, one, None) == -3
    assert lib.mpf_seg_panoptic_paint(one, 0, 4, one, one, None) == -2
    assert lib.mpf_seg_panoptic_paint(one, 4, 4, None, one, None) == -3
