"""GPU: semantic test-time augmentation (csrc/seg_infer.hip: seg_tta_accumulate_kernel, seg_tta_resize_add_kernel,
seg_tta_finish_kernel via mp_former_amd.inference.SemanticTTA) against the reference's four lines
(mask2former/test_time_augmentation.py:83-97)

    sem_seg = (sum over the views of flip_v(S_v)) / V

written here on an fp64 restatement of the per-view "sem_seg" (logits and masks widened to double, F.interpolate bilinear,
align_corners=False), and against ``postprocess`` of the same inputs.

Shapes: three view geometries (low-res, padded, image), each added plain and flipped = 6 views, every geometry with its own seed;
outputs (97, 131) (odd, H * W no multiple of 4: the per-pixel epilogue), (96, 132) (the float4 epilogue, also mirrored) and
(96, 131) (float4 for the plain views, per pixel for the mirrored ones);
(K, Q) = (19, 100), (150, 37) (Q no multiple of 4 or 32), (200, 100) (a second chunk of 192 classes), (5, 3) (Q below one MFMA k-step,
K below one 16-row tile), (40, 37) and (80, 37) (the 64- and 96-class tiles of the VALU kernels, 4 and 8 MFMA row tiles); fp32 and
bf16 masks; both config modes.

The bound rtol = atol = 1e-5 is the project's bound for "sem_seg" (tests/test_infer_gpu.py).  It follows from the formats too: an fp32
dot product of Q non-negative terms is off by at most about Q * 2^-24 relative in any order (6e-6 at Q = 100), the sum over the views
adds V * 2^-24, the sigmoid and resample roundings stay below 1e-6."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_infer_eval_gpu import _assert_inside_the_band
from test_infer_gpu import _coco_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RTOL = ATOL = 1e-5
GEOMS = {"A": ((50, 76), (200, 304), (197, 301)), "B": ((32, 48), (128, 192), (123, 189)), "C": ((72, 104), (288, 416), (281, 412))}
VIEWS = [("A", False), ("A", True), ("B", False), ("B", True), ("C", False), ("C", True)]
OUT_ODD, OUT_VEC = (97, 131), (96, 132)
OUT_MIXED = (96, 131)         # H * W a multiple of 4, W not: plain views take the float4 epilogue, mirrored ones the per-pixel one
KQ = [(19, 100), (150, 37), (200, 100), (5, 3), (40, 37), (80, 37)]
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
MODES = {"before": True, "after": False}


def _cfg(K, Q, before, **kw):
    from mp_former_amd.inference import InferenceConfig
    return InferenceConfig(num_classes=K, num_queries=Q, semantic_on=True, instance_on=False, sem_seg_postprocess_before_inference=before,
                           **kw)


@functools.lru_cache(maxsize=None)
def _view_inputs(K, Q, dtype, name, tie=False):
    """(pred_logits [1, Q, K+1] fp32, pred_masks [1, Q, h, w] dtype) of one geometry, on the device; never modified."""
    low = GEOMS[name][0]
    logits, masks = _coco_inputs(K, Q=Q, hw=low, seed=11 + "ABC".index(name), strong=min(20, Q))
    if tie:                                                 # as test_labels_tie_goes_to_the_lower_class builds them
        logits[..., 140] = logits[..., 7]
        logits[..., 7] += 4.0
        logits[..., 140] += 4.0
    return logits.to(DEV), masks.to(DEV).to(DTYPES[dtype])


def _resize(x, size):
    return F.interpolate(x[None], size=tuple(size), mode="bilinear", align_corners=False)[0]


def _sem_seg64(logits, masks, image, padded, out, before):
    """The reference's "sem_seg" of one view in fp64 (maskformer_model.py:236-279, :301-306)."""
    m = _resize(masks.double(), padded)[:, :image[0], :image[1]]
    prob = logits.double().softmax(-1)[:, :-1]
    if before:
        return torch.einsum("qc,qhw->chw", prob, _resize(m, out).sigmoid())
    return _resize(torch.einsum("qc,qhw->chw", prob, m.sigmoid()), out)


@functools.lru_cache(maxsize=None)
def _reference(K, Q, dtype, mode, out, nviews=6):
    """fp64: the four lines of the reference over the first nviews views -> numpy [K, H, W]; computed once per case."""
    final = None
    for name, hflip in VIEWS[:nviews]:
        lg, mk = _view_inputs(K, Q, dtype, name)
        _, padded, image = GEOMS[name]
        s = _sem_seg64(lg[0], mk[0], image, padded, out, MODES[mode])
        s = s.flip(-1) if hflip else s
        final = s if final is None else final + s
    return (final / nviews).cpu().numpy()


def _run(K, Q, dtype, mode, out, views=VIEWS, tta=None, tie=False, **kw):
    from mp_former_amd.inference import SemanticTTA
    tta = tta or SemanticTTA(_cfg(K, Q, MODES[mode], **kw))
    for name, hflip in views:
        lg, mk = _view_inputs(K, Q, dtype, name, tie)
        _, padded, image = GEOMS[name]
        tta.add(lg, mk, image, padded, out, hflip)
    return tta.result()


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. parity with the fp64 restatement, both modes ---------------------------------------------------------------------------
@pytest.mark.parametrize("out", [OUT_ODD, OUT_VEC], ids=["97x131", "96x132"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("K,Q", KQ)
def test_parity_with_the_fp64_reference(K, Q, dtype, mode, out):
    res = _run(K, Q, dtype, mode, out)
    assert set(res) == {"sem_seg"}
    got = res["sem_seg"]
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (K, *out)
    want = _reference(K, Q, dtype, mode, out)
    err = np.abs(_np(got) - want) / (ATOL + RTOL * np.abs(want))
    print(f"K{K}/Q{Q}/{dtype}/{mode}/{out}: largest error {err.max():.3f} of the bound")
    np.testing.assert_allclose(_np(got), want, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("K,Q", [(19, 100), (150, 37)])
def test_both_epilogues_into_one_accumulator(K, Q, mode):
    """Output (96, 131): the plain views store and add through the float4 form, the mirrored views pixel by pixel, alternating, into
    the same accumulator.  Same reference, same bound; the labels are the argmax of the dense result."""
    got = _np(_run(K, Q, "f32", mode, OUT_MIXED)["sem_seg"])
    np.testing.assert_allclose(got, _reference(K, Q, "f32", mode, OUT_MIXED), rtol=RTOL, atol=ATOL)
    lab = _run(K, Q, "f32", mode, OUT_MIXED, semantic_labels=True)["sem_seg_labels"]
    np.testing.assert_array_equal(_np(lab), got.argmax(0))


# ---- 2. the flip is on the output -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", [OUT_ODD, OUT_VEC], ids=["97x131", "96x132"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("K,Q", [(19, 100), (150, 37)])
def test_one_flipped_view_is_the_mirrored_postprocess_result(K, Q, mode, out):
    from mp_former_amd.inference import postprocess
    lg, mk = _view_inputs(K, Q, "f32", "A")
    _, padded, image = GEOMS["A"]
    want = postprocess(lg, mk, [image], padded, [out], _cfg(K, Q, MODES[mode]))[0]["sem_seg"]
    assert not torch.equal(want, want.flip(-1)), "the inputs must not be mirror-symmetric"
    got = _run(K, Q, "f32", mode, out, views=[("A", True)])["sem_seg"]
    print(f"K{K}/Q{Q}/{mode}/{out}: mirrored view bitwise equal to postprocess().flip(-1): {torch.equal(got, want.flip(-1))}")
    np.testing.assert_allclose(_np(got), _np(want.flip(-1)), rtol=RTOL, atol=ATOL)
    assert not np.allclose(_np(got), _np(want), rtol=RTOL, atol=ATOL), "a flipped view came out unmirrored"


# ---- 3. store mode against seg_semantic_kernel -------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", [OUT_ODD, OUT_VEC], ids=["97x131", "96x132"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("K,Q", KQ)
def test_store_mode_against_the_valu_kernel(K, Q, dtype, out):
    """One plain view, "before" mode: the MFMA product against seg_semantic_kernel's fmaf chain.  The bound is required; whether the
    two are bitwise equal (the fp32 MFMA is documented as a k-ordered fmaf chain) is printed, and recorded in DESIGN 9.2."""
    from mp_former_amd.inference import postprocess
    lg, mk = _view_inputs(K, Q, dtype, "A")
    _, padded, image = GEOMS["A"]
    want = postprocess(lg, mk, [image], padded, [out], _cfg(K, Q, True))[0]["sem_seg"]
    got = _run(K, Q, dtype, "before", out, views=[("A", False)])["sem_seg"]
    diff = (got != want)
    print(f"K{K}/Q{Q}/{dtype}/{out}: bitwise equal to seg_semantic_kernel: {not bool(diff.any())} ({int(diff.sum())} of {diff.numel()} differ)")
    np.testing.assert_allclose(_np(got), _np(want), rtol=RTOL, atol=ATOL)


# ---- 4. labels --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", [OUT_ODD, OUT_VEC], ids=["97x131", "96x132"])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("K,Q", KQ)
def test_labels_equal_the_argmax_of_the_dense_result(K, Q, mode, out):
    dense = _np(_run(K, Q, "f32", mode, out)["sem_seg"])
    res = _run(K, Q, "f32", mode, out, semantic_labels=True)
    assert set(res) == {"sem_seg_labels"}
    lab = res["sem_seg_labels"]
    assert lab.dtype == torch.int32 and lab.is_cuda and tuple(lab.shape) == out
    np.testing.assert_array_equal(_np(lab), dense.argmax(0))
    _assert_inside_the_band(_np(lab), _reference(K, Q, "f32", mode, out), f"K{K}/Q{Q}/{mode}/{out} against fp64")


@pytest.mark.parametrize("mode", list(MODES))
def test_labels_tie_goes_to_the_lower_class(mode):
    K, Q = 150, 37
    dense = _np(_run(K, Q, "f32", mode, OUT_ODD, tie=True)["sem_seg"])
    lab = _np(_run(K, Q, "f32", mode, OUT_ODD, tie=True, semantic_labels=True)["sem_seg_labels"])
    np.testing.assert_array_equal(dense[7], dense[140])
    assert (dense.argmax(0) == 7).mean() > 0.2, "the tie should decide a good part of the image"
    assert not (lab == 140).any()
    np.testing.assert_array_equal(lab, dense.argmax(0))


# ---- 5. count and order -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(MODES))
def test_five_views_reruns_and_reuse_of_one_object(mode):
    from mp_former_amd.inference import SemanticTTA
    K, Q = 19, 100
    five = VIEWS[:5]
    a = _run(K, Q, "f32", mode, OUT_ODD, views=five)["sem_seg"]
    np.testing.assert_allclose(_np(a), _reference(K, Q, "f32", mode, OUT_ODD, 5), rtol=RTOL, atol=ATOL)     # an odd divisor
    b = _run(K, Q, "f32", mode, OUT_ODD, views=five)["sem_seg"]
    assert torch.equal(a, b), "the same views in the same order must give the same bits"
    fresh = _run(K, Q, "f32", mode, OUT_ODD, views=[("B", True)])["sem_seg"]
    tta = SemanticTTA(_cfg(K, Q, MODES[mode]))
    _run(K, Q, "f32", mode, OUT_ODD, views=five, tta=tta)                              # result() leaves it ready for the next image
    assert torch.equal(_run(K, Q, "f32", mode, OUT_ODD, views=[("B", True)], tta=tta)["sem_seg"], fresh)
    lg, mk = _view_inputs(K, Q, "f32", "A")
    tta.add(lg, mk, GEOMS["A"][2], GEOMS["A"][1], OUT_ODD, False)
    with pytest.raises(ValueError, match="output size"):
        tta.add(lg, mk, GEOMS["A"][2], GEOMS["A"][1], OUT_VEC, False)
    tta.reset()                                                                         # ... and so does reset()
    assert torch.equal(_run(K, Q, "f32", mode, OUT_ODD, views=[("B", True)], tta=tta)["sem_seg"], fresh)
    with pytest.raises(RuntimeError, match="no view"):
        tta.result()
    with pytest.raises(TypeError):
        tta.add(lg, mk.half(), GEOMS["A"][2], GEOMS["A"][1], OUT_ODD, False)


# ---- 6. no sync, no hidden copies, the route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [False, True], ids=["dense", "labels"])
@pytest.mark.parametrize("mode", list(MODES))
def test_no_host_sync(mode, labels):
    K, Q = 150, 37
    _run(K, Q, "f32", mode, OUT_ODD, semantic_labels=labels)                           # warm: inputs cached, scratch allocated
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        _run(K, Q, "f32", mode, OUT_ODD, semantic_labels=labels)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_memory_of_the_labels_route():
    """"before" mode with labels: the accumulator is native scratch, and no view makes a [K, H, W] temporary."""
    K, Q = 150, 37
    run = lambda: _run(K, Q, "f32", "before", OUT_ODD, semantic_labels=True)
    run()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    khw = K * OUT_ODD[0] * OUT_ODD[1] * 4
    print(f"peak increase {peak / 2**20:.2f} MiB, K * H * W * 4 B = {khw / 2**20:.2f} MiB")
    assert peak < 1.5 * khw, (peak, khw)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("K,Q", [(19, 100), (150, 37)])
def test_kernels_on_the_route(K, Q, mode):
    from mp_former_amd import _lib
    _lib.profile_enable(True)
    try:
        _run(K, Q, "f32", mode, OUT_ODD)
        torch.cuda.synchronize()
        n = {k: _lib.profile_get(k)[0] for k in ("seg_tta_accumulate_kernel", "seg_tta_resize_add_kernel", "seg_tta_finish_kernel",
                                                 "seg_semantic_kernel", "seg_labels")}
    finally:
        _lib.profile_enable(False)
    assert n["seg_tta_accumulate_kernel"] >= 6 and n["seg_semantic_kernel"] == 0 and n["seg_labels"] == 0, n
    assert n["seg_tta_finish_kernel"] == 1, n
    assert n["seg_tta_resize_add_kernel"] >= 6 if mode == "after" else n["seg_tta_resize_add_kernel"] == 0, n
    assert _lib.last_kernel() == "seg_tta_finish_kernel"


# ---- 7. the wrapper ---------------------------------------------------------------------------------------------------------------
class ImageList:
    """detectron2.structures.ImageList.from_tensors: pad to the largest image, rounded up to size_divisibility."""

    def __init__(self, tensor, image_sizes):
        self.tensor, self.image_sizes = tensor, image_sizes

    @staticmethod
    def from_tensors(tensors, size_divisibility=0, pad_value=0.0):
        sizes = [(int(t.shape[-2]), int(t.shape[-1])) for t in tensors]
        d = max(int(size_divisibility), 1)
        hmax, wmax = ((max(s[i] for s in sizes) + d - 1) // d * d for i in (0, 1))
        out = tensors[0].new_full((len(tensors), tensors[0].shape[0], hmax, wmax), pad_value)
        for i, t in enumerate(tensors):
            out[i, :, :t.shape[-2], :t.shape[-1]].copy_(t)
        return ImageList(out, sizes)


class HFlipTransform:
    """Stands in for fvcore.transforms.HFlipTransform (matched by class name where fvcore is absent)."""


class ResizeTransform:
    pass


class _StubHead:
    """Fixed random predictions sized from the input: [1, Q, K+1] logits and [1, Q, Hp / 4, Wp / 4] mask logits."""

    def __init__(self, K, Q):
        self.num_classes, self.Q = K, Q

    def __call__(self, x):
        hp, wp = int(x.shape[-2]), int(x.shape[-1])
        logits, masks = _coco_inputs(self.num_classes, Q=self.Q, hw=(hp // 4, wp // 4), seed=hp * 7 + wp, strong=10)
        return {"pred_logits": logits.to(DEV), "pred_masks": masks.to(DEV)}


def _stub_model(K, Q, before):
    return SimpleNamespace(device=DEV, pixel_mean=torch.tensor([120.0, 115.0, 100.0], device=DEV).view(3, 1, 1),
                           pixel_std=torch.tensor([58.0, 57.0, 57.0], device=DEV).view(3, 1, 1), size_divisibility=32,
                           backbone=lambda x: x, sem_seg_head=_StubHead(K, Q), num_queries=Q, object_mask_threshold=0.8,
                           overlap_threshold=0.8, test_topk_per_image=100, semantic_on=True, instance_on=False, panoptic_on=False,
                           sem_seg_postprocess_before_inference=before, metadata=None, input_format="RGB")


def _stub_mapper(inp):
    try:
        from fvcore.transforms import HFlipTransform as Flip
        flip = Flip(1)
    except ImportError:
        flip = HFlipTransform()
    views = []
    for size in ((90, 150), (123, 189), (160, 250)):
        img = F.interpolate(inp["image"][None].float(), size=size, mode="bilinear", align_corners=False)[0]
        for tfms in ([ResizeTransform()], [ResizeTransform(), flip]):
            views.append({"image": img.flip(-1) if len(tfms) == 2 else img, "transforms": SimpleNamespace(transforms=tfms),
                          "height": inp["height"], "width": inp["width"]})
    return views


@pytest.mark.parametrize("before", [False, True], ids=["after", "before"])
def test_wrapper_equals_the_per_view_route(before):
    from mp_former_amd import d2_plugin
    from mp_former_amd.inference import InferenceConfig
    K, Q = 19, 37
    model = _stub_model(K, Q, before)
    g = torch.Generator().manual_seed(3)
    inputs = [{"image": torch.rand(3, 120, 180, generator=g) * 255, "height": 97, "width": 131},
              {"image": torch.rand(3, 100, 160, generator=g) * 255}]
    seg = d2_plugin.SemanticSegmentorWithTTAHIP(None, model, _stub_mapper, image_list_cls=ImageList)
    got = seg(inputs)
    assert len(got) == 2 and tuple(got[0]["sem_seg"].shape) == (K, 97, 131) and tuple(got[1]["sem_seg"].shape) == (K, 100, 160)
    cfg = InferenceConfig.from_maskformer(model)
    for inp, res in zip(inputs, got):
        full = dict(inp, height=inp.get("height", inp["image"].shape[1]), width=inp.get("width", inp["image"].shape[2]))
        views = _stub_mapper(full)
        assert len(views) == 6
        total = None
        for v in views:
            s = d2_plugin.native_eval_forward(model, [v], cfg, ImageList)[0]["sem_seg"]
            s = s.flip(-1) if d2_plugin.is_hflip(v["transforms"]) else s
            total = s.clone() if total is None else total + s
        np.testing.assert_allclose(_np(res["sem_seg"]), _np(total / len(views)), rtol=RTOL, atol=ATOL)
    lab = d2_plugin.SemanticSegmentorWithTTAHIP(None, model, _stub_mapper, image_list_cls=ImageList, semantic_labels=True)(inputs)
    for a, b in zip(lab, got):
        assert set(a) == {"sem_seg_labels"}
        np.testing.assert_array_equal(_np(a["sem_seg_labels"]), _np(b["sem_seg"]).argmax(0))


def test_head_inference_tta():
    """MPFormerHead.inference_tta == SemanticTTA over the predictor's own per-view outputs (head_small, eval mode)."""
    from conftest import load_head_fixture
    from mp_former_amd.head import MPFormerHead
    from mp_former_amd.inference import InferenceConfig, SemanticTTA
    z, c, pp, dp, feats, targets, _ = load_head_fixture("head_small")
    h = MPFormerHead(num_classes=c["num_classes"], num_queries=c["num_queries"], enc_layers=c["enc_layers"],
                     dec_layers=c["dec_layers"], num_points=c["num_points"], factored_masks=False)
    h.pixel_decoder.load_state_dict(pp)
    h.predictor.load_state_dict(dp)
    h = h.to(DEV).eval()
    N = next(iter(feats.values())).shape[0]
    per_view = [{k: v[n:n + 1].to(DEV) for k, v in feats.items()} for n in range(N)]
    cfg = InferenceConfig(num_classes=c["num_classes"], num_queries=c["num_queries"], semantic_on=True, instance_on=False,
                          sem_seg_postprocess_before_inference=False)
    out = (61, 83)
    tta = SemanticTTA(cfg)
    views = []
    with torch.no_grad():
        for n, f in enumerate(per_view):
            mf, _, ms = h.pixel_decoder.forward_features(f)
            o = h.predictor(ms, mf, None, None)
            padded = (mf.shape[-2] * 4, mf.shape[-1] * 4)
            image = (padded[0] - 3 * n, padded[1] - 5 * n)
            views.append((f, image, padded, n % 2 == 1))
            tta.add(o["pred_logits"], o["pred_masks"], image, padded, out, n % 2 == 1)
        want = tta.result()["sem_seg"]
        got = h.inference_tta(views, out, cfg)
    assert set(got) == {"sem_seg"} and tuple(got["sem_seg"].shape) == (c["num_classes"], *out)
    assert torch.equal(got["sem_seg"], want)
    lab = h.inference_tta(views, out, dataclasses.replace(cfg, semantic_labels=True))["sem_seg_labels"]
    np.testing.assert_array_equal(_np(lab), _np(want).argmax(0))
