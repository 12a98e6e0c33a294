"""GPU: the evaluation-form results of native inference (csrc/seg_infer.hip: seg_labels_kernel, seg_labels_resize_kernel,
seg_confusion_kernel, seg_rle_*) against the default route of the same inputs: label maps against argmax of "sem_seg", the
confusion matrix against numpy's bincount, run-length masks against the dense "pred_masks".

Shapes: the _coco_inputs recipe of test_infer_gpu.py scaled down to low-res (50, 76), padded (200, 304), image (197, 301) and an
odd output that is no multiple of any tile; Q = 100 and 37 (not a multiple of the 32-query staging round); K = 19, 150 and 200
(a second 192-class chunk), and for the "before" labels also 40 and 80 (the 64- and 96-class tiles)."""
import dataclasses

import numpy as np
import pytest
import torch

from test_infer_cpu import load_infer
from test_infer_eval_cpu import rle_decode, rle_encode
from test_infer_gpu import _coco_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LOW, PADDED, IMAGE, OUT = (50, 76), (200, 304), (197, 301), (97, 131)


def _cfg(K, Q=100, **kw):
    from mp_former_amd.inference import InferenceConfig
    return InferenceConfig(num_classes=K, num_queries=Q, **kw)


def _np(t):
    return t.detach().cpu().numpy()


def _inputs(K, Q, dtype, seed=0):
    logits, masks = _coco_inputs(K, Q=Q, hw=LOW, seed=seed, strong=min(20, Q))
    return logits.to(DEV), masks.to(DEV).to(dtype)


def _semantic_pair(lg, mk, image, padded, out, **kw):
    """(sem_seg of the default route, labels of the labels route) of image 0, as numpy."""
    from mp_former_amd.inference import postprocess
    K = lg.shape[-1] - 1
    base = dict(semantic_on=True, instance_on=False, **kw)
    dense = postprocess(lg, mk, [image], padded, [out], _cfg(K, lg.shape[1], **base))[0]
    lab = postprocess(lg, mk, [image], padded, [out], _cfg(K, lg.shape[1], semantic_labels=True, **base))[0]
    assert "sem_seg" not in lab and "sem_seg_labels" not in dense
    t = lab["sem_seg_labels"]
    assert t.dtype == torch.int32 and t.is_cuda and tuple(t.shape) == tuple(out)
    return _np(dense["sem_seg"]), _np(t)


def _assert_inside_the_band(labels, sem, tag):
    """labels may differ from argmax(sem) only where sem's top-two gap is <= 2 * (1e-5 + 1e-5 * top1), on <= 0.5 % of the pixels."""
    ref = sem.argmax(0)
    top2 = np.partition(sem, -2, axis=0)[-2:]
    top1, second = top2[1], top2[0]
    band = (top1 - second) <= 2 * (1e-5 + 1e-5 * top1)
    diff = labels != ref
    print(f"{tag}: {int(diff.sum())} of {diff.size} pixels differ, {100 * band.mean():.3f} % of the pixels are in the band")
    assert not (diff & ~band).any(), f"{tag}: {int((diff & ~band).sum())} pixels differ outside the tie band"
    assert diff.mean() <= 0.005, f"{tag}: {100 * diff.mean():.3f} % of the pixels differ"


# ---- 1. labels, "before" mode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Q", [100, 37])
@pytest.mark.parametrize("K", [19, 40, 80, 150, 200])
def test_labels_before_mode_equal_the_argmax_of_the_scores(K, Q, dtype):
    lg, mk = _inputs(K, Q, dtype)
    sem, lab = _semantic_pair(lg, mk, IMAGE, PADDED, OUT)
    assert lab.min() >= 0 and lab.max() < K
    np.testing.assert_array_equal(lab, sem.argmax(0))


def test_labels_tie_goes_to_the_lower_class():
    K, Q = 150, 37
    lg, mk = _inputs(K, Q, torch.float32, seed=1)
    lg[..., 140] = lg[..., 7]                         # two identical columns: identical probabilities, identical scores
    lg[..., 7] += 4.0                                  # ... and they win often
    lg[..., 140] += 4.0
    sem, lab = _semantic_pair(lg, mk, IMAGE, PADDED, OUT)
    np.testing.assert_array_equal(sem[7], sem[140])
    assert (sem.argmax(0) == 7).mean() > 0.2, "the tie should decide a good part of the image"
    assert not (lab == 140).any()
    np.testing.assert_array_equal(lab, sem.argmax(0))


@pytest.mark.parametrize("variant", ["f32", "bf16"])
def test_labels_of_the_infer_all_fixture(variant):
    from mp_former_amd.inference import postprocess
    z, cfg, padded = load_infer("infer_all")
    lg = torch.from_numpy(z["pred_logits"]).to(DEV)
    mk = torch.from_numpy(z["pred_masks"]).to(DEV) if variant == "f32" else torch.from_numpy(z["pred_masks_bf16"]).to(DEV).to(torch.bfloat16)
    dense = postprocess(lg, mk, z["image_sizes"], padded, z["output_sizes"], cfg)
    lab = postprocess(lg, mk, z["image_sizes"], padded, z["output_sizes"], dataclasses.replace(cfg, semantic_labels=True))
    for n in range(len(dense)):
        np.testing.assert_array_equal(_np(lab[n]["sem_seg_labels"]), _np(dense[n]["sem_seg"]).argmax(0))
        assert torch.equal(lab[n]["panoptic_seg"][0], dense[n]["panoptic_seg"][0])        # the other routes are untouched
        assert torch.equal(lab[n]["instances"].pred_masks, dense[n]["instances"].pred_masks)


# ---- 2. labels, "after" mode ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,Q", [(19, 100), (150, 37), (200, 100)])
def test_labels_after_mode_without_resize_are_exact(K, Q, dtype):
    lg, mk = _inputs(K, Q, dtype)
    sem, lab = _semantic_pair(lg, mk, IMAGE, PADDED, IMAGE, sem_seg_postprocess_before_inference=False)
    np.testing.assert_array_equal(lab, sem.argmax(0))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,Q,out", [(19, 100, (120, 181)), (150, 37, (120, 181)), (200, 100, OUT), (19, 37, (211, 340))])
def test_labels_after_mode_with_resize_stay_in_the_tie_band(K, Q, out, dtype):
    lg, mk = _inputs(K, Q, dtype)
    sem, lab = _semantic_pair(lg, mk, IMAGE, PADDED, out, sem_seg_postprocess_before_inference=False)
    _assert_inside_the_band(lab, sem, f"K{K}/Q{Q}/{out}")


@pytest.mark.parametrize("variant", ["f32", "bf16"])
def test_labels_of_the_infer_semantic_fixture(variant):
    """The reference's own "after"-mode sem_seg (golden): labels inside its tie band."""
    from mp_former_amd.inference import postprocess
    z, cfg, padded = load_infer("infer_semantic")
    assert not cfg.sem_seg_postprocess_before_inference
    lg = torch.from_numpy(z["pred_logits"]).to(DEV)
    mk = torch.from_numpy(z["pred_masks"]).to(DEV) if variant == "f32" else torch.from_numpy(z["pred_masks_bf16"]).to(DEV).to(torch.bfloat16)
    lab = postprocess(lg, mk, z["image_sizes"], padded, z["output_sizes"], dataclasses.replace(cfg, semantic_labels=True))
    for n in range(len(lab)):
        assert "sem_seg" not in lab[n]
        _assert_inside_the_band(_np(lab[n]["sem_seg_labels"]), z[f"{variant}_{n}_sem_seg"], f"infer_semantic/{variant}/{n}")


# ---- 3. confusion matrix --------------------------------------------------------------------------------------------------------
def _bincount(pred, gt, K, ignore):
    g = gt.astype(np.int64).copy()
    g[(g == ignore) | (g < 0) | (g >= K)] = K
    p = pred.astype(np.int64).copy()
    p[(p < 0) | (p >= K)] = K
    return np.bincount((K + 1) * p.ravel() + g.ravel(), minlength=(K + 1) ** 2).reshape(K + 1, K + 1)


def _label_pair(K, hw, seed, gt_dtype):
    """A blocky prediction and a ground truth that mostly agrees with it, with ignore pixels, a value >= K and a negative one."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.randint(0, K, (1, 1, hw[0] // 8 + 1, hw[1] // 8 + 1), generator=g).float()
    pred = torch.nn.functional.interpolate(coarse, size=hw, mode="nearest")[0, 0].to(torch.int32)
    gt = pred.clone().to(torch.int64)
    flip = torch.rand(hw, generator=g) < 0.2
    gt[flip] = torch.randint(0, K, (int(flip.sum()),), generator=g)
    gt[torch.rand(hw, generator=g) < 0.1] = 255
    gt[0, 0], gt[0, 1] = K, K + 7
    if gt_dtype.is_signed:
        gt[1, 0] = -1
    return pred, gt.to(gt_dtype)


@pytest.mark.parametrize("K", [19, 150, 200])
def test_confusion_matrix_equals_bincount(K):
    """K = 19 / 150: the LDS histogram; K = 200: (K+1)^2 counters do not fit, global integer atomics.  n = 97 * 131 and 61 * 83 are no
    multiple of the 8-pixel runs or of the workgroup."""
    from mp_former_amd.inference import SemSegConfusion
    ignore = 255
    conf = SemSegConfusion(K, ignore_label=ignore, device=DEV)
    p1, g1 = _label_pair(K, OUT, 1, torch.int64)
    p2, g2 = _label_pair(K, (61, 83), 2, torch.uint8 if K < 200 else torch.int16)
    assert (_np(g1) == ignore).any() and (_np(g1) >= K).any() and (_np(g1) < 0).any()
    d1, d2 = (p1.to(DEV), g1.to(DEV)), (p2.to(DEV), g2.to(DEV))
    conf.update(*d1)                                  # warm: the counters are allocated
    conf.reset()
    assert not conf.matrix().any()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        conf.update(*d1)
        conf.update(*d2)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    want1, want2 = _bincount(_np(p1), _np(g1), K, ignore), _bincount(_np(p2), _np(g2), K, ignore)
    m = conf.matrix()
    assert m.dtype == np.int64 and m.shape == (K + 1, K + 1)
    np.testing.assert_array_equal(m, want1 + want2)   # accumulated over two updates
    assert m[:, K].sum() > 0 and m.sum() == p1.numel() + p2.numel()
    conf.reset()
    conf.update(*d2)
    np.testing.assert_array_equal(conf.matrix(), want2)
    with pytest.raises(ValueError):
        conf.update(d1[0], d2[1])
    # a prediction outside [0, K) is counted in row K, never used as an index
    bad = d2[0].clone()
    bad[0, :3] = torch.tensor([-5, K, 1 << 30], dtype=torch.int32, device=DEV)
    conf.reset()
    conf.update(bad, d2[1])
    np.testing.assert_array_equal(conf.matrix(), _bincount(_np(bad), _np(g2), K, ignore))
    assert conf.matrix()[K].sum() == 3
    r = conf.results()
    assert 0.0 <= r["mIoU"] <= 100.0 and 0.0 <= r["pACC"] <= 100.0


def test_confusion_of_the_labels_route():
    """End to end: labels of the native route into the counters, against numpy on the default route's argmax."""
    from mp_former_amd.inference import SemSegConfusion, confusion_results
    K = 19
    lg, mk = _inputs(K, 37, torch.float32, seed=4)
    sem, lab = _semantic_pair(lg, mk, IMAGE, PADDED, OUT)
    _, gt = _label_pair(K, OUT, 9, torch.uint8)
    from mp_former_amd.inference import postprocess
    t = postprocess(lg, mk, [IMAGE], PADDED, [OUT], _cfg(K, 37, semantic_on=True, instance_on=False, semantic_labels=True))[0]["sem_seg_labels"]
    conf = SemSegConfusion(K, device=DEV)
    conf.update(t, gt.to(DEV))
    want = _bincount(sem.argmax(0), _np(gt), K, 255)
    np.testing.assert_array_equal(conf.matrix(), want)
    assert conf.results() == pytest.approx(confusion_results(want), nan_ok=True)


# ---- 4. run-length masks --------------------------------------------------------------------------------------------------------
def _instance_pair(lg, mk, image, padded, out, **kw):
    from mp_former_amd.inference import postprocess
    K, Q = lg.shape[-1] - 1, lg.shape[1]
    dense = postprocess(lg, mk, [image], padded, [out], _cfg(K, Q, **kw))[0]["instances"]
    rle = postprocess(lg, mk, [image], padded, [out], _cfg(K, Q, instance_masks="rle", **kw))[0]["instances"]
    return dense, rle


def _assert_rle_equals_dense(dense, rle, out, tag=""):
    assert not rle.has("pred_masks") and not dense.has("pred_masks_rle")
    assert torch.equal(rle.scores, dense.scores) and torch.equal(rle.pred_classes, dense.pred_classes), tag
    masks = _np(dense.pred_masks) > 0.5
    got = rle.pred_masks_rle
    assert isinstance(got, list) and len(got) == masks.shape[0] == len(rle), tag
    for t, r in enumerate(got):
        assert r["size"] == list(out) and all(type(c) is int for c in r["counts"]), tag
        np.testing.assert_array_equal(rle_decode(r), masks[t], err_msg=f"{tag} instance {t}")   # (also: sum == H * W, positive runs)
        assert r == rle_encode(masks[t]), f"{tag} instance {t}"
    return masks, got


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("K,Q", [(19, 100), (150, 37)])
def test_rle_masks_equal_the_dense_masks(K, Q, dtype):
    lg, mk = _inputs(K, Q, dtype)
    dense, rle = _instance_pair(lg, mk, IMAGE, PADDED, OUT)
    masks, _ = _assert_rle_equals_dense(dense, rle, OUT, f"K{K}/Q{Q}")
    assert len(rle) == min(100, Q * K) and 0.05 < masks.mean() < 0.95
    _, again = _instance_pair(lg, mk, IMAGE, PADDED, OUT)
    assert again.pred_masks_rle == rle.pred_masks_rle            # two runs are identical


@pytest.mark.parametrize("name", ["infer_instance", "infer_all"])
def test_rle_masks_of_the_fixtures(name):
    from mp_former_amd.inference import postprocess
    z, cfg, padded = load_infer(name)
    lg, mk = torch.from_numpy(z["pred_logits"]).to(DEV), torch.from_numpy(z["pred_masks"]).to(DEV)
    dense = postprocess(lg, mk, z["image_sizes"], padded, z["output_sizes"], cfg)
    rle = postprocess(lg, mk, z["image_sizes"], padded, z["output_sizes"], dataclasses.replace(cfg, instance_masks="rle"))
    for n in range(len(dense)):
        _assert_rle_equals_dense(dense[n]["instances"], rle[n]["instances"], tuple(int(v) for v in z["output_sizes"][n]), f"{name}/{n}")


def _all_pairs_inputs(masks):
    """Q queries, K = 3, top-k = every (query, class) pair: every query is among the instances."""
    Q = masks.shape[0]
    g = torch.Generator().manual_seed(Q)
    return torch.randn(1, Q, 4, generator=g).to(DEV), masks[None].to(DEV), dict(test_topk_per_image=3 * Q)


@pytest.mark.parametrize("out", [OUT, (1, 131), (97, 1), (1, 1)], ids=lambda o: f"{o[0]}x{o[1]}")
def test_rle_constructed_empty_full_and_thin_outputs(out):
    g = torch.Generator().manual_seed(11)
    masks = torch.randn(5, *LOW, generator=g) * 4
    masks[1] = -5.0                                     # nowhere on
    masks[3] = 5.0                                      # everywhere on
    lg, mk, kw = _all_pairs_inputs(masks)
    dense, rle = _instance_pair(lg, mk, IMAGE, PADDED, out, **kw)
    assert len(rle) == 15
    _assert_rle_equals_dense(dense, rle, out, str(out))
    counts = [r["counts"] for r in rle.pred_masks_rle]
    hw = out[0] * out[1]
    assert counts.count([hw]) >= 3 and counts.count([0, hw]) >= 3    # (a 1-pixel output has no other form)


@pytest.mark.parametrize("hw", [(100, 170), (128, 128), (113, 145)], ids=lambda o: f"{o[0]}x{o[1]}")
def test_rle_runs_across_column_word_and_tile_boundaries(hw):
    """Identity geometry (low-res = padded = image = output), so the masks are painted directly.  A tile of the run-length kernels is
    256 words of 64 positions = 16384 positions: 128 x 128 is exactly one tile, 113 x 145 = 16385 is one tile + 1, and in
    100 x 170 the run 16350 .. 16419 crosses the tile boundary (16384) and the column boundary (16400) in one piece.  In the two
    smaller shapes the same run is cut off by the end of the mask."""
    H, W = hw
    g = torch.Generator().manual_seed(H)
    masks = torch.randn(4, H, W, generator=g)
    flat = torch.full((H * W,), -1.0)
    flat[16350:16420] = 1.0
    flat[-1] = 1.0                                      # the last position on: a run that ends with the mask
    flat[:3] = 1.0                                      # the first position on: counts start with 0
    masks[0] = flat.view(W, H).t()                      # column-major positions
    masks[1] = -masks[0]
    lg, mk, kw = _all_pairs_inputs(masks)
    dense, rle = _instance_pair(lg, mk, hw, hw, hw, **kw)
    _, got = _assert_rle_equals_dense(dense, rle, hw, str(hw))
    counts = [r["counts"] for r in got]
    want0, want1 = rle_encode(masks[0].numpy() > 0)["counts"], rle_encode(masks[1].numpy() > 0)["counts"]
    if hw == (100, 170):
        assert want0 == [0, 3, 16347, 70, 17000 - 16421, 1] and want1 == want0[1:]
    elif hw == (128, 128):
        assert want0 == [0, 3, 16347, 34]                 # the run ends with the tile and the mask
    else:
        assert want0 == [0, 3, 16347, 35]                 # ... or one position into the second tile
    assert counts.count(want0) == 3 and counts.count(want1) == 3, (want0, [c for c in counts if len(c) < 8])


def test_rle_with_no_instance_kept():
    from mp_former_amd.inference import postprocess
    lg, mk = _inputs(19, 37, torch.float32)
    cfg = _cfg(19, 37, panoptic_on=True, instance_masks="rle", thing_ids=frozenset())       # no thing class: nothing is kept
    ins = postprocess(lg, mk, [IMAGE], PADDED, [OUT], cfg)[0]["instances"]
    assert ins.pred_masks_rle == [] and not ins.has("pred_masks") and ins.scores.numel() == 0 and ins.pred_classes.numel() == 0


# ---- 5. memory ------------------------------------------------------------------------------------------------------------------
COCO = dict(padded=(800, 1216), image=[(800, 1199)], out=[(480, 719)])


def _peak(fn):
    fn()                                                # warm: the scratch buffers are allocated
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated() - base
    del r
    return p


def test_memory_of_the_labels_route():
    from mp_former_amd.inference import postprocess
    logits, masks = _coco_inputs(133, seed=7)
    lg, mk = logits.to(DEV), masks.to(DEV)
    kw = dict(semantic_on=True, instance_on=False)
    scores = _peak(lambda: postprocess(lg, mk, COCO["image"], COCO["padded"], COCO["out"], _cfg(133, **kw)))
    labels = _peak(lambda: postprocess(lg, mk, COCO["image"], COCO["padded"], COCO["out"], _cfg(133, semantic_labels=True, **kw)))
    print(f"peak increase: labels {labels / 2**20:.2f} MiB, scores {scores / 2**20:.2f} MiB")
    assert labels <= scores / 16, (labels, scores)


def test_memory_of_the_rle_route():
    from mp_former_amd.inference import postprocess
    logits, masks = _coco_inputs(80, seed=7)
    lg, mk = logits.to(DEV), masks.to(DEV)
    H, W = COCO["out"][0]
    d = postprocess(lg, mk, COCO["image"], COCO["padded"], COCO["out"], _cfg(80))[0]["instances"].pred_masks
    flat = d.transpose(1, 2).reshape(d.shape[0], -1)    # column-major positions
    runs = 1 + (flat[:, 1:] != flat[:, :-1]).sum(1).float()
    del d, flat
    assert float(runs.mean()) <= H * W / 16, f"the input masks average {float(runs.mean()):.0f} runs, more than H * W / 16"
    dense = _peak(lambda: postprocess(lg, mk, COCO["image"], COCO["padded"], COCO["out"], _cfg(80)))
    rle = _peak(lambda: postprocess(lg, mk, COCO["image"], COCO["padded"], COCO["out"], _cfg(80, instance_masks="rle")))
    print(f"peak increase: rle {rle / 2**20:.2f} MiB, dense {dense / 2**20:.2f} MiB, {float(runs.mean()):.0f} runs per mask")
    assert rle <= dense / 4, (rle, dense)


# ---- 6. route -------------------------------------------------------------------------------------------------------------------
def test_kernels_on_the_route():
    from mp_former_amd import _lib
    from mp_former_amd.inference import SemSegConfusion, postprocess
    K, Q = 19, 37
    lg, mk = _inputs(K, Q, torch.float32)
    _, gt = _label_pair(K, OUT, 3, torch.uint8)
    conf = SemSegConfusion(K, device=DEV)

    def counts(cfg):
        _lib.profile_enable(True)
        try:
            r = postprocess(lg, mk, [IMAGE], PADDED, [OUT], cfg)[0]
            if "sem_seg_labels" in r:
                conf.update(r["sem_seg_labels"], gt.to(DEV))
            torch.cuda.synchronize()
            return {k: _lib.profile_get(k)[0] for k in ("seg_semantic_kernel", "seg_labels_kernel", "seg_labels_resize_kernel",
                                                        "seg_confusion_kernel", "seg_instance_kernel", "seg_instance_scores",
                                                        "seg_rle_bits_kernel", "seg_rle_scatter_kernel")}
        finally:
            _lib.profile_enable(False)

    before = counts(_cfg(K, Q, semantic_on=True, instance_on=False, semantic_labels=True))
    assert before["seg_labels_kernel"] == 1 and before["seg_confusion_kernel"] == 1
    assert before["seg_semantic_kernel"] == 0 and before["seg_labels_resize_kernel"] == 0
    after = counts(_cfg(K, Q, semantic_on=True, instance_on=False, semantic_labels=True, sem_seg_postprocess_before_inference=False))
    assert after["seg_labels_resize_kernel"] == 1 and after["seg_semantic_kernel"] == 1 and after["seg_labels_kernel"] == 0
    rle = counts(_cfg(K, Q, instance_masks="rle"))
    assert rle["seg_rle_bits_kernel"] == 1 and rle["seg_rle_scatter_kernel"] == 1 and rle["seg_instance_scores"] == 1
    assert rle["seg_instance_kernel"] == 0, "the dense-mask pass ran under instance_masks='rle'"
    dense = counts(_cfg(K, Q))
    assert dense["seg_instance_kernel"] == 1 and dense["seg_rle_bits_kernel"] == 0
    assert _lib.last_kernel() == "seg_instance_kernel"


def test_head_inference_passes_the_options_through():
    """MPFormerHead.inference with both options == postprocess of the predictor's own outputs (head_small, eval mode)."""
    from conftest import load_head_fixture
    from mp_former_amd.head import MPFormerHead
    from mp_former_amd.inference import InferenceConfig, postprocess
    z, c, pp, dp, feats, targets, _ = load_head_fixture("head_small")
    h = MPFormerHead(num_classes=c["num_classes"], num_queries=c["num_queries"], enc_layers=c["enc_layers"],
                     dec_layers=c["dec_layers"], num_points=c["num_points"], factored_masks=False)
    h.pixel_decoder.load_state_dict(pp)
    h.predictor.load_state_dict(dp)
    h = h.to(DEV).eval()
    gfeats = {k: v.to(DEV) for k, v in feats.items()}
    N = next(iter(gfeats.values())).shape[0]
    with torch.no_grad():
        mf, _, ms = h.pixel_decoder.forward_features(gfeats)
        eval_out = h.predictor(ms, mf, None, None)
    hw = mf.shape[-2:]
    padded = (hw[0] * 4, hw[1] * 4)
    sizes = [(padded[0] - 3 * n, padded[1] - 5 * n) for n in range(N)]
    outs = [(s[0] + 7, s[1] - 2) for s in sizes]
    K = c["num_classes"]
    cfg = InferenceConfig(num_classes=K, num_queries=c["num_queries"], semantic_on=True, semantic_labels=True, instance_masks="rle")
    got = h.inference(gfeats, sizes, padded, outs, cfg)
    want = postprocess(eval_out["pred_logits"], eval_out["pred_masks"], sizes, padded, outs, cfg)
    dense = postprocess(eval_out["pred_logits"], eval_out["pred_masks"], sizes, padded, outs,
                        InferenceConfig(num_classes=K, num_queries=c["num_queries"], semantic_on=True))
    assert len(got) == N
    for a, b, d, out in zip(got, want, dense, outs):
        assert set(a) == {"sem_seg_labels", "instances"}
        assert torch.equal(a["sem_seg_labels"], b["sem_seg_labels"]) and tuple(a["sem_seg_labels"].shape) == out
        assert a["instances"].pred_masks_rle == b["instances"].pred_masks_rle
        assert torch.equal(a["instances"].scores, b["instances"].scores)
        np.testing.assert_array_equal(_np(a["sem_seg_labels"]), _np(d["sem_seg"]).argmax(0))
        _assert_rle_equals_dense(d["instances"], a["instances"], out, "head_small")
