"""GPU: native inference post-processing (csrc/seg_infer.hip via mp_former_amd.inference.postprocess) against the reference's
eval branch (tests/golden/infer_*.npz) and against the torch restatement at COCO / Cityscapes sizes.

Pixels may differ only inside the tie band: where the restatement's final-resolution logit is within 2e-5 of 0 (the "> 0" and
"sigmoid >= 0.5" decisions), or where the panoptic winner leads the runner-up by <= 1e-6."""
import numpy as np
import pytest
import torch

from _infer_restate import restate
from test_infer_cpu import INFER_FIXTURES, load_infer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BAND = 2e-5


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def compare(got, want, margins, cfg, tag=""):
    """got: postprocess output of one image; want: {"sem_seg", "pan_ids", "pan_segments", "inst_*"} numpy; margins: restate(...,
    keep_margins=True) of the same image."""
    if cfg.semantic_on:
        np.testing.assert_allclose(_np(got["sem_seg"]), want["sem_seg"], rtol=1e-5, atol=1e-5, err_msg=tag)
    logit = _np(margins["logits"]) if "logits" in margins else None
    if cfg.panoptic_on:
        ids, info = got["panoptic_seg"]
        assert [[s["id"], int(s["isthing"]), s["category_id"]] for s in info] == want["pan_segments"], tag
        band = _np(margins["pan_gap"]) <= 1e-6
        labels = margins["areas"][0]
        if labels:
            prob = margins["kept_logits"]
            band |= (np.abs(prob) <= BAND).any(0)
        bad = (_np(ids) != want["pan_ids"]) & ~band
        assert not bad.any(), f"{tag}: {int(bad.sum())} panoptic pixels differ outside the tie band"
    if cfg.instance_on:
        ins = got["instances"]
        cls_g, sc_g, m_g = _np(ins.pred_classes), _np(ins.scores), _np(ins.pred_masks)
        og = np.lexsort((-sc_g, cls_g))
        ow = np.lexsort((-want["inst_scores"], want["inst_classes"]))
        np.testing.assert_array_equal(cls_g[og], want["inst_classes"][ow], err_msg=tag)
        np.testing.assert_allclose(sc_g[og], want["inst_scores"][ow], rtol=1e-5, atol=1e-7, err_msg=tag)
        q = want["inst_query"][ow]
        for j in range(len(og)):
            bad = (m_g[og[j]] != want["inst_masks"][ow[j]]) & (np.abs(logit[q[j]]) > BAND)
            assert not bad.any(), f"{tag}: instance {j}: {int(bad.sum())} mask pixels differ outside the tie band"


def _want_from_restate(r, cfg):
    w = {}
    if cfg.semantic_on:
        w["sem_seg"] = _np(r["sem_seg"])
    if cfg.panoptic_on:
        ids, info = r["panoptic_seg"]
        w["pan_ids"] = _np(ids)
        w["pan_segments"] = [[s["id"], int(s["isthing"]), s["category_id"]] for s in info]
    if cfg.instance_on:
        i = r["instances"]
        w.update(inst_masks=_np(i["pred_masks"]), inst_scores=_np(i["scores"]), inst_classes=_np(i["pred_classes"]),
                 inst_query=_np(i["query"]))
    return w


def _margins(logits, masks, image_sizes, padded, output_sizes, cfg):
    res = restate(logits, masks, image_sizes, padded, output_sizes, cfg, keep_margins=True)
    for n, r in enumerate(res):
        if cfg.panoptic_on and r["areas"][0]:
            prob = logits[n].float().softmax(-1)
            score, label = prob.max(-1)
            kept = torch.nonzero((label != cfg.num_classes) & (score > cfg.object_mask_threshold)).flatten()
            r["kept_logits"] = _np(r["logits"][kept])
    return res


@pytest.mark.parametrize("name", INFER_FIXTURES)
@pytest.mark.parametrize("variant", ["f32", "bf16"])
def test_fixture_parity(name, variant):
    from mp_former_amd.inference import postprocess
    z, cfg, padded = load_infer(name)
    logits = torch.from_numpy(z["pred_logits"])
    masks = torch.from_numpy(z["pred_masks" if variant == "f32" else "pred_masks_bf16"])
    marg = _margins(logits, masks, z["image_sizes"], padded, z["output_sizes"], cfg)
    dm = masks.to(DEV) if variant == "f32" else masks.to(DEV).to(torch.bfloat16)
    got = postprocess(logits.to(DEV), dm, z["image_sizes"], padded, z["output_sizes"], cfg)
    for n in range(len(got)):
        p = f"{variant}_{n}_"
        want = {k[len(p):]: z[k] for k in z if k.startswith(p)}
        if "pan_segments" in want:
            want["pan_segments"] = want["pan_segments"].tolist()
        if cfg.instance_on:
            # the reference's entries carry no query index: the restatement's (it reproduces the reference, test_infer_cpu)
            ri = marg[n]["instances"]
            o1 = np.lexsort((-_np(ri["scores"]), _np(ri["pred_classes"])))
            o2 = np.lexsort((-want["inst_scores"], want["inst_classes"]))
            q = np.empty_like(_np(ri["query"]))
            q[o2] = _np(ri["query"])[o1]
            want["inst_query"] = q
        compare(got[n], want, marg[n], cfg, f"{name}/{variant}/{n}")


def _coco_inputs(K, Q=100, hw=(200, 304), N=1, seed=0, strong=20):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(N, Q, K + 1, generator=g)
    for n in range(N):                       # a score above the panoptic threshold for some queries
        qs = torch.randperm(Q, generator=g)[:strong]
        logits[n, qs, torch.randint(0, K, (strong,), generator=g)] = 9.0
    low = torch.randn(N, Q, hw[0] // 8, hw[1] // 8, generator=g) * 4
    masks = torch.nn.functional.interpolate(low, size=hw, mode="bilinear", align_corners=False) + 0.3 * torch.randn(N, Q, *hw, generator=g)
    return logits, masks


def _cfg(K, **kw):
    from mp_former_amd.inference import InferenceConfig
    return InferenceConfig(num_classes=K, num_queries=100, **kw)


COCO = dict(padded=(800, 1216), image=[(800, 1199)], out=[(480, 719)])


@pytest.mark.parametrize("case", ["instance_k80", "all_k133", "cityscapes_semantic"])
def test_large_parity_against_restatement(case):
    from mp_former_amd.inference import postprocess
    if case == "instance_k80":
        K, cfg, geo, hw = 80, _cfg(80), COCO, (200, 304)
    elif case == "all_k133":
        K, cfg, geo, hw = 133, _cfg(133, semantic_on=True, panoptic_on=True, thing_ids=frozenset(range(80))), COCO, (200, 304)
    else:
        K, hw = 19, (256, 512)
        cfg = _cfg(19, semantic_on=True, instance_on=False, sem_seg_postprocess_before_inference=False)
        geo = dict(padded=(1024, 2048), image=[(1024, 2048)], out=[(1024, 2048)])
    logits, masks = _coco_inputs(K, hw=hw)
    lg, mk = logits.to(DEV), masks.to(DEV)
    got = postprocess(lg, mk, geo["image"], geo["padded"], geo["out"], cfg)
    marg = _margins(lg, mk, geo["image"], geo["padded"], geo["out"], cfg)
    compare(got[0], _want_from_restate(marg[0], cfg), marg[0], cfg, case)


def test_strided_input_slice_of_the_decoder_output():
    """pred_masks as the last layer's slice of an [N, L*Q, h, w] tensor: used in place, same results as a contiguous copy."""
    from mp_former_amd.inference import postprocess
    z, cfg, padded = load_infer("infer_all")
    masks = torch.from_numpy(z["pred_masks"]).to(DEV)
    N, Q = masks.shape[:2]
    big = torch.randn(N, 3 * Q, *masks.shape[2:], device=DEV)
    big[:, 2 * Q:] = masks
    sl = big[:, 2 * Q:]
    assert not sl.is_contiguous()
    lg = torch.from_numpy(z["pred_logits"]).to(DEV)
    a = postprocess(lg, sl, z["image_sizes"], padded, z["output_sizes"], cfg)
    b = postprocess(lg, masks, z["image_sizes"], padded, z["output_sizes"], cfg)
    _assert_bitwise(a, b)


def _assert_bitwise(a, b):
    for ra, rb in zip(a, b):
        if "sem_seg" in ra:
            assert torch.equal(ra["sem_seg"], rb["sem_seg"])
        if "panoptic_seg" in ra:
            assert torch.equal(ra["panoptic_seg"][0], rb["panoptic_seg"][0]) and ra["panoptic_seg"][1] == rb["panoptic_seg"][1]
        if "instances" in ra:
            ia, ib = ra["instances"], rb["instances"]
            assert torch.equal(ia.pred_masks, ib.pred_masks) and torch.equal(ia.scores, ib.scores)
            assert torch.equal(ia.pred_classes, ib.pred_classes)


def test_deterministic_and_kernel_names():
    from mp_former_amd import _lib
    from mp_former_amd.inference import postprocess
    logits, masks = _coco_inputs(133, seed=3)
    cfg = _cfg(133, semantic_on=True, panoptic_on=True, thing_ids=frozenset(range(80)))
    lg, mk = logits.to(DEV), masks.to(DEV)
    a = postprocess(lg, mk, COCO["image"], COCO["padded"], COCO["out"], cfg)
    assert _lib.last_kernel() == "seg_instance_kernel"
    b = postprocess(lg, mk, COCO["image"], COCO["padded"], COCO["out"], cfg)
    _assert_bitwise(a, b)
    _lib.profile_enable(True)
    try:
        postprocess(lg, mk, COCO["image"], COCO["padded"], COCO["out"], cfg)
        torch.cuda.synchronize()
        for k in ("seg_softmax_kernel", "seg_semantic_kernel", "seg_panoptic_kernel", "seg_paint_kernel", "seg_instance_scores",
                  "seg_instance_kernel"):
            assert _lib.profile_get(k)[0] >= 1, k
    finally:
        _lib.profile_enable(False)


@pytest.mark.parametrize("route", ["semantic", "instance"])
def test_no_host_sync(route):
    from mp_former_amd.inference import postprocess
    logits, masks = _coco_inputs(80 if route == "instance" else 133, seed=5)
    cfg = _cfg(80) if route == "instance" else _cfg(133, semantic_on=True, instance_on=False)
    lg, mk = logits.to(DEV), masks.to(DEV)
    postprocess(lg, mk, COCO["image"], COCO["padded"], COCO["out"], cfg)          # warm: scratch buffers allocated
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        postprocess(lg, mk, COCO["image"], COCO["padded"], COCO["out"], cfg)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


def test_memory_of_the_instance_route():
    from mp_former_amd.inference import postprocess
    logits, masks = _coco_inputs(80, seed=7)
    cfg = _cfg(80)
    lg, mk = logits.to(DEV), masks.to(DEV)

    def peak(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        r = fn()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        del r
        return p

    postprocess(lg, mk, COCO["image"], COCO["padded"], COCO["out"], cfg)
    native = peak(lambda: postprocess(lg, mk, COCO["image"], COCO["padded"], COCO["out"], cfg))
    torch_route = peak(lambda: restate(lg, mk, COCO["image"], COCO["padded"], COCO["out"], cfg))
    print(f"peak increase: native {native / 2**20:.1f} MiB, restatement {torch_route / 2**20:.1f} MiB")
    assert native <= torch_route / 4, (native, torch_route)


def test_head_inference_end_to_end():
    """MPFormerHead.inference in eval mode (dn_args=None) == postprocess of the predictor's own outputs, and its learnable-query
    predictions match a training-mode forward of the same weights with targets (the MP queries are isolated by tgt_mask)."""
    from conftest import load_head_fixture
    from mp_former_amd.head import MPFormerHead
    from mp_former_amd.inference import postprocess
    z, c, pp, dp, feats, targets, _ = load_head_fixture("head_small")
    h = MPFormerHead(num_classes=c["num_classes"], num_queries=c["num_queries"], enc_layers=c["enc_layers"],
                     dec_layers=c["dec_layers"], num_points=c["num_points"], factored_masks=False)
    h.pixel_decoder.load_state_dict(pp)
    h.predictor.load_state_dict(dp)
    h = h.to(DEV)
    gfeats = {k: v.to(DEV) for k, v in feats.items()}
    gtargets = [{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in t.items()} for t in targets]
    N = next(iter(gfeats.values())).shape[0]
    with torch.no_grad():
        h.train()
        mf, _, ms = h.pixel_decoder.forward_features(gfeats)
        train_out = h.predictor(ms, mf, None, {"tgt": gtargets, "scalar": h.scalar, "noise_scale": h.noise_scale})
        h.eval()
        mf, _, ms = h.pixel_decoder.forward_features(gfeats)
        eval_out = h.predictor(ms, mf, None, None)
    for k, tol in (("pred_logits", 2e-3), ("pred_masks", 5e-3)):
        a, b = eval_out[k].float(), train_out[k].float()
        assert a.shape == b.shape, k
        assert (a - b).norm() <= tol * b.norm() + 1e-6, k
    hw = mf.shape[-2:]
    padded = (hw[0] * 4, hw[1] * 4)
    sizes = [(padded[0] - 3 * n, padded[1] - 5 * n) for n in range(N)]
    outs = [(s[0] + 7, s[1] - 2) for s in sizes]
    from mp_former_amd.inference import InferenceConfig
    cfg = InferenceConfig(num_classes=c["num_classes"], num_queries=c["num_queries"], semantic_on=True, panoptic_on=True,
                          object_mask_threshold=0.0, thing_ids=frozenset(range(c["num_classes"] // 2)))
    got = h.inference(gfeats, sizes, padded, outs, cfg)
    want = postprocess(eval_out["pred_logits"], eval_out["pred_masks"], sizes, padded, outs, cfg)
    _assert_bitwise(got, want)
    assert len(got) == N and got[0]["sem_seg"].shape == (c["num_classes"], *outs[0])
