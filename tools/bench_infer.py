"""Inference post-processing: native route (mp_former_amd.inference.postprocess) vs the torch restatement of the reference's
eval branch (tests/_infer_restate.py), per image on one GPU.  Prints one line per case: us per image, peak MB above the
inputs, the algorithmic bytes / FLOP of the native route and the fraction of the measured 6.3 TB/s copy rate or of the
157 TF fp32 peak it reaches (whichever bound applies).

    python tools/bench_infer.py [--iters 20] [--rows base,eval,tta,pq,ap,boundary]

The ``eval`` rows measure the evaluation-form results (``semantic_labels``, ``SemSegConfusion``, ``instance_masks="rle"``) against
the default route brought to the same end product: ``sem_seg`` + ``torch.argmax`` (+ ``.cpu()`` of the label map where the metric
is wanted), and the dense masks + ``.cpu()``.  These rows are wall-clock medians between two device synchronisations, because
their host copies and the host's list building are part of the product; peak MB above the inputs; bytes crossing to the host.

The ``tta`` rows (not in the default set) measure semantic test-time augmentation, 6 synthetic scales x {plain, flip} = 12 views per
image in "after" mode with low-res = padded / 4 and Q = 100: ``SemanticTTA`` (dense and labels) against what the package offered
before it, ``postprocess`` per view + ``flip`` + ``+=`` + one divide (+ ``argmax``).  One more line per case times
``seg_tta_accumulate_kernel`` in store mode against ``seg_semantic_kernel`` on the same single view.  Wall-clock medians as above.
The memory columns of these rows come from a call that starts without native scratch (``cold_memory``): the peak includes the scratch
the route allocates, and "held" is what stays allocated for the next image after the result is dropped.

The ``pq`` row (not in the default set; COCO panoptic case only) measures panoptic quality: ``postprocess`` with ``panoptic_on``
followed by ``PanopticQuality.update`` against ``postprocess``, ``ids.cpu()`` and the numpy restatement of panopticapi's per-image
arithmetic (tests/_pq_restate.py).  The ground truth is in place on both sides before the clock starts (RGB bytes on the device,
an id map on the host).  Wall-clock medians as above; the id map's 4 H W bytes cross to the host on the parent side only.

The ``ap`` row (not in the default set; COCO instance case only) measures the per-image part of instance mask AP: ``instance_bits``
+ ``pack_masks`` of the ground truth + ``InstanceAP.update`` against ``postprocess`` with dense masks, ``pred_masks.cpu()`` and the
numpy restatement of the COCO IoU and matching (tests/_ap_restate.py).  The ground truth (about 20 dense masks) is in place on
both sides before the clock starts.  Wall-clock medians as above; the 4 T H W bytes of the masks cross on the parent side only.

The ``boundary`` row (not in the default set; COCO instance case only; prints the ``ap`` row first, in the same run) measures
Boundary AP on the ``ap`` row's scene (d = 17 at 480 x 719): ``instance_bits`` + ``pack_masks`` + ``InstanceAP(iou_type="boundary")
.update`` against the only route there was before it: the dense masks to the host, ``scipy.ndimage.binary_erosion`` of every mask
and the numpy restatement (tests/_boundary_restate.py's min of the two IoUs in tests/_ap_restate.py).  Same protocol as ``ap``:
median of --iters, the host route's of --iters / 4, ground truth in place first.  ``added_over_ap_us`` is what the two boundary
launches and the second pair count cost on top of mask AP.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from _infer_restate import restate  # noqa: E402
from mp_former_amd import _lib  # noqa: E402
from mp_former_amd.inference import (InferenceConfig, InstanceAP, PanopticQuality, SemanticTTA, SemSegConfusion,  # noqa: E402
                                     boundary_dilation, instance_bits, mask_boundaries, mask_pair_counts, pack_masks, postprocess)

CASES = {
    # name: (K, low-res hw, padded, image, output, config)
    "coco_instance_k80": (80, (200, 304), (800, 1216), (800, 1199), (480, 719), dict()),
    "coco_panoptic_k133": (133, (200, 304), (800, 1216), (800, 1199), (480, 719),
                           dict(semantic_on=True, panoptic_on=True, thing_ids=frozenset(range(80)))),
    "ade20k_semantic_k150": (150, (160, 160), (640, 640), (640, 640), (640, 640),
                             dict(semantic_on=True, instance_on=False, sem_seg_postprocess_before_inference=False)),
    "cityscapes_semantic_k19": (19, (256, 512), (1024, 2048), (1024, 2048), (1024, 2048),
                                dict(semantic_on=True, instance_on=False, sem_seg_postprocess_before_inference=False)),
}


def inputs(K, hw, dev, Q=100, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(1, Q, K + 1, generator=g)
    logits[0, torch.randperm(Q, generator=g)[:20], torch.randint(0, K, (20,), generator=g)] = 9.0
    low = torch.randn(1, Q, hw[0] // 8, hw[1] // 8, generator=g) * 4
    masks = torch.nn.functional.interpolate(low, size=hw, mode="bilinear", align_corners=False)
    return logits.to(dev), masks.to(dev)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 1e6
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], peak


def timed_wall(fn, iters):
    """-> (median us between two synchronisations, peak MB above what was allocated before)"""
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 1e6
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return ts[len(ts) // 2], peak


def cold_memory(fn):
    """-> (peak MB, MB still held after the result is dropped) of one call that starts without native scratch: what the route
    costs a process, its persistent scratch included (timed_wall's baseline, taken after a warm call, leaves that out)."""
    _lib._scratch.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 1e6
    del r
    return peak, (torch.cuda.memory_allocated() - base) / 1e6


def eval_rows(name, K, hw, padded, image, out, iters, dev):
    """The evaluation-form rows of one case: labels in both modes, without and with the confusion counts, and rle masks."""
    lg, mk = inputs(K, hw, dev)
    H, W = out
    gt = torch.randint(0, K, out, dtype=torch.int64, device=dev)
    conf = SemSegConfusion(K, device=dev)
    rows = []

    def row(kind, native, parent, native_host_bytes, parent_host_bytes):
        t_nat, m_nat = timed_wall(native, iters)
        t_par, m_par = timed_wall(parent, iters)
        rows.append({"case": name, "row": kind, "native_us": round(t_nat, 1), "parent_us": round(t_par, 1), "speedup": round(t_par / t_nat, 2),
                     "native_peak_MB": round(m_nat, 1), "parent_peak_MB": round(m_par, 1), "native_host_bytes": int(native_host_bytes),
                     "parent_host_bytes": int(parent_host_bytes)})
        print(json.dumps(rows[-1]), flush=True)

    for before in (True, False):
        kw = dict(semantic_on=True, instance_on=False, sem_seg_postprocess_before_inference=before)
        c_lab = InferenceConfig(num_classes=K, num_queries=100, semantic_labels=True, **kw)
        c_par = InferenceConfig(num_classes=K, num_queries=100, **kw)
        mode = "before" if before else "after"

        def labels():
            return postprocess(lg, mk, [image], padded, [out], c_lab)[0]["sem_seg_labels"]

        def parent_labels():
            return postprocess(lg, mk, [image], padded, [out], c_par)[0]["sem_seg"].argmax(0)

        def labels_conf():
            conf.update(labels(), gt)

        def parent_conf():                               # the label map crosses; the host's bincount is not timed
            return parent_labels().cpu()

        row(f"labels_{mode}", labels, parent_labels, 0, 0)
        row(f"labels_{mode}+confusion", labels_conf, parent_conf, 0, 8 * H * W)
    c_rle = InferenceConfig(num_classes=K, num_queries=100, instance_masks="rle")
    c_dense = InferenceConfig(num_classes=K, num_queries=100)
    n_counts = []

    def rle():
        r = postprocess(lg, mk, [image], padded, [out], c_rle)[0]["instances"].pred_masks_rle
        n_counts.append(sum(len(x["counts"]) for x in r))
        return r

    def dense():
        return postprocess(lg, mk, [image], padded, [out], c_dense)[0]["instances"].pred_masks.cpu()

    rle()
    T = min(100, 100 * K)
    row("instance_rle", rle, dense, 8 * (T + 1) + 4 * n_counts[0], 4 * T * H * W)
    return rows


TTA_CASES = {"ade20k_semantic_k150": (150, (640, 640)), "cityscapes_semantic_k19": (19, (1024, 2048))}
TTA_SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)


def tta_rows(name, iters, dev, Q=100):
    """The test-time-augmentation rows of one case ("after" mode, the default of the semantic configs), and the single-view line
    of the two product kernels."""
    K, out = TTA_CASES[name]
    views = []
    for i, s in enumerate(TTA_SCALES):
        image = (int(out[0] * s), int(out[1] * s))
        padded = tuple((v + 31) // 32 * 32 for v in image)
        lg, mk = inputs(K, (padded[0] // 4, padded[1] // 4), dev, Q, seed=i)
        views += [(lg, mk, image, padded, False), (lg, mk, image, padded, True)]
    kw = dict(num_classes=K, num_queries=Q, semantic_on=True, instance_on=False, sem_seg_postprocess_before_inference=False)
    c_par = InferenceConfig(**kw)
    ttas = {False: SemanticTTA(c_par), True: SemanticTTA(InferenceConfig(semantic_labels=True, **kw))}

    def native(labels):
        t = ttas[labels]
        for lg, mk, image, padded, flip in views:
            t.add(lg, mk, image, padded, out, flip)
        return t.result()

    def parent(labels):
        final = None
        for lg, mk, image, padded, flip in views:
            s = postprocess(lg, mk, [image], padded, [out], c_par)[0]["sem_seg"]
            s = s.flip(-1) if flip else s
            if final is None:
                final = s
            else:
                final += s
        final = final / len(views)
        return final.argmax(0) if labels else final

    for labels in (False, True):
        (m_nat, held_nat), (m_par, held_par) = cold_memory(lambda: native(labels)), cold_memory(lambda: parent(labels))
        t_nat, _ = timed_wall(lambda: native(labels), iters)
        t_par, _ = timed_wall(lambda: parent(labels), iters)
        print(json.dumps({"case": name, "row": "tta_labels" if labels else "tta_dense", "views": len(views), "native_us": round(t_nat, 1),
                          "parent_us": round(t_par, 1), "speedup": round(t_par / t_nat, 2), "native_peak_MB": round(m_nat, 1),
                          "parent_peak_MB": round(m_par, 1), "native_held_MB": round(held_nat, 1),
                          "parent_held_MB": round(held_par, 1)}), flush=True)
    # one view (scale 1.0), scores on its own grid: the MFMA product in store mode against the VALU product
    lg, mk, image, padded, _ = views[4]
    stream = _lib.stream_ptr(dev)
    probs = lg[0].softmax(-1)[:, :K].contiguous()
    dst = torch.empty((K, *image), dtype=torch.float32, device=dev)
    geom = [Q, mk.shape[-2], mk.shape[-1], *padded, *image, *image]
    args = (mk.data_ptr(), mk.stride(1), _lib.MPF_F32, *geom, probs.data_ptr(), K)
    t_mfma, _ = timed_wall(lambda: _lib.call("mpf_seg_tta_accumulate", dev, *args, 0, dst.data_ptr(), stream), iters)
    a = dst.clone()
    t_valu, _ = timed_wall(lambda: _lib.call("mpf_seg_semantic", dev, *args, dst.data_ptr(), stream), iters)
    fl = 2.0 * K * Q * image[0] * image[1]
    print(json.dumps({"case": name, "row": "single_view_product", "seg_tta_accumulate_us": round(t_mfma, 1),
                      "seg_semantic_us": round(t_valu, 1), "speedup": round(t_valu / t_mfma, 2), "bitwise_equal": bool(torch.equal(a, dst)),
                      "alg_GFLOP": round(fl / 1e9, 2), "mfma_frac_157TF": round(fl / (t_mfma * 1e-6) / 157e12, 3),
                      "valu_frac_157TF": round(fl / (t_valu * 1e-6) / 157e12, 3)}), flush=True)


def pq_rows(name, K, hw, padded, image, out, iters, dev):
    """Panoptic quality of one image: the device route against the id map's copy to the host + the numpy restatement."""
    import numpy as np
    import _pq_restate as R
    things = frozenset(range(80))
    cfg = InferenceConfig(num_classes=K, num_queries=100, instance_on=False, panoptic_on=True, thing_ids=things)
    # 20 confident queries that each own one block of a 4 x 5 grid (the random masks of inputs() keep no segment at all)
    g = torch.Generator().manual_seed(0)
    Q = 100
    lg = torch.randn(1, Q, K + 1, generator=g)
    strong = torch.randperm(Q, generator=g)[:20]
    lg[0, strong, torch.randint(0, K, (20,), generator=g)] = 9.0
    low = torch.randn(1, Q, hw[0] // 8, hw[1] // 8, generator=g) - 6.0
    bh, bw = low.shape[-2] // 4, low.shape[-1] // 5
    for j, q in enumerate(strong.tolist()):
        low[0, q, j // 5 * bh:(j // 5 + 1) * bh, j % 5 * bw:(j % 5 + 1) * bw] += 14.0
    lg, mk = lg.to(dev), torch.nn.functional.interpolate(low, size=hw, mode="bilinear", align_corners=False).to(dev)
    H, W = out
    ids0, info0 = postprocess(lg, mk, [image], padded, [out], cfg)[0]["panoptic_seg"]
    assert len(info0) >= 10, f"the synthetic image keeps {len(info0)} segments"
    # ground truth: the predicted partition moved by (5, 9) pixels under panoptic-PNG ids, a VOID band, one crowd segment
    g = np.random.default_rng(0)
    new_id = np.concatenate(([0], np.sort(g.choice(np.arange(1, 1 << 24), size=len(info0), replace=False))))
    gt = new_id[np.roll(ids0.cpu().numpy().astype(np.int64), (5, 9), axis=(0, 1))]
    gt[:16] = 0
    gts = [{"id": int(new_id[s["id"]]), "category_id": s["category_id"], "iscrowd": int(n == 1)} for n, s in enumerate(info0)]
    gt_dev = torch.from_numpy(R.id2rgb(gt)).to(dev)
    pq = PanopticQuality(K, things, device=dev)
    host_total = [R.zero_stats(K)]

    def native():
        ids, info = postprocess(lg, mk, [image], padded, [out], cfg)[0]["panoptic_seg"]
        pq.update(ids, info, gt_dev, gts)

    def parent():
        ids, info = postprocess(lg, mk, [image], padded, [out], cfg)[0]["panoptic_seg"]
        host_total[0] = R.add_stats(host_total[0], R.pq_single(gt, ids.cpu().numpy(), gts, info, K, 0))

    def post_only():
        return postprocess(lg, mk, [image], padded, [out], cfg)[0]["panoptic_seg"]

    t_nat, m_nat = timed_wall(native, iters)
    t_par, m_par = timed_wall(parent, iters)
    t_post, _ = timed_wall(post_only, iters)
    t_upd, _ = timed_wall(lambda: pq.update(ids0, info0, gt_dev, gts), iters)
    pq.reset()
    pq.update(ids0, info0, gt_dev, gts)
    got, want = pq.stats(), R.pq_single(gt, ids0.cpu().numpy(), gts, info0, K, 0)
    same = all(np.array_equal(got[k], want[k]) for k in ("tp", "fp", "fn")) and got["iou"].tobytes() == want["iou"].tobytes()
    print(json.dumps({"case": name, "row": "pq", "segments": len(info0), "native_us": round(t_nat, 1), "parent_us": round(t_par, 1),
                      "speedup": round(t_par / t_nat, 2), "native_slower": bool(t_nat > t_par), "postprocess_us": round(t_post, 1),
                      "pq_update_us": round(t_upd, 1), "native_peak_MB": round(m_nat, 1), "parent_peak_MB": round(m_par, 1),
                      "native_host_bytes": 0, "parent_host_bytes": 4 * H * W, "equal_to_restatement": bool(same),
                      "tp_fp_fn": [int(want[k].sum()) for k in ("tp", "fp", "fn")]}), flush=True)


def ap_rows(name, K, hw, padded, image, out, iters, dev, n_gt=20, boundary=False):
    """Instance mask AP of one image: the device route against the dense masks' copy to the host + the numpy restatement.
    boundary: the Boundary AP row after it, on the same scene."""
    import numpy as np
    import _ap_restate as R
    cfg = InferenceConfig(num_classes=K, num_queries=100)
    lg, mk = inputs(K, hw, dev)
    H, W = out
    ins = postprocess(lg, mk, [image], padded, [out], cfg)[0]["instances"]
    T = len(ins)
    # ground truth: the first n_gt predictions moved by (5, 9) pixels (every third stays in place), their classes, one crowd
    pm = ins.pred_masks[:n_gt] > 0.5
    gt_dev = torch.stack([m if j % 3 == 0 else torch.roll(m, (5, 9), (0, 1)) for j, m in enumerate(pm)]).to(torch.uint8)
    gt_cls = ins.pred_classes[:n_gt].clone()
    crowd = torch.zeros(n_gt, dtype=torch.int32, device=dev)
    crowd[1] = 1
    gt_host, cls_host, crowd_host = gt_dev.cpu().numpy().astype(bool), gt_cls.cpu().tolist(), crowd.cpu().tolist()
    gts = [{"id": j + 1, "category": int(cls_host[j]), "iscrowd": int(crowd_host[j]), "mask": gt_host[j], "area": float(gt_host[j].sum())}
           for j in range(n_gt)]
    ap = InstanceAP(K, device=dev)

    def native():
        b = instance_bits(lg, mk, [image], padded, [out], cfg)[0]
        ap.update(b["bits"], b["scores"], b["pred_classes"], pack_masks(gt_dev), gt_cls, crowd)

    def host_dets(i):
        masks, sc, cl = i.pred_masks.cpu().numpy() > 0.5, i.scores.cpu().numpy(), i.pred_classes.cpu().numpy()
        return [{"id": t + 1, "category": int(cl[t]), "score": float(sc[t]), "mask": masks[t], "area": float(masks[t].sum())}
                for t in range(len(sc))]

    def parent():
        i = postprocess(lg, mk, [image], padded, [out], cfg)[0]["instances"]
        return R.evaluate([(host_dets(i), gts)], K, R.COCO_AREA_RNGS, (1, 10, 100))

    def bits_only():
        return instance_bits(lg, mk, [image], padded, [out], cfg)

    b0 = instance_bits(lg, mk, [image], padded, [out], cfg)[0]
    g0 = pack_masks(gt_dev)
    t_nat, m_nat = timed_wall(native, iters)
    t_par, m_par = timed_wall(parent, max(3, iters // 4))
    t_bits, _ = timed_wall(bits_only, iters)
    t_pack, _ = timed_wall(lambda: pack_masks(gt_dev), iters)
    t_upd, _ = timed_wall(lambda: ap.update(b0["bits"], b0["scores"], b0["pred_classes"], g0, gt_cls, crowd), iters)
    ap.reset()
    native()
    got = ap.stats()
    dts = host_dets(ins)
    want = R.expected_stats([(dts, gts)], K, R.COCO_AREA_RNGS, (1, 10, 100))
    same = got["scores"].tobytes() == want["scores"].tobytes() and all(np.array_equal(got[k], want[k])
                                                                        for k in ("category", "rank", "matched", "ignored", "npig"))
    print(json.dumps({"case": name, "row": "ap", "detections": T, "ground_truths": n_gt, "native_us": round(t_nat, 1),
                      "parent_us": round(t_par, 1), "speedup": round(t_par / t_nat, 2), "native_slower": bool(t_nat > t_par),
                      "instance_bits_us": round(t_bits, 1), "pack_masks_us": round(t_pack, 1), "ap_update_us": round(t_upd, 1),
                      "native_peak_MB": round(m_nat, 1), "parent_peak_MB": round(m_par, 1), "native_host_bytes": 0,
                      "parent_host_bytes": 4 * T * H * W, "records_equal_to_restatement": bool(same),
                      "matched_at_0.5": int(want["matched"][:, 0, 0].sum())}), flush=True)
    if not boundary:
        return
    import _boundary_restate as B
    from scipy import ndimage
    d = boundary_dilation(H, W)
    bap = InstanceAP(K, device=dev, iou_type="boundary")

    def native_b():
        b = instance_bits(lg, mk, [image], padded, [out], cfg)[0]
        bap.update(b["bits"], b["scores"], b["pred_classes"], pack_masks(gt_dev), gt_cls, crowd, size=(H, W))

    def to_boundaries(items):
        box = np.ones((3, 3), dtype=bool)
        return [{**o, "mask": o["mask"] & ~ndimage.binary_erosion(o["mask"], box, iterations=d, border_value=0)} for o in items]

    def iou_min(dt, gt, max_det, crowd_rule):           # boundaries made once per image, outside: see parent_b
        return np.minimum(B._MASK_IOU(dt, gt, max_det, crowd_rule),
                          B._MASK_IOU([x["b"] for x in dt], [x["b"] for x in gt], max_det, crowd_rule)) if len(dt) or len(gt) else []

    gts_b = [{**g, "b": b} for g, b in zip(gts, to_boundaries(gts))]      # the ground truth's boundaries are in place too

    def parent_b():
        i = postprocess(lg, mk, [image], padded, [out], cfg)[0]["instances"]
        dts_h = host_dets(i)
        dts_b = [{**x, "b": b} for x, b in zip(dts_h, to_boundaries(dts_h))]
        R.compute_iou = iou_min
        try:
            return R.evaluate([(dts_b, gts_b)], K, R.COCO_AREA_RNGS, (1, 10, 100))
        finally:
            R.compute_iou = B._MASK_IOU

    t_natb, m_natb = timed_wall(native_b, iters)
    t_parb, m_parb = timed_wall(parent_b, max(3, iters // 4))
    t_bnd, _ = timed_wall(lambda: (mask_boundaries(b0["bits"], (H, W), d=d), mask_boundaries(g0, (H, W), d=d)), iters)
    bd, bg = mask_boundaries(b0["bits"], (H, W), d=d), mask_boundaries(g0, (H, W), d=d)
    t_cnt, _ = timed_wall(lambda: mask_pair_counts(bd, bg), iters)
    t_updb, _ = timed_wall(lambda: bap.update(b0["bits"], b0["scores"], b0["pred_classes"], g0, gt_cls, crowd, size=(H, W)), iters)
    bap.reset()
    native_b()
    got = bap.stats()
    want = R.expected_stats([(dts, gts)], K, R.COCO_AREA_RNGS, (1, 10, 100), eval_imgs=parent_b())
    same = got["scores"].tobytes() == want["scores"].tobytes() and all(np.array_equal(got[k], want[k])
                                                                        for k in ("category", "rank", "matched", "ignored", "npig"))
    print(json.dumps({"case": name, "row": "boundary", "detections": T, "ground_truths": n_gt, "d": d, "native_us": round(t_natb, 1),
                      "parent_us": round(t_parb, 1), "speedup": round(t_parb / t_natb, 2), "native_slower": bool(t_natb > t_parb),
                      "ap_row_native_us": round(t_nat, 1), "added_over_ap_us": round(t_natb - t_nat, 1),
                      "mask_boundaries_us": round(t_bnd, 1), "boundary_pair_counts_us": round(t_cnt, 1),
                      "boundary_update_us": round(t_updb, 1), "mask_update_us": round(t_upd, 1),
                      "native_peak_MB": round(m_natb, 1), "parent_peak_MB": round(m_parb, 1), "native_host_bytes": 0,
                      "parent_host_bytes": 4 * T * H * W, "records_equal_to_restatement": bool(same),
                      "matched_at_0.5": int(want["matched"][:, 0, 0].sum())}), flush=True)


def work(K, cfg, hw, out, Q=100, T=100):
    """(bytes, flop) the native route must move / compute: the logits once per kernel that reads them, the results once."""
    H, W = out
    lowres = Q * hw[0] * hw[1] * 4
    by, fl = 0.0, 0.0
    if cfg.semantic_on:
        by += lowres + K * H * W * 4
        fl += 2.0 * K * Q * H * W
    if cfg.panoptic_on:
        by += lowres + 2 * H * W * 4 * 2
    if cfg.instance_on:
        by += 2 * lowres + T * H * W * 4
    return by, fl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--rows", default="base,eval")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kinds = args.rows.split(",")
    for name in args.cases.split(","):
        K, hw, padded, image, out, kw = CASES[name]
        if "tta" in kinds and name in TTA_CASES:
            tta_rows(name, args.iters, dev)
        if "pq" in kinds and name == "coco_panoptic_k133":
            pq_rows(name, K, hw, padded, image, out, args.iters, dev)
        if ("ap" in kinds or "boundary" in kinds) and name == "coco_instance_k80":
            ap_rows(name, K, hw, padded, image, out, args.iters, dev, boundary="boundary" in kinds)
        if "eval" in kinds:
            eval_rows(name, K, hw, padded, image, out, args.iters, dev)
        if "base" not in kinds:
            continue
        cfg = InferenceConfig(num_classes=K, num_queries=100, **kw)
        lg, mk = inputs(K, hw, dev)
        t_nat, m_nat = timed(lambda: postprocess(lg, mk, [image], padded, [out], cfg), args.iters)
        t_ref, m_ref = timed(lambda: restate(lg, mk, [image], padded, [out], cfg), max(3, args.iters // 4))
        by, fl = work(K, cfg, hw, out)
        print(json.dumps({"case": name, "native_us": round(t_nat, 1), "restatement_us": round(t_ref, 1),
                          "speedup": round(t_ref / t_nat, 2), "native_peak_MB": round(m_nat, 1), "restatement_peak_MB": round(m_ref, 1),
                          "alg_MB": round(by / 1e6, 1), "alg_GFLOP": round(fl / 1e9, 2),
                          "frac_6.3TBps": round(by / (t_nat * 1e-6) / 6.3e12, 3), "frac_157TF": round(fl / (t_nat * 1e-6) / 157e12, 3)}),
              flush=True)


if __name__ == "__main__":
    main()
