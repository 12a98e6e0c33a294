"""Independent torch restatement of the eval branch after the head (maskformer_model.py:236-279, :301-401), shared by
tests/test_infer_cpu.py, tests/test_infer_gpu.py and tools/bench_infer.py.  It materialises the full-resolution masks as
the reference does, so it also yields what the native route does not keep: the final-resolution logits (for the tie-band
margins of the GPU comparisons) and the per-query panoptic areas (for the host segment table)."""
import torch
import torch.nn.functional as F

from mp_former_amd.inference import segment_table


def _resize(x, size):
    return F.interpolate(x, size=tuple(int(s) for s in size), mode="bilinear", align_corners=False)


def restate(pred_logits, pred_masks, image_sizes, padded_hw, output_sizes, cfg, keep_margins=False):
    """-> list of per-image dicts like mp_former_amd.inference.postprocess, plus (keep_margins) "logits" [Q, H, W] at the final
    resolution, "pan_gap" [H, W] (winner minus runner-up of score * sigmoid) and "areas" (labels, mask, original, inter)."""
    K = cfg.num_classes
    padded = _resize(pred_masks.float(), padded_hw)
    out = []
    for n in range(pred_logits.shape[0]):
        hi, wi = (int(v) for v in image_sizes[n])
        H, W = (int(v) for v in output_sizes[n])
        prob = pred_logits[n].float().softmax(-1)
        crop = padded[n, :, :hi, :wi]
        m = _resize(crop[None], (H, W))[0] if cfg.sem_seg_postprocess_before_inference else crop
        sig = m.sigmoid()
        res = {}
        if cfg.semantic_on:
            sem = (prob[:, :K].t() @ sig.flatten(1)).view(K, *sig.shape[1:])
            res["sem_seg"] = sem if cfg.sem_seg_postprocess_before_inference else _resize(sem[None], (H, W))[0]
        if cfg.panoptic_on:
            score, label = prob.max(-1)
            kept = torch.nonzero((label != K) & (score > cfg.object_mask_threshold)).flatten()
            ids = torch.zeros((H, W), dtype=torch.int32, device=m.device)
            info = []
            gap = torch.full((H, W), float("inf"), device=m.device)
            areas = ([], [], [], [])
            if kept.numel():
                ks = sig[kept]
                weighted = score[kept][:, None, None] * ks
                win = weighted.argmax(0)
                if kept.numel() > 1:
                    top2 = weighted.topk(2, dim=0).values
                    gap = top2[0] - top2[1]
                n_k = kept.numel()
                onehot = win[None] == torch.arange(n_k, device=m.device)[:, None, None]
                on = ks >= 0.5
                labels = label[kept].tolist()
                mask_area = onehot.flatten(1).sum(1).tolist()
                orig = on.flatten(1).sum(1).tolist()
                inter = (onehot & on).flatten(1).sum(1).tolist()
                areas = (labels, mask_area, orig, inter)
                lut, info = segment_table(labels, mask_area, orig, inter, cfg.thing_ids, cfg.overlap_threshold)
                lut_t = torch.tensor(lut, dtype=torch.int32, device=m.device)
                won_on = torch.gather(on, 0, win[None])[0]
                ids = torch.where(won_on, lut_t[win], torch.zeros_like(ids))
            res["panoptic_seg"] = (ids, info)
            if keep_margins:
                res["pan_gap"], res["areas"] = gap, areas
        if cfg.instance_on:
            flat = prob[:, :K].reshape(-1)
            sc, idx = flat.topk(min(cfg.test_topk_per_image, flat.numel()))
            q, lab = idx // K, idx % K
            if cfg.panoptic_on:
                sel = torch.tensor([int(c) in cfg.thing_ids for c in lab.tolist()], dtype=torch.bool, device=sc.device)
                sc, q, lab = sc[sel], q[sel], lab[sel]
            mq = m[q]
            binm = (mq > 0).float()
            mscore = (mq.sigmoid() * binm).flatten(1).sum(1) / (binm.flatten(1).sum(1) + 1e-6)
            res["instances"] = {"pred_masks": binm, "scores": sc * mscore, "pred_classes": lab, "query": q}
        if keep_margins:
            res["logits"] = m
        out.append(res)
    return out
