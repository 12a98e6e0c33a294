"""Losses of a clip — mirror of mask2former_video/video_maskformer_model.py:227-253 (``prepare_targets``),
mask2former_video/modeling/matcher.py:70-189 (``VideoHungarianMatcher``) and modeling/criterion.py:90-259 (``VideoSetCriterion``).

The video criterion is the image criterion on (pair, frame) rows: a matched tube contributes its F planes as F rows of the
point-sampled BCE / dice sums, each with its own point set, and ``num_masks`` counts tubes.  Only the matching cost differs in
kind: it sums over the F * P samples of ONE point set shared by every frame and every mask of the clip (csrc/loss.hip,
``mpf_match_cost_clip``).  Everything else is the image path's native code on other index arrays:

  * ground truth: the [G, F, H, W] masks of a clip are G * F planes of the byte / bit-packed store (``GTTubes``), plane
    g * F + f; no float copy exists;
  * predictions: ``pred_masks`` [B, Q, F, h, w] is addressed in place as [B, Q * F, h, w] (``MapSet``): no gathered
    [M * F, 1, h, w] copy, and the gradient of the sums goes to it in one piece;
  * predictions as factors (``mask_fused.FactoredClipMasks``, the clip decoder with ``factored_masks = True``): the matching
    cost comes from (mask_embed, mask_features) directly (``mpf_match_cost_fused_clip``), and only the matched tubes get planes:
    ``PairPlanes`` on the clip as one tall image writes a pair's F frame planes back to back, which ARE its (pair, frame) rows;
  * assignment: the device solver by default (lsa.py) — the step has no device->host copy; it reports per pair the tube and
    the element offset of the matched query's first frame, which are expanded to (pair, frame) rows on the device.
"""
import os

import numpy as np
import torch

from . import _rng
from ._h2d import upload
from .criterion import LossDict, SetCriterion, group_mask_losses, strided_stack
from .dist import distributed, global_num_masks, global_num_masks_device
from .lsa import MAX_DIM as LSA_MAX_DIM, lsa_assign
from . import mask_fused
from .mask_fused import FactoredClipMasks, PairPlanes, match_cost_fused_clip
from .matcher import GTMasks, HungarianMatcher
from .point_sample import MapSet, MaskLossSums, MaskLossSumsPlanes, match_cost_clip, sample_select_uncertain


def prepare_video_targets(frame_masks, frame_ids, classes, padded_hw):
    """The targets of one clip (video_maskformer_model.py:227-253).  frame_masks: F tensors [G, h_f, w_f] (bool), frame_ids: F
    vectors [G] (-1 = the instance is absent from that frame), classes [G] (the reference reads the LAST frame's ``gt_classes``),
    padded_hw = the padded image size.  -> {"labels" [G'], "ids" [G', F], "masks" [G', F, H_pad, W_pad] bool} with the instances
    dropped whose id is -1 in every frame.  Plain torch on the tensors' device (the masks stay bool: the native matcher and
    criterion read bytes / bits, the reference's ``.float()`` copy has no reader here); only G' is read back, by the boolean
    index, as in the reference."""
    H, W = int(padded_hw[0]), int(padded_hw[1])
    G, dev = frame_masks[0].shape[0], frame_masks[0].device
    masks = torch.zeros((G, len(frame_masks), H, W), dtype=torch.bool, device=dev)
    for f, m in enumerate(frame_masks):
        masks[:, f, :m.shape[-2], :m.shape[-1]] = m
    ids = torch.stack(list(frame_ids), dim=1)
    valid = (ids != -1).any(dim=-1)
    return {"labels": classes[valid], "ids": ids[valid], "masks": masks[valid]}


def clip_planes(pred_masks):
    """[B, Q, F, h, w] -> the same memory as [B, Q * F, h, w] where the strides allow it (a query-slice view of a larger tensor
    does), a copy otherwise: frame f of query q is row q * F + f.  Factors are evaluated first."""
    if isinstance(pred_masks, FactoredClipMasks):
        pred_masks = pred_masks.materialize()
    B, Q, Fr, h, w = pred_masks.shape
    return pred_masks.reshape(B, Q * Fr, h, w)


class GTTubes(GTMasks):
    """The ground-truth tubes of a batch: the G_b * F planes of every clip in the byte / bit-packed store of ``GTMasks`` (row =
    tube * F + frame, ``image_of_row`` per plane), while ``counts`` / ``offsets`` / ``total`` / ``tmax`` count TUBES, which is what
    the matcher and the criterion assign."""

    def __init__(self, targets):
        m0 = targets[0]["masks"]
        if m0.dim() != 4:
            raise RuntimeError(f"video targets carry [G, F, H, W] masks, got {tuple(m0.shape)}")
        self.F = int(m0.shape[1])
        super().__init__([{"masks": t["masks"].flatten(0, 1)} for t in targets])
        self.counts = [c // self.F for c in self.counts]
        self.offsets = [o // self.F for o in self.offsets]
        self.total, self.tmax = self.total // self.F, self.tmax // self.F


class VideoHungarianMatcher(HungarianMatcher):
    """``match_many`` / ``forward`` / ``__repr__`` are the image matcher's; the store holds tubes and the mask + dice cost is the
    clip kernel's."""

    @staticmethod
    def _store(targets):
        return GTTubes(targets)

    @torch.no_grad()
    def cost_matrices(self, outs, targets, gt=None, tags=None, mapset=None, map_index=None):
        """The matching cost of every (output, clip, query, tube) (matcher.py:96-148), on the device: fp32 [L, B, Q, Tmax]
        (columns >= the clip's tube count are padding), or None when no clip has a tube.  One sampling launch and one cost call
        for all outputs; draws the point sets either way (RNG parity).  ``mapset``: a MapSet of ``clip_planes`` of the outputs'
        masks, in output order."""
        L = len(outs)
        B, Q = outs[0]["pred_logits"].shape[:2]
        gt = gt or self._store(targets)
        dev = gt.device
        P = self.num_points
        tags = tags or ["match"] + [f"match_{i}" for i in range(L - 1)]
        # one point set per (output, clip), shared by all frames and masks of that clip (matcher.py:120)
        coords = _rng.rand_cat([(tags[l], (1, P, 2)) for l in range(L) for _ in range(B)], dev)   # [L*B,P,2]
        if gt.tmax == 0:
            return None
        Fr = gt.F
        if outs[0]["pred_masks"].shape[2] != Fr:
            raise RuntimeError(f"pred_masks has {outs[0]['pred_masks'].shape[2]} frames, the targets {Fr}")
        Tt, Tmax = gt.total, gt.tmax
        counts = np.asarray(gt.counts, dtype=np.int64)
        firsts = np.asarray(gt.offsets[:-1], dtype=np.int64)
        # ground-truth samples [L*Tt*F, P] = [L*Tt, F*P] frame-major: every plane at the point set of its (output, clip)
        n_planes = Tt * Fr
        gt_offs = np.tile(np.arange(n_planes, dtype=np.int64) * (gt.H * gt.W), L)
        gcrow = (np.repeat(np.arange(L), n_planes) * B + np.tile(gt.image_of_row, L)).astype(np.int32)
        masks = [o["pred_masks"] for o in outs]
        if (mapset is None and not self.reference_amp_rounding and Tmax <= 128
                and all(isinstance(m, FactoredClipMasks) and m.same_factors(masks[0]) for m in masks)
                and mask_fused.supported(masks[0].me, masks[0].mf)):
            # the maps are kept as (mask_embed, mask_features): cost straight from the factors (csrc/mask_fused.hip)
            tsamp = self._gt_samples(gt, upload(gt_offs, dev), coords, upload(gcrow, dev), dev)
            l_idx, b_idx = np.meshgrid(np.arange(L), np.arange(B), indexing="ij")
            l_idx, b_idx = l_idx.reshape(-1), b_idx.reshape(-1)
            C = match_cost_fused_clip(masks, coords, tsamp, l_idx * Tt + firsts[b_idx], counts[b_idx], l_idx, b_idx, Q, Tmax,
                                      self.cost_mask, self.cost_dice).view(L, B, Q, Tmax)
            return self._add_class_cost(C, outs, targets, gt)
        if mapset is None:
            mapset = MapSet([clip_planes(m) for m in masks])
        l_idx, b_idx, q_idx = np.meshgrid(np.arange(L), np.arange(B), np.arange(Q), indexing="ij")
        l_idx, b_idx, q_idx = l_idx.reshape(-1), b_idx.reshape(-1), q_idx.reshape(-1)
        pred_offs = mapset.offsets(l_idx, b_idx, q_idx * Fr)                # frame 0 of every (output, clip, query)
        i64 = upload(np.concatenate([pred_offs, gt_offs]), dev)
        i32 = upload(np.concatenate([
            (l_idx * B + b_idx),                                            # coord row of every prediction row
            (l_idx * Tt + firsts[b_idx]),                                   # first tsamp row (of F*P floats) of its clip
            counts[b_idx],                                                  # number of tubes of its clip
            gcrow,                                                          # coord row of every ground-truth plane
        ]).astype(np.int32), dev)
        n_rows = L * B * Q
        pred_offs_d, gt_offs_d = i64[:n_rows], i64[n_rows:]
        crow_d, tfirst_d, tcount_d, gcrow_d = i32[:n_rows], i32[n_rows:2 * n_rows], i32[2 * n_rows:3 * n_rows], i32[3 * n_rows:]
        tsamp = self._gt_samples(gt, gt_offs_d, coords, gcrow_d, dev)
        C = match_cost_clip(mapset, pred_offs_d, Fr, coords, crow_d, tsamp, tfirst_d, tcount_d, Tmax, self.cost_mask, self.cost_dice,
                            rows_per_group=Q).view(L, B, Q, Tmax)           # rows are (l, b, q), q fastest
        return self._add_class_cost(C, outs, targets, gt)


class VideoSetCriterion(SetCriterion):
    """The reference's constructor arguments (the image criterion's, without its ``dn_no_lb``), same ``forward(outputs, targets) -> dict`` with its 3 x (1 + #aux) keys.  Class loss,
    ``weighted_total`` and ``__repr__`` are the image criterion's."""

    def forward(self, outputs, targets):
        outs = [{"pred_logits": outputs["pred_logits"], "pred_masks": outputs["pred_masks"]}] + list(outputs.get("aux_outputs", []))
        L = len(outs)
        suffixes = [""] + [f"_{i}" for i in range(L - 1)]
        B, Q = outs[0]["pred_logits"].shape[:2]
        Fr, h, w = outs[0]["pred_masks"].shape[2:]
        dev = outs[0]["pred_logits"].device
        K, P = self.num_classes, self.num_points
        n_local = sum(len(t["labels"]) for t in targets)                    # tubes, not tube-frames (criterion.py:221)
        num_masks = global_num_masks_device(n_local, dev) if distributed() else global_num_masks(n_local, dev)

        gt = GTTubes(targets)
        # the clip decoder's training path may hand the predictions over as their factors (mask_fused.FactoredClipMasks):
        # matching cost and loss planes are then produced from (mask_embed, mask_features) and no [B, Q, F, h, w] map exists;
        # factors this route cannot take (mixed, more than 128 tubes in a clip, unsupported operands) are evaluated here
        masks = [o["pred_masks"] for o in outs]
        fm = masks[0] if isinstance(masks[0], FactoredClipMasks) else None
        if fm is not None and not (all(fm.same_factors(m) for m in masks) and gt.tmax <= 128 and mask_fused.supported(fm.me, fm.mf)):
            fm = None
        if fm is None and any(isinstance(m, FactoredClipMasks) for m in masks):
            masks = [m.materialize() if isinstance(m, FactoredClipMasks) else m for m in masks]
            outs = [{"pred_logits": o["pred_logits"], "pred_masks": m} for o, m in zip(outs, masks)]
        ms = MapSet([clip_planes(m) for m in masks]) if fm is None else None
        hw = h * w

        # ---- stage 1: all matchings (device solver, or MPF_DEVICE_LSA=0 / a large problem: one D2H copy + SciPy) ----------------
        tags = ["match" + s for s in suffixes]
        dev_lsa = (os.environ.get("MPF_DEVICE_LSA", "1") == "1" and max(Q, gt.tmax) <= LSA_MAX_DIM)
        firsts = gt.offsets
        if dev_lsa:
            C = self.matcher.cost_matrices(outs, targets, gt=gt, tags=tags, mapset=ms)
            indices = None
        else:
            indices = self.matcher.match_many(outs, targets, gt=gt, tags=tags, mapset=ms)

        # ---- pair lists (host): per output, per clip, min(Q, tubes) pairs ------------------------------------------------------
        ti, bi, qi, tube, over_parts, rand_parts = [], [], [], [], [], []
        num_uncertain = int(self.importance_sample_ratio * P)
        num_sampled = int(P * self.oversample_ratio)
        logits_main, order_main = strided_stack([o["pred_logits"] for o in outs])
        slot_of_output = {l: i for i, l in enumerate(order_main)}            # row of output l in logits_main
        problems = []
        n_pairs = 0
        if dev_lsa:
            labels_dev = torch.cat([t["labels"] for t in targets]) if gt.total else None
            Tmax = gt.tmax
        else:
            tc_main = np.full((L, B, Q), K, dtype=np.int64)
            if gt.total:
                lab = torch.cat([t["labels"] for t in targets]).cpu().numpy()
                labels_host = [lab[firsts[b]:firsts[b + 1]] for b in range(B)]
        for l in range(L):
            n_l = 0
            for b in range(B):
                if dev_lsa:
                    k = min(Q, gt.counts[b])
                    if k:
                        problems.append([(l * B + b) * Q * Tmax, Q, gt.counts[b], Tmax, n_pairs, firsts[b],
                                         0, 0, 0, 0, (slot_of_output[l] * B + b) * Q])
                    src = np.zeros(k, np.int64)      # filled in on the device
                    tgt = np.zeros(k, np.int64)
                else:
                    src, tgt = (x.numpy() for x in indices[l][b])
                    if len(src):
                        tc_main[l, b, src] = labels_host[b][tgt]
                ti.append(np.full(len(src), l)); bi.append(np.full(len(src), b)); qi.append(src)
                tube.append(firsts[b] + tgt)
                n_l += len(src)
                n_pairs += len(src)
            # one point set per (pair, frame) (criterion.py:154-165: the matched tubes are flattened to M * F rows)
            over_parts.append(("loss" + suffixes[l] + "_over", (n_l * Fr, num_sampled, 2)))
            rand_parts.append(("loss" + suffixes[l] + "_rand", (n_l * Fr, P - num_uncertain, 2)))
        cat = lambda xs: np.concatenate(xs).astype(np.int64) if xs else np.zeros(0, np.int64)  # noqa: E731
        ti, bi, qi, tube = cat(ti), cat(bi), cat(qi), cat(tube)
        losses = LossDict()

        # ---- index arrays of the pairs -> device; the solver fills them; then one row per (pair, frame) ------------------------
        tc_main_d = torch.full((L, B, Q), K, dtype=torch.int64, device=dev) if dev_lsa else None
        planes = None
        if n_pairs:
            if fm is not None:
                # factors: pair i = embedding row p_offs[i] (elements from mask_embed's base) -> slot[i] of a compact
                # [pairs, F * h * w] tensor produced AFTER the assignment: the pair's F frame planes back to back
                q0s = np.array([m.q0 for m in masks], dtype=np.int64)
                p_offs = bi * fm.me.stride(0) + (q0s[ti] + qi) * fm.me.stride(1)
                slot, s_first, s_count = self._slot_layout(bi, B)
                g_offs = slot * (Fr * hw)
                # (a pair's slot does not depend on the matched query)
                q_stride, g_stride = np.full(n_pairs, fm.me.stride(1), dtype=np.int64), 0
                if not dev_lsa:
                    # mpf_pair_planes_backward WRITES the d_embed row of a slot (include/mpformer_hip.h): rows must be distinct
                    assert len(np.unique(p_offs)) == n_pairs, "an embedding row is paired twice in one step"
            else:
                p_offs = ms.offsets(ti, bi, qi * Fr)                        # frame 0 of the matched query
                g_offs = ms.grad_offsets(ti, bi, qi * Fr)
                q_stride, g_stride = ms.s1[ms.base_of[ti]] * Fr, Fr * hw    # a query is F planes further on
                if not dev_lsa:
                    assert len(np.unique(g_offs)) == n_pairs, "a prediction tube is paired twice in one step"
            up = upload(np.concatenate([p_offs, g_offs]), dev)
            pair_pred, pair_grad = up[:n_pairs], up[n_pairs:]
            pair_tube = upload(tube.astype(np.int32), dev)
            if dev_lsa and problems:
                pr = np.asarray(problems, dtype=np.int64)
                pos = pr[:, 4]
                pr[:, 6], pr[:, 7] = p_offs[pos], q_stride[pos]
                pr[:, 8], pr[:, 9] = g_offs[pos], g_stride
                into = {"cols": pair_tube, "a": pair_pred}
                if fm is None:
                    into["b"] = pair_grad
                lsa_assign(C, pr, n_pairs, want_rows=False, scatter_dst=tc_main_d, scatter_src=labels_dev, into=into)
            if fm is not None:
                inv = np.zeros(n_pairs, dtype=np.int32)
                inv[slot] = np.arange(n_pairs, dtype=np.int32)
                i32 = upload(np.concatenate([inv, s_first, s_count]), dev)
                planes = PairPlanes.apply(fm.me, fm.mf, pair_pred, i32[:n_pairs], i32[n_pairs:n_pairs + B], i32[n_pairs + B:],
                                          n_pairs, int(s_count.max()))
                ms = MapSet([planes.view(1, n_pairs * Fr, h, w)])
                pair_pred = pair_grad               # from here on a pair is addressed by its planes
            fr = torch.arange(Fr, dtype=torch.int64, device=dev)
            pred_offs = (pair_pred[:, None] + fr * hw).reshape(-1)           # row = pair * F + frame (criterion.py:154-155)
            grad_offs = (pair_grad[:, None] + fr * hw).reshape(-1)
            gt_rows = (pair_tube[:, None] * Fr + fr.to(torch.int32)).reshape(-1)       # plane tube * F + frame of the store
            gid = np.repeat(ti, Fr)                                          # group = output: one run of the row list each

        # ---- stage 2: mask losses ----------------------------------------------------------------------------------------------
        if "masks" in self.losses:
            if n_pairs:
                with torch.no_grad():   # criterion.py:157-171: point selection carries no gradient
                    coords_over = _rng.rand_cat(over_parts, dev)
                    coords = sample_select_uncertain(ms, pred_offs, coords_over, num_uncertain, P)
                    if P - num_uncertain > 0:
                        coords[:, num_uncertain:] = _rng.rand_cat(rand_parts, dev)
                if planes is not None:
                    sums = MaskLossSumsPlanes.apply(ms, pred_offs, gt, gt_rows, coords, planes)
                else:
                    sums = MaskLossSums.apply(ms, pred_offs, grad_offs, gt, gt_rows, coords, *ms.bases)
                if torch.is_tensor(num_masks):
                    norm = num_masks * upload([1.0] * L, dev, torch.float32)
                else:
                    norm = upload([float(num_masks)] * L, dev, torch.float32)
                g_mask, g_dice = group_mask_losses(sums, gid, None, L, norm, P)
            else:
                # no tube anywhere: sums over empty sets (still consume the draws for RNG parity)
                _rng.rand_cat(over_parts, dev)
                _rng.rand_cat(rand_parts, dev)
                if fm is not None:
                    zero = (fm.me.sum() * 0.0 + fm.mf.sum() * 0.0).float()
                else:
                    zero = sum(m.sum() * 0.0 for m in masks).float()
                g_mask = g_dice = zero.expand(L)
            losses.add_group(["loss_mask" + s_ for s_ in suffixes], g_mask)
            losses.add_group(["loss_dice" + s_ for s_ in suffixes], g_dice)

        # ---- stage 3: class losses ---------------------------------------------------------------------------------------------
        if "labels" in self.losses:
            tc_d = tc_main_d if dev_lsa else upload(tc_main[order_main], dev)
            ce = self._class_losses(logits_main, tc_d)
            losses.add_group(["loss_ce" + suffixes[i] for i in order_main], ce)
        return losses
