"""Losses of a clip, forward + backward: the native matcher + criterion (mp_former_amd/video_losses.py) against the fp32 torch
restatement of the reference's (tests/_vtrain_restate.py: per (output, clip) cost matrix, blocking copy and SciPy; gathered
[M*F, 1, h, w] predictions, float tubes, two point_sample calls, topk over [M*F, 3P]) on the same GPU.

    python tools/bench_video_losses.py [--iters 10] [--ref-iters 4] [--factored-iters 10] [--only-factored]

YouTube-VIS training shape: B = 2 clips of F = 2 frames, Q = 100 queries, L = 10 decoder outputs, P = 12544 points (oversample 3,
importance 0.75), mask logits 96 x 160 (bf16 for the native route, the same values as fp32 for the restatement), ground truth
384 x 640, 8 tubes per clip, K = 40 classes.

One JSON line per row.  "check": both routes on the same replayed draws, before anything is timed.  "native" / "restatement": a
step = criterion forward, weighted total, backward to pred_masks and pred_logits; times are the median over the iterations, after
two warm steps, of (a) the wall clock between two device synchronisations and (b) device events around the step; the draws are the
production ones (torch.rand on the device).  "native_kernels": the native launches of one step and their summed device time
(the library's own event pairs).  "launches": device kernels of one step per route, from torch.profiler.

"maps_from_factors" / "factored": the two ways from the decoder's heads to the losses, both starting from the same bf16
(mask_embed [B, L*Q, 256], channel-last mask_features [B*F, 256, 96, 160]) with gradients back to both.  "maps_from_factors"
forms the [B, L*Q, F, h, w] parent with the native product INSIDE the step (and pays its backward), then runs the map route
above; "factored" hands the criterion mask_fused.FactoredClipMasks.  The routes alternate call by call; each row gives the
median with min - max of wall clock and device events, and torch.cuda.max_memory_allocated over a step with the bytes allocated
before it.  "factored_check": both on the same replayed draws, before anything is timed.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _vtrain_restate as VR  # noqa: E402
from mp_former_amd import _lib, _rng, mask_fused  # noqa: E402
from mp_former_amd.video_losses import VideoHungarianMatcher, VideoSetCriterion  # noqa: E402

B, FRAMES, Q, L, K, P = 2, 2, 100, 10, 40, 12544
LOWRES, GT_HW, TUBES = (96, 160), (384, 640), 8
OVERSAMPLE, IMPORTANCE = 3.0, 0.75
W_CLASS, W_MASK, W_DICE, EOS = 2.0, 5.0, 5.0, 0.1


def inputs(dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(L, B, Q, FRAMES, LOWRES[0] // 8, LOWRES[1] // 8, generator=g) * 4
    masks = torch.nn.functional.interpolate(low.flatten(0, 3)[None], size=LOWRES, mode="bilinear", align_corners=False)[0]
    masks = masks.view(L, B, Q, FRAMES, *LOWRES).to(torch.bfloat16)
    logits = torch.randn(L, B, Q, K + 1, generator=g) * 2
    targets = []
    for _ in range(B):
        blobs = torch.rand(TUBES, FRAMES, GT_HW[0] // 32, GT_HW[1] // 32, generator=g) < 0.25
        m = torch.nn.functional.interpolate(blobs.float(), size=GT_HW, mode="nearest") > 0
        targets.append({"labels": torch.randint(0, K, (TUBES,), generator=g).to(dev), "masks": m.to(dev)})
    return masks.to(dev), logits.to(dev), targets


def weight_dict():
    base = {"loss_ce": W_CLASS, "loss_mask": W_MASK, "loss_dice": W_DICE}
    wd = dict(base)
    for i in range(L - 1):
        wd.update({k + f"_{i}": v for k, v in base.items()})
    return wd


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    wall, devt = [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        devt.append(e0.elapsed_time(e1))
    wall.sort(); devt.sort()
    return {"wall_ms_median": round(wall[len(wall) // 2], 3), "wall_ms_min": round(wall[0], 3), "wall_ms_max": round(wall[-1], 3),
            "event_ms_median": round(devt[len(devt) // 2], 3), "iters": iters}


def factors(dev, seed=2):
    """bf16 mask_embed [B, L*Q, 256] and channel-last mask_features [B*F, 256, h, w]; logits of ~N(0, 4^2)"""
    g = torch.Generator().manual_seed(seed)
    me = (torch.randn(B, L * Q, 256, generator=g) * 0.25).to(torch.bfloat16).to(dev)
    mf = torch.randn(B * FRAMES, *LOWRES, 256, generator=g).to(torch.bfloat16).to(dev).permute(0, 3, 1, 2)
    return me, mf


def timed_alternating(fns, iters):
    """fns: {name: step}; the routes take turns, one call each, ``iters`` rounds after two warm rounds"""
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    rec = {k: {"wall": [], "event": [], "peak": [], "before": []} for k in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(iters):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            r = rec[k]
            r["wall"].append((time.perf_counter() - t0) * 1e3); r["event"].append(e0.elapsed_time(e1))
            r["peak"].append(torch.cuda.max_memory_allocated()); r["before"].append(before)
    out = {}
    for k, r in rec.items():
        w, e = sorted(r["wall"]), sorted(r["event"])
        out[k] = {"wall_ms_median": round(w[len(w) // 2], 3), "wall_ms_min": round(w[0], 3), "wall_ms_max": round(w[-1], 3),
                  "event_ms_median": round(e[len(e) // 2], 3), "event_ms_min": round(e[0], 3), "event_ms_max": round(e[-1], 3),
                  "peak_allocated_mb": round(max(r["peak"]) / 2 ** 20, 1), "allocated_before_mb": round(max(r["before"]) / 2 ** 20, 1),
                  "iters": iters}
    return out


def factored_rows(dev, crit, logits, targets, wd, iters):
    me, mf = factors(dev)
    if not mask_fused.supported(me, mf.view(B, FRAMES, 256, *LOWRES).permute(0, 2, 1, 3, 4).reshape(B, 256, FRAMES * LOWRES[0], LOWRES[1])):
        raise SystemExit("bench_video_losses.py: the native product does not take the benchmark's factors")

    def step(factored):
        me_, mf_, lg = me.detach().requires_grad_(True), mf.detach().requires_grad_(True), logits.detach().requires_grad_(True)
        mf4 = mf_.view(B, FRAMES, 256, *LOWRES).permute(0, 2, 1, 3, 4).reshape(B, 256, FRAMES * LOWRES[0], LOWRES[1])
        pm = mask_fused.FactoredClipMasks(me_, mf4, FRAMES)
        if not factored:
            pm = pm.materialize()                      # the [B, L*Q, F, h, w] parent, and its backward, inside the step
        o = [{"pred_logits": lg[l], "pred_masks": pm[:, l * Q:(l + 1) * Q]} for l in range(L)]
        losses = crit(o[0] | {"aux_outputs": o[1:]}, targets)
        crit.weighted_total(losses).backward()
        return losses, me_.grad, mf_.grad

    g = torch.Generator().manual_seed(1)
    rows, k = min(Q, TUBES) * B * FRAMES, int(IMPORTANCE * P)
    draws = []
    for _ in range(L):
        draws += [torch.rand(1, P, 2, generator=g) for _ in range(B)]
        draws += [torch.rand(rows, int(P * OVERSAMPLE), 2, generator=g), torch.rand(rows, P - k, 2, generator=g)]
    res = []
    for factored in (False, True):
        try:
            _rng.install_replay(VR.draws_to_tags(draws, L, B))
            res.append(step(factored))
        finally:
            _rng.install_replay(None)
    (lm, gme_m, gmf_m), (lf, gme_f, gmf_f) = res
    rel = max(abs(float(lf[k_]) - float(lm[k_])) / max(abs(float(lm[k_])), 1e-6) for k_ in lm)
    print(json.dumps({"row": "factored_check", "max_rel_loss_diff": round(rel, 7),
                      "grad_me_rel_l2": round(float((gme_f.float() - gme_m.float()).norm() / gme_m.float().norm()), 5),
                      "grad_mf_rel_l2": round(float((gmf_f.float() - gmf_m.float()).norm() / gmf_m.float().norm()), 5)}), flush=True)
    del draws, res, lm, lf, gme_m, gmf_m, gme_f, gmf_f      # (a loss keeps its graph's maps alive)
    fns = {"maps_from_factors": lambda: step(False), "factored": lambda: step(True)}
    t = timed_alternating(fns, iters)
    for name, fn in fns.items():
        _lib.profile_enable(True)
        fn()
        torch.cuda.synchronize()
        n_all, ms_all, _ = _lib.profile_get("")
        n_mc, ms_mc, _ = _lib.profile_get("match_cost")
        _lib.profile_enable(False)
        print(json.dumps({"row": name, **t[name], "launches": kernel_launches(fn), "profiled_native_launches": n_all,
                          "profiled_native_ms": round(ms_all, 3), "match_cost_ms": round(ms_mc, 3), "match_cost_calls": n_mc}), flush=True)
    a, b = t["maps_from_factors"], t["factored"]
    print(json.dumps({"row": "factored_ratio", "maps_over_factored_wall": round(a["wall_ms_median"] / b["wall_ms_median"], 3),
                      "maps_over_factored_event": round(a["event_ms_median"] / b["event_ms_median"], 3),
                      "peak_mb_saved": round(a["peak_allocated_mb"] - b["peak_allocated_mb"], 1),
                      "factored_slower": bool(b["wall_ms_median"] > a["wall_ms_median"])}), flush=True)


def kernel_launches(fn):
    """device kernels of one call, or None where the profiler gives no device events"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        return n or None
    except Exception:   # noqa: BLE001 - a profiler that cannot start is "not measured", not a failed benchmark
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ref-iters", type=int, default=4)
    ap.add_argument("--factored-iters", type=int, default=10)
    ap.add_argument("--only-factored", action="store_true", help="skip the rows that compare with the torch restatement")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_video_losses.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    masks, logits, targets = inputs(dev)
    wd = weight_dict()
    crit = VideoSetCriterion(K, matcher=VideoHungarianMatcher(W_CLASS, W_MASK, W_DICE, P), weight_dict=wd, eos_coef=EOS,
                             losses=["labels", "masks"], num_points=P, oversample_ratio=OVERSAMPLE,
                             importance_sample_ratio=IMPORTANCE).to(dev)

    if args.only_factored:
        del masks
        factored_rows(dev, crit, logits, targets, wd, args.factored_iters)
        return
    masks32 = masks.float()

    def outs_of(m, lg):
        return [{"pred_logits": lg[l], "pred_masks": m[l]} for l in range(L)]

    def native():
        m, lg = masks.detach().requires_grad_(True), logits.detach().requires_grad_(True)
        o = outs_of(m, lg)
        losses = crit(o[0] | {"aux_outputs": o[1:]}, targets)
        crit.weighted_total(losses).backward()
        return losses, m.grad, lg.grad

    def restatement(draws=None):
        m, lg = masks32.detach().requires_grad_(True), logits.detach().requires_grad_(True)
        if draws is None:       # the reference's draws: one per (output, clip), then the two loss draws
            rows, k = min(Q, TUBES) * B * FRAMES, int(IMPORTANCE * P)
            draws = []
            for _ in range(L):
                draws += [torch.rand(1, P, 2, device=dev) for _ in range(B)]
                draws += [torch.rand(rows, int(P * OVERSAMPLE), 2, device=dev), torch.rand(rows, P - k, 2, device=dev)]
        losses, _, _ = VR.criterion(outs_of(m, lg), targets, draws, K, W_CLASS, W_MASK, W_DICE, EOS, P, OVERSAMPLE, IMPORTANCE,
                                    dtype=torch.float32)
        sum(losses[k] * wd[k] for k in losses).backward()
        return losses, m.grad, lg.grad

    # ---- the two routes on the same draws ------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(1)
    rows, k = min(Q, TUBES) * B * FRAMES, int(IMPORTANCE * P)
    draws = []
    for _ in range(L):
        draws += [torch.rand(1, P, 2, generator=g) for _ in range(B)]
        draws += [torch.rand(rows, int(P * OVERSAMPLE), 2, generator=g), torch.rand(rows, P - k, 2, generator=g)]
    try:
        _rng.install_replay(VR.draws_to_tags(draws, L, B))
        ln, gm_n, gl_n = native()
    finally:
        _rng.install_replay(None)
    lr, gm_r, gl_r = restatement([d.to(dev) for d in draws])
    rel = max(abs(float(ln[k_]) - float(lr[k_])) / max(abs(float(lr[k_])), 1e-6) for k_ in lr)
    print(json.dumps({"row": "check", "loss_keys": len(lr), "max_rel_loss_diff": round(rel, 6),
                      "grad_masks_rel_l2": round(float((gm_n.float() - gm_r).norm() / gm_r.norm()), 5),
                      "grad_logits_rel_l2": round(float((gl_n - gl_r).norm() / gl_r.norm()), 6)}), flush=True)
    del draws, gm_n, gm_r, gl_n, gl_r

    # ---- times ---------------------------------------------------------------------------------------------------------------
    t_n = timed(native, args.iters)
    print(json.dumps({"row": "native", **t_n}), flush=True)
    t_r = timed(restatement, args.ref_iters)
    print(json.dumps({"row": "restatement", **t_r}), flush=True)
    _lib.profile_enable(True)
    native()
    torch.cuda.synchronize()
    n_all, ms_all, _ = _lib.profile_get("")
    n_mc, ms_mc, _ = _lib.profile_get("match_cost_clip")
    _lib.profile_enable(False)
    print(json.dumps({"row": "native_kernels", "profiled_native_launches": n_all, "profiled_native_ms": round(ms_all, 3),
                      "match_cost_clip_calls": n_mc, "match_cost_clip_ms": round(ms_mc, 3), "kernel": _lib.last_kernel()}), flush=True)
    print(json.dumps({"row": "launches", "native": kernel_launches(native), "restatement": kernel_launches(restatement)}), flush=True)
    print(json.dumps({"row": "ratio", "restatement_over_native_wall": round(t_r["wall_ms_median"] / t_n["wall_ms_median"], 2),
                      "restatement_over_native_event": round(t_r["event_ms_median"] / t_n["event_ms_median"], 2),
                      "native_slower": bool(t_n["wall_ms_median"] > t_r["wall_ms_median"])}), flush=True)
    del masks32
    factored_rows(dev, crit, logits, targets, wd, args.factored_iters)


if __name__ == "__main__":
    main()
