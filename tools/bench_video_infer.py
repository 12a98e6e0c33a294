"""Video instance segmentation post-processing: the native route (mp_former_amd.inference.postprocess_video) against the torch
restatement of the reference's video eval branch (tests/_video_restate.py: upsample all Q x F planes to the padded size, select,
crop, resize, threshold), for one clip on one GPU.

    python tools/bench_video_infer.py [--iters 20] [--frames 36]

One JSON line per row.  Every time is the median over --iters of the wall clock between two device synchronisations, after a warm
call: the host copies and the host's list building are part of each product.  Peak MB is what the call allocates above what was
allocated before it (inputs and warm scratch); host bytes are what crosses to the host.
  restatement+cpu   the reference's product: bool [10, F, H, W] on the host ("pred_masks": [m for m in masks.cpu()])
  restatement       the same without the copy of the masks to the host (scores and labels still go through .tolist())
  native_dense      postprocess_video, masks "dense": bool [10, F, H, W] on the device, scores and labels as lists
  native_bits       masks "bits": packed words and frame areas, nothing crosses to the host
  native_rle        masks "rle": uncompressed run lengths on the host (two copies: offsets, counts)
The last line gives the kernel's own time (device events around the one launch) with its algorithmic bytes and the fraction of the
measured 6.3 TB/s copy rate they amount to; the kernel is bound by its resampling arithmetic and the strided logit reads, not by
those bytes.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from _video_restate import inference_video  # noqa: E402
from mp_former_amd import _lib  # noqa: E402
from mp_former_amd.inference import VideoInferenceConfig, postprocess_video  # noqa: E402

Q, K, TOPK = 100, 40, 10
LOWRES, PADDED, IMAGE, OUT = (96, 168), (384, 672), (360, 640), (360, 640)


def inputs(frames, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(Q, K + 1, generator=g)
    low = torch.randn(Q, frames, LOWRES[0] // 8, LOWRES[1] // 8, generator=g) * 4
    masks = torch.nn.functional.interpolate(low, size=LOWRES, mode="bilinear", align_corners=False)
    return logits.to(dev), masks.to(dev)


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
    return ts[len(ts) // 2], peak, ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frames", type=int, default=36)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_video_infer.py measures on the GPU: no device found")
    dev = torch.device("cuda:0")
    F = args.frames
    H, W = OUT
    lg, mk = inputs(F, dev)
    cfgs = {form: VideoInferenceConfig(num_classes=K, num_queries=Q, topk=TOPK, masks=form) for form in ("dense", "bits", "rle")}
    n_counts = []

    def native(form):
        return postprocess_video(lg, mk, IMAGE, PADDED, OUT, cfgs[form])

    def native_rle():
        r = native("rle")
        n_counts.append(sum(len(x["counts"]) for t in r["pred_masks_rle"] for x in t))
        return r

    def restatement(to_host):
        r = inference_video(lg, mk, IMAGE, PADDED, H, W, topk=TOPK)
        out = {"pred_scores": r["scores"].tolist(), "pred_labels": r["labels"].tolist()}
        out["pred_masks"] = [m for m in r["masks"].cpu()] if to_host else r["masks"]
        return out

    # the two routes give the same clip before anything is timed
    a, b = native("dense"), inference_video(lg, mk, IMAGE, PADDED, H, W, topk=TOPK)
    diff = a["pred_masks"] != b["masks"]
    same_sel = a["pred_queries"] == b["query"].tolist() and a["pred_labels"] == b["labels"].tolist()
    outside = int((diff & (b["logits"].abs() > 2e-5)).sum())
    print(json.dumps({"row": "check", "frames": F, "selection_equal": bool(same_sel), "mask_pixels_differing": int(diff.sum()),
                      "outside_tie_band": outside, "pixels": diff.numel()}), flush=True)
    del a, b, diff
    dense_bytes = TOPK * F * H * W
    rows = [("restatement+cpu", lambda: restatement(True), dense_bytes + 16 * TOPK, max(3, args.iters // 4)),
            ("restatement", lambda: restatement(False), 16 * TOPK, max(3, args.iters // 4)),
            ("native_dense", lambda: native("dense"), 20 * TOPK, args.iters),
            ("native_bits", lambda: native("bits"), 0, args.iters),
            ("native_rle", native_rle, None, args.iters)]
    times = {}
    for name, fn, host_bytes, iters in rows:
        t, peak, lo, hi = timed_wall(fn, iters)
        times[name] = t
        if host_bytes is None:
            host_bytes = 8 * (TOPK * F + 1) + 4 * n_counts[-1] + 20 * TOPK
        print(json.dumps({"row": name, "frames": F, "median_us": round(t, 1), "min_us": round(lo, 1), "max_us": round(hi, 1),
                          "iters": iters, "peak_MB": round(peak, 1), "host_bytes": int(host_bytes)}), flush=True)
    # the kernel alone: device events around the launch of the "bits" form
    query = torch.arange(TOPK, dtype=torch.int64, device=dev) * 7 % Q
    nwords = (H * W + 63) // 64
    bits = torch.empty((TOPK, F, nwords), dtype=torch.int64, device=dev)
    area = torch.empty((TOPK, F), dtype=torch.int32, device=dev)
    stream = _lib.stream_ptr(dev)

    def launch():
        _lib.call("mpf_seg_video_bits", dev, mk.data_ptr(), mk.stride(0), mk.stride(1), _lib.MPF_F32, Q, F, *LOWRES, *PADDED, *IMAGE, H, W,
                  query.data_ptr(), TOPK, bits.data_ptr(), area.data_ptr(), None, stream)
    launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(args.iters):
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    t_k = ts[len(ts) // 2]
    by = TOPK * F * LOWRES[0] * LOWRES[1] * 4 + TOPK * F * nwords * 8 + TOPK * F * 4
    ref_by = Q * F * PADDED[0] * PADDED[1] * 4 + TOPK * F * H * W * 4 + TOPK * F * H * W
    print(json.dumps({"row": "seg_video_bits_kernel", "frames": F, "median_us": round(t_k, 1), "alg_MB": round(by / 1e6, 2),
                      "frac_6.3TBps": round(by / (t_k * 1e-6) / 6.3e12, 4), "bits_MB": round(TOPK * F * nwords * 8 / 1e6, 2),
                      "reference_written_MB": round(ref_by / 1e6, 1),
                      "speedup_dense_vs_restatement+cpu": round(times["restatement+cpu"] / times["native_dense"], 2),
                      "speedup_dense_vs_restatement": round(times["restatement"] / times["native_dense"], 2),
                      "native_slower": bool(times["native_dense"] > times["restatement"])}), flush=True)


if __name__ == "__main__":
    main()
