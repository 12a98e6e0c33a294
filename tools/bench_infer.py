"""Inference post-processing: native route (mp_former_amd.inference.postprocess) vs the torch restatement of the reference's
eval branch (tests/_infer_restate.py), per image on one GPU.  Prints one line per case: us per image, peak MB above the
inputs, the algorithmic bytes / FLOP of the native route and the fraction of the measured 6.3 TB/s copy rate or of the
157 TF fp32 peak it reaches (whichever bound applies).

    python tools/bench_infer.py [--iters 20]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from _infer_restate import restate  # noqa: E402
from mp_former_amd.inference import InferenceConfig, postprocess  # noqa: E402

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


def inputs(K, hw, dev, Q=100):
    g = torch.Generator().manual_seed(0)
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
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in args.cases.split(","):
        K, hw, padded, image, out, kw = CASES[name]
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
