#!/usr/bin/env python3
"""Host time per call of the fused mask product host layer (problem record, check, launch): 1 000 back-to-back calls each of
mpf_match_cost_fused, mpf_match_cost_fused_clip, mpf_pair_planes_forward and mpf_pair_planes_backward between two stream
synchronisations, timed with the host clock.  The cost entries get 20 target columns, the most a benchmark image has, so they run
the training step's instantiation (TCH = 12, 52 736 bytes of dynamic LDS), but two groups of 100 queries at 128 points on 16 x 16
planes (the clip: two frames), and the pair planes two images of 256 pixels with four slots each — small, so the device keeps up
and the loop is paced by the launch thread.  Prints one JSON line per entry and repeat.  A/B two builds with MPF_LIB_PATH
(tools/ab_lib.sh)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mp_former_amd import _lib  # noqa: E402


def main(calls=1000, repeats=5):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    C, G, Q, Tmax, P, F, h, w = 256, 2, 100, 20, 128, 2, 16, 16
    N, HW, per_image = 2, h * w, 4
    slots = N * per_image
    embed = (torch.randn(G, Q, C, device=dev) * 0.5).bfloat16()
    feat = torch.randn(G, F, h * w, C, device=dev).bfloat16()
    first = (torch.arange(G, device=dev) * Q * C).long()
    group, t_first, t_count = (torch.tensor(v, device=dev, dtype=torch.int32) for v in ([0, 1], [0, Tmax], [Tmax, Tmax]))
    coords, tsamp = torch.rand(G, F * P, 2, device=dev), torch.rand(2 * Tmax, F * P, device=dev)          # (the clip entry reads P points per group)
    cost = torch.empty(G, Q, Tmax, device=dev)
    ws_img = torch.empty(lib.mpf_match_cost_fused_workspace_bytes(G, Q, Tmax, F * P, 2 * Tmax), dtype=torch.uint8, device=dev)
    ws_clip = torch.empty(lib.mpf_match_cost_fused_clip_workspace_bytes(G, Q, Tmax, P, F, 2 * Tmax), dtype=torch.uint8, device=dev)
    row_off = (torch.arange(slots, device=dev) * C).long()
    slot_first = torch.tensor([0, per_image], device=dev, dtype=torch.int32)
    slot_count = torch.full((N,), per_image, device=dev, dtype=torch.int32)
    planes = torch.empty(slots, HW, device=dev, dtype=torch.bfloat16)
    grad = torch.randn(slots, HW, device=dev).bfloat16()
    d_feat, d_embed = torch.empty(N, HW, C, device=dev, dtype=torch.bfloat16), torch.zeros_like(embed)
    ws_bwd = torch.empty(lib.mpf_pair_planes_backward_workspace_bytes(N, HW, slots, per_image), dtype=torch.uint8, device=dev)
    cost_tail = (coords.data_ptr(), tsamp.data_ptr(), 2 * Tmax, t_first.data_ptr(), t_count.data_ptr(), cost.data_ptr(), G, Q, Tmax)
    pair_head = (embed.data_ptr(), row_off.data_ptr(), None, slot_first.data_ptr(), slot_count.data_ptr(), feat.data_ptr(), F * HW * C)
    entries = {
        # (the image entry reads the two frames' samples as one row of 2 P points of the first frame's plane)
        "mpf_match_cost_fused": (embed.data_ptr(), first.data_ptr(), C, feat.data_ptr(), F * HW * C, group.data_ptr(), h, w, C, *cost_tail, F * P,
                                 5.0, 5.0, ws_img.data_ptr(), ws_img.numel(), st),
        "mpf_match_cost_fused_clip": (embed.data_ptr(), first.data_ptr(), C, feat.data_ptr(), F * HW * C, HW * C, group.data_ptr(), h, w, C,
                                      *cost_tail, P, F, 5.0, 5.0, ws_clip.data_ptr(), ws_clip.numel(), st),
        "mpf_pair_planes_forward": (*pair_head, planes.data_ptr(), N, HW, C, st),
        "mpf_pair_planes_backward": (grad.data_ptr(), *pair_head, d_feat.data_ptr(), HW * C, d_embed.data_ptr(), _lib.MPF_BF16, N, HW, C, slots,
                                     per_image, ws_bwd.data_ptr(), ws_bwd.numel(), st),
    }
    for name, args in entries.items():
        fn = getattr(lib, name)
        for _ in range(100):
            _lib.check(fn(*args), name)
    for _ in range(repeats):
        for name, args in entries.items():
            fn = getattr(lib, name)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn(*args)
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / calls * 1e6
            print(json.dumps({"what": f"host us per {name} call (Tmax = 20, 2 groups x 100 queries, 128 points; 2 x 256 pixels, 8 slots)",
                              "calls": calls, "us_per_call": round(us, 3), "kernel": _lib.last_kernel(), "lib": _lib.LIB_PATH}), flush=True)


if __name__ == "__main__":
    main()
