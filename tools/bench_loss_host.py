#!/usr/bin/env python3
"""Host time per call of the loss host layer (problem record, check, route, launch): 1 000 back-to-back calls each of mpf_match_cost,
mpf_sample_select_uncertain, mpf_mask_loss_forward, mpf_mask_loss_backward_dense and mpf_match_cost_clip on the criterion's planes
(256 x 256 bf16 = 128 KiB, so every entry takes its LDS route with the dynamic-LDS size of a training step) but with two rows and
1 024 points (3 072 candidates) — small, so the device keeps up and the loop is paced by the launch thread — between two stream
synchronisations, timed with the host clock.  Prints one JSON line per entry and repeat.  A/B two builds with MPF_LIB_PATH
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
    h = w = 256
    n, P, F, Tmax, H, W = 2, 1024, 2, 4, 64, 64
    M, k = 3 * P, 3 * P // 4
    maps = torch.randn(n, F, h, w, device=dev).bfloat16()
    offs, offs_clip = (torch.arange(n, device=dev) * h * w).long(), (torch.arange(n, device=dev) * F * h * w).long()
    coords, cand = torch.rand(n, P, 2, device=dev), torch.rand(n, M, 2, device=dev)
    picked = torch.empty(n, k, 2, device=dev)
    gt = (torch.rand(n, H, W, device=dev) < 0.4).view(torch.uint8)
    rows = torch.arange(n, device=dev, dtype=torch.int32)
    partial, gs = torch.empty(n, 8, 4, device=dev), torch.randn(n, 4, device=dev)
    grad = torch.empty(n, h, w, device=dev, dtype=torch.bfloat16)
    tsamp = torch.rand(Tmax, F * P, device=dev)
    crow, first, cnt = (torch.full((n,), v, device=dev, dtype=torch.int32) for v in (0, 0, Tmax))
    cost = torch.empty(n, Tmax, device=dev)
    ws = torch.empty(lib.mpf_match_cost_clip_workspace_bytes(n, F, Tmax), dtype=torch.uint8, device=dev)
    bf, u8 = _lib.MPF_BF16, _lib.MPF_U8
    cost_tail = (coords.data_ptr(), crow.data_ptr(), tsamp.data_ptr(), first.data_ptr(), cnt.data_ptr(), cost.data_ptr(), n, Tmax, P, 5.0, 5.0, n)
    entries = {
        "mpf_match_cost": (maps.data_ptr(), bf, h, w, offs_clip.data_ptr(), *cost_tail, st),
        "mpf_sample_select_uncertain": (maps.data_ptr(), bf, h, w, offs.data_ptr(), cand.data_ptr(), picked.data_ptr(), n, M, k, k, st),
        "mpf_mask_loss_forward": (maps.data_ptr(), bf, h, w, offs.data_ptr(), gt.data_ptr(), u8, H, W, rows.data_ptr(), coords.data_ptr(),
                                  partial.data_ptr(), n, P, 8, st),
        "mpf_mask_loss_backward_dense": (maps.data_ptr(), bf, h, w, offs.data_ptr(), gt.data_ptr(), u8, H, W, rows.data_ptr(), coords.data_ptr(),
                                         gs.data_ptr(), grad.data_ptr(), bf, offs.data_ptr(), n, P, st),
        "mpf_match_cost_clip": (maps.data_ptr(), bf, h, w, offs_clip.data_ptr(), F, h * w, *cost_tail, ws.data_ptr(), ws.numel(), st),
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
            print(json.dumps({"what": f"host us per {name} call (256 x 256 bf16, n = 2, P = 1024)", "calls": calls, "us_per_call": round(us, 3),
                              "kernel": _lib.last_kernel(), "lib": _lib.LIB_PATH}), flush=True)


if __name__ == "__main__":
    main()
