#!/usr/bin/env python3
"""Host time per call of the attention host layer (problem record, check, split, launch): 2 000 back-to-back calls each of
mpf_attn_forward_kv, mpf_attn_bwd_prep_aux and mpf_attn_backward_kv_aux at the decoder's self-attention shape (Lq = Lk = 120, N = 2,
H = 8, one mask for all images) — small, so the device keeps up and the loop is paced by the launch thread — between two stream
synchronisations, timed with the host clock.  Prints one JSON line per entry and repeat.  A/B two builds with MPF_LIB_PATH
(tools/ab_lib.sh)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mp_former_amd import _lib  # noqa: E402


def main(calls=2000, repeats=5):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    Lq = Lk = 120
    N, H, E, LqP = 2, 8, 256, 128
    q, k, v, do = (torch.randn(Lq, N, E, device=dev).bfloat16() for _ in range(4))
    kT, vT = (t.permute(1, 2, 0).contiguous() for t in (k, v))
    mask = torch.rand(Lq, Lk, device=dev) < 0.5
    mask[:, 0] = False
    out, lse = torch.empty(Lq, N, E, device=dev, dtype=torch.bfloat16), torch.empty(N, H, Lq, device=dev)
    qT, doT = (torch.empty(N, E, LqP, device=dev, dtype=torch.bfloat16) for _ in range(2))
    delta = torch.empty(N, H, Lq, device=dev)
    dq, dk, dv = (torch.empty(Lq, N, E, device=dev, dtype=torch.bfloat16) for _ in range(3))
    ws = torch.empty(lib.mpf_attn_workspace_bytes(Lq, Lk, N, H), dtype=torch.uint8, device=dev)
    aux = torch.empty(lib.mpf_attn_bwd_aux_bytes(Lq, Lk, N, H, 1), dtype=torch.uint8, device=dev)
    scale = 32 ** -0.5
    entries = {
        "mpf_attn_forward_kv": (q.data_ptr(), k.data_ptr(), 0, 0, vT.data_ptr(), mask.data_ptr(), 0, out.data_ptr(), lse.data_ptr(), Lq, Lk, N,
                                H, 32, scale, ws.data_ptr(), ws.numel(), st),
        "mpf_attn_bwd_prep_aux": (q.data_ptr(), do.data_ptr(), out.data_ptr(), lse.data_ptr(), mask.data_ptr(), 0, Lk, qT.data_ptr(),
                                  doT.data_ptr(), delta.data_ptr(), aux.data_ptr(), aux.numel(), Lq, LqP, N, H, st),
        "mpf_attn_backward_kv_aux": (q.data_ptr(), k.data_ptr(), v.data_ptr(), 0, 0, kT.data_ptr(), qT.data_ptr(), do.data_ptr(), doT.data_ptr(),
                                     mask.data_ptr(), 0, lse.data_ptr(), delta.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), 0, 0,
                                     Lq, LqP, Lk, N, H, 32, scale, ws.data_ptr(), ws.numel(), aux.data_ptr(), st),
    }
    for name, args in entries.items():                    # (in this order: each entry's inputs are the one before's outputs)
        fn = getattr(lib, name)
        for _ in range(200):
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
            print(json.dumps({"what": f"host us per {name} call (Lq = Lk = 120, N = 2, H = 8)", "calls": calls, "us_per_call": round(us, 3),
                              "kernel": _lib.last_kernel(), "lib": _lib.LIB_PATH}), flush=True)


if __name__ == "__main__":
    main()
