#!/usr/bin/env python3
"""Host time per call of the gemm3 host layer (fill, route, launch): 2 000 back-to-back mpf_gemm3_tn_h2 calls at
(M, N, K) = (128, 256, 32) — small, so the device keeps up and the loop is paced by the launch thread — between two stream
synchronisations, timed with the host clock.  Prints one JSON line per repeat.  A/B two builds with MPF_LIB_PATH
(tools/ab_lib.sh)."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mp_former_amd import _lib  # noqa: E402
from mp_former_amd.gemm3 import amax, split_weights_grouped_h2  # noqa: E402


def main(calls=2000, repeats=5):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    M, N, K = 128, 256, 32
    a = torch.randn(M, K, device=dev)
    (planes, w_am), = split_weights_grouped_h2([([torch.randn(N, K, device=dev)], False)])
    a_am = amax(a)
    c = torch.empty(M, N, device=dev)
    fn = _lib.lib().mpf_gemm3_tn_h2
    st = _lib.stream_ptr(dev)
    args = (a.data_ptr(), a.stride(0), a_am.data_ptr(), planes.data_ptr(), w_am.data_ptr(), None, None, 0, None, 0, None, 0,
            c.data_ptr(), c.stride(0), None, M, N, K, 0, st)
    for _ in range(200):
        _lib.check(fn(*args), "mpf_gemm3_tn_h2")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn(*args)
        torch.cuda.synchronize()
        us = (time.perf_counter() - t0) / calls * 1e6
        print(json.dumps({"what": "host us per mpf_gemm3_tn_h2 call (128, 256, 32)", "calls": calls, "us_per_call": round(us, 3),
                          "kernel": _lib.last_kernel(), "lib": _lib.LIB_PATH}), flush=True)


if __name__ == "__main__":
    main()
