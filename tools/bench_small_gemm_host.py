#!/usr/bin/env python3
"""Host time per call of the small-row GEMM host layer (fill, check, route, launch): 2 000 back-to-back calls between two stream
synchronisations, timed with the host clock, median of 5 — of mpf_small_gemm_bf16 at (I, J, Kc) = (16, 16, 32), one block, so the
device keeps up and the loop is paced by the launch thread, and of one decoder layer forward + backward (decoder_layer() of
mp_former_amd/decoder_layer.py and autograd's backward through it: the two native calls and the Python wrapper around them, which is
the same for every build of the library) at the smallest case of tests/test_decoder_layer_direct_gpu.py.  Prints
one JSON line per row.  A/B two builds with MPF_LIB_PATH (tools/ab_lib.sh)."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from mp_former_amd import _lib  # noqa: E402


def _timed(what, fn, calls, repeats):
    for _ in range(200):
        fn()
    us = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / calls * 1e6)
    print(json.dumps({"what": what, "calls": calls, "us_per_call": round(statistics.median(us), 3), "min": round(min(us), 3),
                      "max": round(max(us), 3), "kernel": _lib.last_kernel(), "lib": _lib.LIB_PATH}), flush=True)


def main(calls=2000, repeats=5):
    import test_decoder_layer_direct_gpu as D
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    a, b = torch.randn(16, 32, device=dev).bfloat16(), torch.randn(16, 32, device=dev).bfloat16()
    c = torch.empty(16, 16, dtype=torch.bfloat16, device=dev)
    fn = _lib.lib().mpf_small_gemm_bf16
    args = (a.data_ptr(), 32, 1, None, b.data_ptr(), 32, 1, None, None, 0, c.data_ptr(), 16, None, 16, 16, 32, 0, _lib.stream_ptr(dev))
    _lib.check(fn(*args), "mpf_small_gemm_bf16")
    _timed("host us per mpf_small_gemm_bf16 call (16, 16, 32)", lambda: fn(*args), calls, repeats)

    P = D._problem(D.CASES[0])
    seeds = [P[s].to(dev) for s in D.SEEDS]

    from mp_former_amd.decoder_layer import decoder_layer
    T = D._forward_native(P, dev)               # (the leaves on the device, made once)
    mask_c = P["mask_c"].to(dev)
    assert P["case"][5] is None and P["mask_s"] is None

    def layer():
        outs = decoder_layer(T["x0"], T["xb0"], T["Kp"], T["Vp"], mask_c, None, D.H, D.EPS, T["params"], None)
        torch.autograd.backward(list(outs), seeds)

    _timed("host us per decoder layer forward + backward (Qt 1, N 1, S 8, F 32)", layer, calls, repeats)


if __name__ == "__main__":
    main()
