#!/usr/bin/env python3
"""Bounding boxes of instance masks: the torch route on dense masks (``any`` over each axis, then the first and last set index,
what Detectron2's ``BitMasks.get_bounding_boxes`` computes per mask and what the reference's instance_inference leaves commented
out as slow, maskformer_model.py:393-395) against the native route on packed bits (inference.mask_boxes, csrc/seg_box.hip, one
launch), at T = 100 masks of 1024 x 1024.

    python tools/bench_mask_boxes.py      time per call: events around blocks of back-to-back calls (a call's host side is inside
                                          the block), the two routes alternated in one process, median over the rounds; then the
                                          native kernel alone by the library's launch profiler (events around the launch); the
                                          two routes' results are compared first

The dense masks are the fp32 0 / 1 [T, H, W] tensor ``postprocess`` returns; the bits are those ``instance_bits`` returns.  Packing
is not part of either route: a caller has one form or the other.

Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T, H, W = 100, 1024, 1024


def setup(dev):
    """-> dense fp32 [T, H, W]: a filled ellipse per mask (seeded), every tenth with a far-away pixel, one mask empty"""
    import numpy as np
    import torch
    g = np.random.default_rng(1024)
    ys, xs = torch.arange(H, device=dev)[:, None], torch.arange(W, device=dev)[None, :]
    dense = torch.zeros((T, H, W), dtype=torch.float32, device=dev)
    for t in range(1, T):
        cy, cx = int(g.integers(H // 8, 7 * H // 8)), int(g.integers(W // 8, 7 * W // 8))
        ry, rx = int(g.integers(8, H // 3)), int(g.integers(8, W // 3))
        dense[t] = ((((ys - cy) / ry) ** 2 + ((xs - cx) / rx) ** 2) <= 1).float()
        if t % 10 == 0:
            dense[t, int(g.integers(0, H)), int(g.integers(0, W))] = 1
    return dense


def torch_route(dense):
    """``any`` over each axis, then the first / last index: int64 [T, 4] XYXY, zeros for an empty mask"""
    import torch
    m = dense > 0
    cols, rows = m.any(1), m.any(2)                      # [T, W], [T, H]
    x0, y0 = cols.int().argmax(1), rows.int().argmax(1)
    x1 = W - cols.flip(1).int().argmax(1)
    y1 = H - rows.flip(1).int().argmax(1)
    boxes = torch.stack([x0, y0, x1, y1], dim=1)
    return boxes * cols.any(1)[:, None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100, help="back-to-back calls per timed block")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mask_boxes.py needs a GPU")
    from mp_former_amd import _lib
    from mp_former_amd.inference import mask_boxes, pack_masks
    dev = torch.device("cuda:0")
    dense = setup(dev)
    bits = pack_masks(dense)
    want, got = torch_route(dense), mask_boxes(bits, (H, W))
    assert _lib.last_kernel() == "seg_bits_boxes_kernel", _lib.last_kernel()
    assert torch.equal(want.int(), got), "the two routes disagree"
    assert got[0].tolist() == [0, 0, 0, 0] and (got[1:, 2] > got[1:, 0]).all()

    def block(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / reps

    def native():
        return mask_boxes(bits, (H, W))

    def torch_():
        return torch_route(dense)

    for fn in (torch_, native):
        block(fn, 10)
    t_torch, t_native = [], []
    for _ in range(args.rounds):
        t_torch.append(block(torch_, args.reps))
        t_native.append(block(native, args.reps))
    tt, tn = statistics.median(t_torch), statistics.median(t_native)
    # the kernel alone: the library's launch profiler puts its events around the launch, inside the call.  A call is short enough
    # that the block figure above can be the host's rate of issuing calls (tensor checks, an allocation, ctypes) and not the device's.
    _lib.profile_enable(True)
    for _ in range(args.reps):
        native()
    torch.cuda.synchronize()
    n_launch, ms, nbytes = _lib.profile_get("seg_bits_boxes_kernel")
    _lib.profile_enable(False)
    assert n_launch == args.reps and nbytes == args.reps * (bits.numel() * 8 + 16 * T), (n_launch, nbytes)
    tk = ms * 1e3 / n_launch
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; T = {T} masks of {H} x {W}; {args.reps} back-to-back calls per "
          f"block, {args.rounds} alternated rounds, median (min - max); a call includes its host side")
    print("| route | input | bytes read | us / call | bytes / call time, GB/s |")
    print("|---|---|---|---|---|")
    print(f"| torch: any over each axis, first / last index | dense fp32 [T, H, W] | {dense.numel() * 4} | {tt:.1f} ({min(t_torch):.1f} - "
          f"{max(t_torch):.1f}) | {dense.numel() * 4 / tt / 1e3:.0f} |")
    print(f"| native: mask_boxes (seg_bits_boxes_kernel) | packed bits int64 [T, nwords] | {bits.numel() * 8} | {tn:.1f} ({min(t_native):.1f} - "
          f"{max(t_native):.1f}) | {bits.numel() * 8 / tn / 1e3:.0f} |")
    print(f"# torch / native, per call = {tt / tn:.1f}")
    print(f"# seg_bits_boxes_kernel alone, events around the launch (launch profiler, mean of {n_launch}): {tk:.1f} us, "
          f"{nbytes / n_launch / tk / 1e3:.0f} GB/s of algorithmic bytes")


if __name__ == "__main__":
    main()
