#!/usr/bin/env python3
"""Video training input: the tube masks of a YouTube-VIS-like clip batch by three routes to the same padded [P, Hc, Wc] store.

    python tools/bench_clip_input.py     B clips of F frames, 720 x 1280 sources with G instances each as RLE, short edge 480
                                         (480 x 853) on a 480 x 864 canvas, a flipped and an unflipped clip; P = B * G * F planes

Time per call: events around blocks of back-to-back calls, the routes alternated in one process after a warm-up, median
(min - max) over the rounds; then the kernel alone by the library's launch profiler, next to the bytes it cannot go below
(P * Hc * Wc written + the source words read).

The routes from the packed masks (``inference.rle_bits``, timed on its own: every device route needs it) to the store:
  native                resample_mask_bits: one staging copy, one launch, no dense intermediate
  torch on the device   unpack_masks (dense at the source size), index_select by the same two tables, flip, a copy into a zeroed
                        canvas: three dense intermediates per plane
  host, one thread      the reference mapper's work restated: a numpy RLE decode, PIL's NEAREST resize, the flip, the pad, np.stack,
                        then the upload of the P dense planes.  A CPU time, not a like-for-like GPU time
"device ops" is the number of kernels, memsets and copies a route enqueues per call, counted in the route's own code.

Needs a GPU: there is no fallback.  Shapes other than these are not measured."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="back-to-back calls per timed block")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--clips", type=int, default=2)
    ap.add_argument("--frames", type=int, default=2)
    ap.add_argument("--instances", type=int, default=6)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_clip_input.py needs a GPU")
    from mp_former_amd import _lib
    from mp_former_amd import augment as A
    from mp_former_amd import clip_input as CI
    from mp_former_amd.inference import rle_bits, unpack_masks
    try:
        from PIL import Image
    except ImportError:
        Image = None
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")

    def events(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / reps

    def clock(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    H, W, B, F, G = 720, 1280, args.clips, args.frames, args.instances
    rh, rw = A.shortest_edge_size(H, W, 480, 1333)
    canvas = ((rh + 31) // 32 * 32, (rw + 31) // 32 * 32)
    g = np.random.default_rng(0)
    yy, xx = np.mgrid[:H, :W]

    def encode(m):
        flat = m.T.reshape(-1)
        edges = np.flatnonzero(flat[1:] != flat[:-1]) + 1
        counts = np.diff(np.concatenate([[0], edges, [flat.size]])).tolist()
        return {"size": [H, W], "counts": ([0] if flat[0] else []) + counts}

    def decode(r):
        c = np.asarray(r["counts"])
        return np.repeat(np.arange(len(c)) % 2 == 1, c).reshape(W, H).T

    samples, rles, params = [], [], []
    for b in range(B):
        clip = tuple(A.SemSegParams((H, W), (rh, rw), (0, 0), (rh, rw), (rh, rw), b % 2 == 1, canvas) for _ in range(F))
        annos = []
        for f in range(F):
            frame = []
            for i in range(G):                               # ellipses that drift from frame to frame
                cy, cx, ry, rx = g.uniform(0.2, 0.8) * H, g.uniform(0.2, 0.8) * W, g.uniform(0.05, 0.3) * H, g.uniform(0.05, 0.3) * W
                m = ((yy - cy - 8 * f) / ry) ** 2 + ((xx - cx - 12 * f) / rx) ** 2 <= 1.0
                frame.append({"id": 10 * b + i, "category_id": i % 40, "iscrowd": 0, "segmentation": encode(m)})
                rles.append(frame[-1]["segmentation"])
                params.append(clip[f])
            annos.append(frame)
        samples.append({"image_raw": [torch.from_numpy(g.integers(0, 256, size=(H, W, 3), dtype=np.uint8)) for _ in range(F)],
                        "clip": clip, "annotations": annos, "num_classes": 40})
    P = len(rles)
    bits = rle_bits(rles, (H, W), device=dev)
    planes = [(bits[i], (H, W), params[i]) for i in range(P)]
    ty = torch.from_numpy(A.nearest_table_pil(H, rh)).to(dev)
    tx = torch.from_numpy(A.nearest_table_pil(W, rw)).to(dev)
    flipped = torch.tensor([p.flip for p in params], device=dev)
    ops = {}

    def native():
        ops["native"] = 3                                    # the staging copy, the memset of the areas, the kernel
        return CI.resample_mask_bits(planes, canvas, device=dev)[0]

    def torch_route():
        dense = unpack_masks(bits, (H, W))                                       # 1
        small = dense.index_select(1, ty).index_select(2, tx)                    # 2, 3
        small = torch.where(flipped[:, None, None], small.flip(2), small)        # 4, 5
        out = torch.zeros((P,) + canvas, dtype=torch.bool, device=dev)           # 6
        out[:, :rh, :rw] = small                                                 # 7
        ops["torch"] = 7
        return out

    def host_route():
        out = np.zeros((P,) + canvas, dtype=bool)
        for i, (r, p) in enumerate(zip(rles, params)):
            m = np.asarray(Image.fromarray(decode(r).astype(np.uint8)).resize((rw, rh), Image.NEAREST))
            out[i, :rh, :rw] = m[:, ::-1] if p.flip else m
        ops["host"] = 1                                      # the upload
        return torch.from_numpy(out).to(dev)

    def packed():
        return rle_bits(rles, (H, W), device=dev)

    def whole():
        return CI.clip_batch(samples, device=dev)

    want = native()
    assert torch.equal(want, torch_route()), "the native and the torch route differ"
    routes = [("rle_bits: the RLE counts to packed bits (every device route starts here)", packed, events, "-"),
              ("native: resample_mask_bits", native, events, "native"),
              ("torch on the device: unpack_masks, index_select x 2, flip, padded copy", torch_route, events, "torch")]
    if Image is not None:
        assert torch.equal(want, host_route()), "the native and the host route differ"
        routes.append(("host, one thread: decode + PIL NEAREST + flip + pad + upload (CPU time)", host_route, clock, "host"))
    routes.append((f"clip_batch end to end: {B * F} frames resized, rle_bits, the masks, its one read-back per clip (host clock)", whole, clock, "-"))
    for _, fn, timer, _ in routes:
        timer(fn, 2)
    times = [[] for _ in routes]
    for _ in range(args.rounds):
        for t, (_, fn, timer, _) in zip(times, routes):
            t.append(timer(fn, args.reps))
    _lib.profile_enable(True)
    for _ in range(args.reps):
        native()
    torch.cuda.synchronize()
    n, ms, by = _lib.profile_get("mask_bits_resample_kernel")
    _lib.profile_enable(False)
    floor = P * canvas[0] * canvas[1] + P * ((H * W + 63) // 64) * 8
    assert abs(by / n - floor) < 1, (by / n, floor)
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {args.reps} back-to-back calls per block, {args.rounds} alternated "
          f"rounds, median (min - max) ms per call")
    print(f"# {B} clips x {F} frames x {G} instances = {P} planes, {H} x {W} -> {rh} x {rw} on a {canvas[0]} x {canvas[1]} canvas")
    print("| route | ms / call | device ops |")
    print("|---|---|---|")
    for (name, _, _, key), t in zip(routes, times):
        print(f"| {name} | {statistics.median(t):.3f} ({min(t):.3f} - {max(t):.3f}) | {ops.get(key, '-')} |")
    print(f"# mask_bits_resample_kernel alone: {ms / n:.4f} ms; it cannot move fewer than {floor / 1e6:.2f} MB ({P * canvas[0] * canvas[1] / 1e6:.2f} MB "
          f"written + {P * ((H * W + 63) // 64) * 8 / 1e6:.2f} MB of source words): {floor / (ms / n) / 1e6:.0f} GB/s of that")
    dense = P * H * W + P * rh * W + 3 * P * rh * rw
    print(f"# the torch route writes {dense / 1e6:.2f} MB of dense intermediates besides the store")


if __name__ == "__main__":
    main()
