#!/usr/bin/env python3
"""COCO ground truth to packed mask bits: the native routes from the annotation's own form (inference.polygon_bits and
inference.rle_bits, csrc/seg_codec.hip: only vertices or run lengths cross to the device) against the only route there was before
them, dense uint8 masks uploaded and packed (``pack_masks``), for COCO-like batches of 7 and 40 objects at 800 x 1216 and
1024 x 1024.

    python tools/bench_mask_codec.py      time per call: events around blocks of back-to-back calls (a call's host side and its
                                          host-to-device copy are inside the block), the routes alternated in one process, median
                                          over the rounds; then the kernels alone by the library's launch profiler; the routes'
                                          results are compared first

The dense route starts from masks that ALREADY exist on the host: rasterising them (pycocotools' frPyObjects + decode on the
loader's CPU) is not timed, because pycocotools is not a dependency of this repository.  Its figure is therefore a lower bound on the
old route.  The native routes start from the python lists a json holds, so their figures include flattening those lists.

Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ((7, 800, 1216), (40, 800, 1216), (7, 1024, 1024), (40, 1024, 1024))


def polygons(M, H, W, seed):
    """M objects as a COCO json holds them: one ring each (every fourth object two) of 12 - 80 vertices on a jittered ellipse, two
    decimals as annotation tools write them"""
    import numpy as np
    g = np.random.default_rng(seed)
    objs = []
    for m in range(M):
        rings = []
        for _ in range(2 if m % 4 == 3 else 1):
            k = int(g.integers(12, 81))
            cx, cy = g.uniform(0.15 * W, 0.85 * W), g.uniform(0.15 * H, 0.85 * H)
            rx, ry = g.uniform(0.03 * W, 0.3 * W), g.uniform(0.03 * H, 0.3 * H)
            t = np.sort(g.uniform(0, 2 * np.pi, k))
            r = g.uniform(0.75, 1.0, k)
            xy = np.stack([np.clip(cx + rx * r * np.cos(t), 0, W), np.clip(cy + ry * r * np.sin(t), 0, H)], axis=1)
            rings.append(np.round(xy, 2).reshape(-1).tolist())
        objs.append(rings)
    return objs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="back-to-back calls per timed block")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mask_codec.py needs a GPU")
    from mp_former_amd import _lib
    from mp_former_amd import inference as I
    dev = torch.device("cuda:0")

    def block(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / reps

    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {args.reps} back-to-back calls per block, {args.rounds} "
          f"alternated rounds, median (min - max); a call includes its host side and its host-to-device copy")
    print("# the dense route EXCLUDES the CPU rasterisation of the masks it uploads: a lower bound on the old route")
    print("| objects, size | route | host-to-device bytes | us / call | kernels alone, us |")
    print("|---|---|---|---|---|")
    for M, H, W in SCENES:
        polys = polygons(M, H, W, seed=M * 10000 + H)
        bits = I.polygon_bits(polys, (H, W), device=dev)
        rles = I.bits_rle(bits, (H, W))                              # the same masks as uncompressed and compressed run lengths
        texts = [I.rle_compress(r) for r in rles]
        dense_host = I.unpack_masks(bits, (H, W), dtype=torch.uint8).cpu()      # what a CPU rasteriser would have produced
        assert torch.equal(I.rle_bits(rles, device=dev), bits) and torch.equal(I.rle_bits(texts, device=dev), bits)
        assert torch.equal(I.pack_masks(dense_host.to(dev)), bits) and bool(bits.any())
        xy, ring_off, ring_obj = I._ring_arrays(polys, "bench")
        counts, off, _ = I._rle_arrays(rles, H, W, "bench")
        routes = (
            ("dense uint8 upload + pack_masks", lambda: I.pack_masks(dense_host.to(dev)), dense_host.numel(), ("seg_pack_masks_kernel",)),
            ("polygon_bits", lambda: I.polygon_bits(polys, (H, W), device=dev), xy.nbytes + ring_off.nbytes + ring_obj.nbytes,
             ("seg_poly_toggles_kernel", "seg_toggles_fill_kernel")),
            ("rle_bits, counts as lists", lambda: I.rle_bits(rles, device=dev), counts.nbytes + off.nbytes + 4 * M,
             ("seg_rle_toggles_kernel", "seg_toggles_fill_kernel")),
            ("rle_bits, counts as strings", lambda: I.rle_bits(texts, device=dev), counts.nbytes + off.nbytes + 4 * M,
             ("seg_rle_toggles_kernel", "seg_toggles_fill_kernel")),
        )
        for _, fn, _, _ in routes:
            block(fn, 3)
        times = [[] for _ in routes]
        for _ in range(args.rounds):
            for t, (_, fn, _, _) in zip(times, routes):
                t.append(block(fn, args.reps))
        for t, (name, fn, nbytes, kernels) in zip(times, routes):
            _lib.profile_enable(True)
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
            alone = []
            for k in kernels:
                n, ms, _ = _lib.profile_get(k)
                assert n == args.reps, (k, n)
                alone.append(f"{k} {ms * 1e3 / n:.1f}")
            _lib.profile_enable(False)
            print(f"| {M}, {H} x {W} | {name} | {nbytes} | {statistics.median(t):.0f} ({min(t):.0f} - {max(t):.0f}) | {', '.join(alone)} |")
        med = [statistics.median(t) for t in times]
        print(f"# {M} objects at {H} x {W}: dense (without its rasterisation) / polygon_bits = {med[0] / med[1]:.1f}, / rle_bits = "
              f"{med[0] / med[2]:.1f}; bytes {routes[0][2] / routes[1][2]:.0f}x and {routes[0][2] / routes[2][2]:.0f}x fewer")


if __name__ == "__main__":
    main()
