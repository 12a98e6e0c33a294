#!/usr/bin/env python3
"""Large-scale-jitter training input: the native route (augment.resample_images / augment.lsj_batch, csrc/img_resample.hip: the
decoded source, a few KB of tables and vertices cross to the device; only the crop window is computed) against two other ways to
the same batch, for B = 16 sources of 480 x 640, crop size S = 1024, at the scales 0.1, 1.0 and 2.0 (one scale per batch, crop draw
0.5, every second image flipped, 7 polygon instances per image).

    python tools/bench_lsj.py     time per batch: events (or, for the host route, a host clock ending in a synchronise) around
                                  blocks of back-to-back batches, the routes alternated in one process after a warm-up of every
                                  shape, median (min - max) over the rounds; then the kernel alone by the library's launch profiler

The routes:
  native images        resample_images on pinned host sources: upload of the sources, tables, one launch -> uint8 [B, 3, S, S]
  native batch         lsj_batch: the same plus the polygons (transform, polygon_bits, unpack_masks) -> images and bool masks
  torch on the device  upload of the sources, then per image flip, F.interpolate(mode="bilinear", antialias=True) of the WHOLE image,
                       crop, pad, round to uint8.  NOT value-equal to PIL (float weights, no uint8 rounding between the passes): a
                       time for the same shape of work with stock kernels, not a replacement
  host, one thread     the reference mapper's image work restated (PIL resize of the flipped image, crop, pad with 128, HWC -> CHW)
                       on ONE CPU thread, then the upload of the image and of T dense S x S masks.  A CPU time, not a like-for-like
                       GPU comparison; the rasterisation of the masks (pycocotools) is NOT in it, so it is a lower bound of that route

Needs a GPU: there is no fallback.  Shapes other than these are not measured."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, S, T = 16, 480, 640, 1024, 7
SCALES = (0.1, 1.0, 2.0)
MEAN, STD = [123.675, 116.280, 103.530], [58.395, 57.120, 57.375]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="back-to-back batches per timed block")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        sys.exit("bench_lsj.py needs a GPU")
    from mp_former_amd import _lib
    from mp_former_amd import augment as A
    from tools.bench_mask_codec import polygons
    try:
        from PIL import Image
    except ImportError:
        Image = None
    torch.set_num_threads(1)
    dev = torch.device("cuda:0")
    g = np.random.default_rng(0)
    sources = [torch.from_numpy(g.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).pin_memory() for _ in range(B)]
    annos = [[{"category_id": m, "iscrowd": 0, "segmentation": rings} for m, rings in enumerate(polygons(T, H, W, seed=b))] for b in range(B)]

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

    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; B = {B} sources of {H} x {W}, S = {S}, {T} instances per image; "
          f"{args.reps} back-to-back batches per block, {args.rounds} alternated rounds, median (min - max) ms per batch")
    print("# 'torch on the device' is NOT value-equal to PIL; 'host, one thread' is a CPU time without the mask rasterisation")
    print("| scale | resized | route | host-to-device bytes per sample | ms / batch | kernel alone, ms |")
    print("|---|---|---|---|---|---|")
    for scale in SCALES:
        params = [A.lsj_params(H, W, b % 2 == 1, scale, 0.5, S) for b in range(B)]
        samples = [{"image_raw": s, "lsj": p, "annotations": a} for s, p, a in zip(sources, params, annos)]
        p0 = params[0]
        tables = sum(a.nbytes for p in (p0,) for a in (*A.resample_coeffs(W, p.resized[1], p.offset[1], p.valid[1]),
                                                       *A.resample_coeffs(H, p.resized[0], p.offset[0], p.valid[0]))) + 4 * A._REC_WORDS
        verts = sum(8 * len(r) for a in annos[0] for r in a["segmentation"])
        pad_dev = torch.full((3, S, S), 128, dtype=torch.uint8, device=dev)

        def native_images():
            return A.resample_images(sources, params, device=dev)

        def native_batch():
            return A.lsj_batch(samples, device=dev)

        def torch_device():
            out = []
            for s, p in zip(sources, params):
                x = s.to(dev, non_blocking=True).permute(2, 0, 1)[None].float()
                if p.flip:
                    x = x.flip(-1)
                x = F.interpolate(x, size=p.resized, mode="bilinear", antialias=True, align_corners=False)[0]
                x = x[:, p.offset[0]:p.offset[0] + p.valid[0], p.offset[1]:p.offset[1] + p.valid[1]]
                o = pad_dev.clone()
                o[:, :p.valid[0], :p.valid[1]] = x.round().clamp(0, 255).to(torch.uint8)
                out.append(o)
            return torch.stack(out)

        masks_host = torch.zeros((T, S, S), dtype=torch.uint8)

        def host_route():
            out = []
            for s, p in zip(sources, params):
                a = s.numpy()
                if p.flip:
                    a = a[:, ::-1]
                a = np.asarray(Image.fromarray(np.ascontiguousarray(a)).resize((p.resized[1], p.resized[0]), Image.BILINEAR))
                a = a[p.offset[0]:p.offset[0] + p.valid[0], p.offset[1]:p.offset[1] + p.valid[1]]
                o = np.full((S, S, 3), 128, dtype=np.uint8)
                o[:a.shape[0], :a.shape[1]] = a
                out.append((torch.as_tensor(np.ascontiguousarray(o.transpose(2, 0, 1))).to(dev), masks_host.to(dev)))
            return out

        routes = [("native images", native_images, events, H * W * 3 + tables, True),
                  ("native batch (images + masks)", native_batch, events, H * W * 3 + tables + verts, True),
                  ("torch on the device (not value-equal)", torch_device, events, H * W * 3, False)]
        if Image is not None:
            routes.append(("host, one thread: PIL + upload (CPU time, no rasterisation)", host_route, clock, 3 * S * S + T * S * S, False))
            got, want = native_images(), torch.stack([o for o, _ in host_route()])
            assert torch.equal(got, want), "the native route and PIL differ"
        else:
            print("# PIL does not import here: the host route is not measured")
        diff = (native_images().int() - torch_device().int()).abs()
        print(f"# scale {scale}: native == PIL route: {Image is not None}; |native - torch antialias| max {int(diff.max())}, "
              f"differing bytes {float((diff > 0).float().mean()) * 100:.1f} %")
        for _, fn, timer, _, _ in routes:
            timer(fn, 2)
        times = [[] for _ in routes]
        for _ in range(args.rounds):
            for t, (_, fn, timer, _, _) in zip(times, routes):
                t.append(timer(fn, args.reps))
        for t, (name, fn, timer, nbytes, native) in zip(times, routes):
            alone = "-"
            if native:
                _lib.profile_enable(True)
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                n, ms, by = _lib.profile_get("img_resample_kernel")
                _lib.profile_enable(False)
                assert n == args.reps, n
                alone = f"img_resample_kernel {ms / n:.3f} ({by / n / (ms / n) / 1e6:.0f} GB/s of output written)"
            print(f"| {scale} | {p0.resized[0]} x {p0.resized[1]} | {name} | {nbytes} | {statistics.median(t):.2f} ({min(t):.2f} - {max(t):.2f}) | {alone} |")
    # the normalised forms at the largest scale: what the model's own (x - mean) / std and ImageList padding would add
    params = [A.lsj_params(H, W, b % 2 == 1, 2.0, 0.5, S) for b in range(B)]
    srcs = [s.to(dev) for s in sources]
    for dtype in (torch.uint8, torch.float32, torch.bfloat16):
        fn = lambda: A.resample_images(srcs, params, dtype=dtype, mean=MEAN, std=STD)      # noqa: E731
        events(fn, 2)
        t = [events(fn, args.reps) for _ in range(args.rounds)]
        print(f"# scale 2.0, sources already on the device, output {dtype}: {statistics.median(t):.2f} ({min(t):.2f} - {max(t):.2f}) ms / batch")


if __name__ == "__main__":
    main()
