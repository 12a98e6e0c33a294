#!/usr/bin/env python3
"""Training input from label maps: the three kernels of csrc/label_input.hip at the real shapes, against two other ways to the same
result.

    python tools/bench_label_input.py     panoptic: a 480 x 640 panoptic PNG, large-scale jitter to a 1024 x 1024 crop at scale 2.0,
                                          T in {20, 60, 100} segments; semantic: a 512 x 683 class map, crop 512 x 512, K = 150, ten
                                          candidate windows

Time per call: events around blocks of back-to-back calls, the routes alternated in one process after a warm-up of every shape,
median (min - max) over the rounds; then the kernels alone by the library's launch profiler.

The routes to the packed masks of one image:
  native                label_bits: one read of the id map whatever T is, the cleared output, the non-zero words
  torch on the device   torch.stack([m == k for k in ids]) then inference.pack_masks: T compare passes, T dense planes, one pack
  host, one thread      the reference mapper's work restated: PIL nearest resize of the PNG, crop, pad, rgb2id, one ``== id`` plane
                        per segment, np.stack, then the upload of the T dense planes.  A CPU time, not a like-for-like GPU time

Needs a GPU: there is no fallback.  Shapes other than these are not measured."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

S = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10, help="back-to-back calls per timed block")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_label_input.py needs a GPU")
    from mp_former_amd import _lib
    from mp_former_amd import augment as A
    from mp_former_amd import label_input as LI
    from mp_former_amd.inference import pack_masks
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

    def measure(routes):
        for _, fn, timer in routes:
            timer(fn, 2)
        times = [[] for _ in routes]
        for _ in range(args.rounds):
            for t, (_, fn, timer) in zip(times, routes):
                t.append(timer(fn, args.reps))
        return [f"{statistics.median(t):.3f} ({min(t):.3f} - {max(t):.3f})" for t in times]

    def alone(fn, kernel):
        _lib.profile_enable(True)
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        n, ms, by = _lib.profile_get(kernel)
        _lib.profile_enable(False)
        return f"{ms / n:.4f} ms, {by / n / 1e6:.2f} MB counted, {by / n / (ms / n) / 1e6:.0f} GB/s"

    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {args.reps} back-to-back calls per block, {args.rounds} alternated "
          f"rounds, median (min - max) ms per call")
    # ---- panoptic: 480 x 640 -> scale 2.0 of 1024 -> crop 1024 x 1024 ----------------------------------------------------------------
    H, W = 480, 640
    g = np.random.default_rng(0)
    yy, xx = np.mgrid[:H, :W]
    p = A.lsj_params(H, W, True, 2.0, 0.5, S)
    print("| workload | route | ms / call | kernel alone |")
    print("|---|---|---|---|")
    for T in (20, 60, 100):
        cells = int(np.ceil(np.sqrt(T)))
        seg = (yy * cells // H) * cells + xx * cells // W                        # a grid of about T segments
        ids = 1000 * (seg + 1) + 70000 * (seg % 3)
        wanted = [int(v) for v in np.unique(ids)[:T]]
        png = np.stack([ids % 256, (ids // 256) % 256, ids // 65536], axis=2).astype(np.uint8)
        src = torch.from_numpy(png).to(dev)
        id_map = LI.resample_labels([src], [p], "rgb", LI.PANOPTIC_PAD_ID, device=dev)[0]

        def native_resample():
            return LI.resample_labels([src], [p], "rgb", LI.PANOPTIC_PAD_ID, device=dev)

        def native_bits():
            return LI.label_bits(id_map, wanted)

        def torch_bits():
            return pack_masks(torch.stack([id_map == k for k in wanted]))

        def host_route():
            a = png[:, ::-1] if p.flip else png
            a = np.asarray(Image.fromarray(np.ascontiguousarray(a)).resize((p.resized[1], p.resized[0]), Image.NEAREST))
            a = a[p.offset[0]:p.offset[0] + p.valid[0], p.offset[1]:p.offset[1] + p.valid[1]]
            o = np.full((S, S, 3), 255, dtype=np.uint8)
            o[:a.shape[0], :a.shape[1]] = a
            o = o.astype(np.int64)
            pan = o[..., 0] + 256 * o[..., 1] + 65536 * o[..., 2]
            return torch.from_numpy(np.stack([pan == k for k in wanted])).to(dev)

        assert torch.equal(native_bits()[0], torch_bits()), "label_bits and the torch route differ"
        routes = [("label_bits", native_bits, events), ("torch: stack of == then pack_masks", torch_bits, events)]
        if Image is not None:
            assert torch.equal(pack_masks(host_route()), native_bits()[0]), "label_bits and the host route differ"
            routes.append(("host, one thread: PIL + numpy masks + upload (CPU time)", host_route, clock))
        if T == 20:
            routes.insert(0, ("resample_labels (RGB PNG, one image)", native_resample, events))
        res = measure(routes)
        nw = (S * S + 63) // 64
        for (name, fn, _), r in zip(routes, res):
            k = "-"
            if name.startswith("label_bits"):
                k = alone(fn, "label_bits_kernel") + f" (map {S * S * 4 / 1e6:.1f} MB read + bits {T * nw * 8 / 1e6:.1f} MB cleared)"
            elif name.startswith("resample_labels"):
                k = alone(fn, "label_resample_kernel")
            print(f"| panoptic {S} x {S}, T = {T} | {name} | {r} | {k} |")
    # ---- semantic: 512 x 683 -> crop 512 x 512, K = 150 ---------------------------------------------------------------------------
    K, H, W, C = 150, 512, 683, 512
    lab = g.integers(0, K, size=(H // 16 + 1, W // 16 + 1)).astype(np.uint8).repeat(16, 0).repeat(16, 1)[:H, :W].copy()
    lab[g.random((H, W)) < 0.05] = 255
    src = torch.from_numpy(lab).to(dev)
    rs = np.random.RandomState(0)
    d = A.draw_semseg(H, W, (512, 512), 2048, "choice", crop=(C, C), single_category_max_area=0.75, size_divisibility=C, rng=rs)
    windows = [[(y0, x0, C, C) for (y0, x0) in d.origins]]

    def native_counts():
        return LI.window_counts([src], [d], windows, K, 255, device=dev)

    counts = native_counts().numpy()[0]
    i = A.choose_category_crop(counts, len(d.origins), 0.75)
    q = d.params(i)
    classes = np.nonzero(counts[i])[0]
    id_map = LI.resample_labels([src], [q], "u8", 255, device=dev)[0]

    def native_resample():
        return LI.resample_labels([src], [q], "u8", 255, device=dev)

    def native_bits():
        return LI.label_bits(id_map, classes)

    def torch_bits():
        return pack_masks(torch.stack([id_map == int(k) for k in classes]))

    def host_route():
        full = lab.astype(np.float64)[A.nearest_table_torch(H, q.resized[0])][:, A.nearest_table_torch(W, q.resized[1])]
        for (y0, x0) in d.origins[:i + 1]:
            np.unique(full[y0:y0 + C, x0:x0 + C], return_counts=True)
        win = full[q.offset[0]:q.offset[0] + C, q.offset[1]:q.offset[1] + C]
        win = (win[:, ::-1] if q.flip else win).astype(np.int64)
        cls = np.unique(win)
        cls = cls[cls != 255]
        return torch.from_numpy(np.stack([win == k for k in cls])).to(dev)

    assert torch.equal(native_bits()[0], torch_bits()), "label_bits and the torch route differ"
    assert torch.equal(pack_masks(host_route()), native_bits()[0]), "label_bits and the host route differ"
    assert native_bits()[1].cpu().tolist() == counts[i][classes].tolist(), "areas and window counts differ"
    routes = [("window_counts (10 windows, with its host wait)", native_counts, clock), ("resample_labels (uint8, one image)", native_resample, events),
              (f"label_bits, {len(classes)} classes present", native_bits, events), ("torch: stack of == then pack_masks", torch_bits, events),
              ("host, one thread: nearest + np.unique per try + numpy masks + upload (CPU time)", host_route, clock)]
    res = measure(routes)
    kern = {0: "label_counts_kernel", 1: "label_resample_kernel", 2: "label_bits_kernel"}
    for n, ((name, fn, _), r) in enumerate(zip(routes, res)):
        print(f"| semantic {C} x {C}, K = {K}, window {i} of {len(d.origins)} taken | {name} | {r} | {alone(fn, kern[n]) if n in kern else '-'} |")


if __name__ == "__main__":
    main()
