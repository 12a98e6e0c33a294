#!/usr/bin/env python3
"""Point noise of the mask-piloted rows: the torch route (the reference's ops, as transformer_decoder.noisy_rows runs them under
replay, with torch.rand as the source of the draws) against the native route (csrc/mp_noise.hip, one launch per mask), at config
B's three level grids, N = 2, 20 instances per image, scalar 1 and 5.

    python tools/bench_mp_noise.py               device time per mask: events around blocks of back-to-back calls, the two
                                                 routes alternated in one process, median over the rounds
    python tools/bench_mp_noise.py --launches    kernel launches per mask of each route, from `rocprofv3 --kernel-trace --stats`
                                                 runs of this file (fresh child processes; two mask counts, the difference
                                                 divided by the extra masks, so that the set-up launches cancel)

Needs a GPU: there is no fallback."""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = ((32, 32), (64, 64), (128, 128))
N, PER_IMAGE, NOISE = 2, 20, 0.2


def setup(hw, scalar, dev):
    """-> base [R, HW] bool (random rectangles, as the ground-truth rows of a level), and both routes' index tables"""
    import numpy as np
    import torch
    h, w = hw
    g = np.random.default_rng(h * 131 + scalar)
    rows = np.ones((N * PER_IMAGE, h, w), dtype=bool)
    for t in range(rows.shape[0]):
        hh, ww = int(g.integers(h // 8, h // 2)), int(g.integers(w // 8, w // 2))
        y0, x0 = int(g.integers(0, h - hh)), int(g.integers(0, w - ww))
        rows[t, y0:y0 + hh, x0:x0 + ww] = False
    base = torch.from_numpy(rows.reshape(rows.shape[0], h * w)).to(dev).repeat(scalar, 1)
    pad = scalar * PER_IMAGE
    bid = torch.arange(N).repeat_interleave(PER_IMAGE).repeat(scalar).to(dev)
    slot = torch.cat([torch.arange(PER_IMAGE).repeat(N) + PER_IMAGE * s for s in range(scalar)]).to(dev)
    src_of = torch.full((N, pad), -1, dtype=torch.int32)
    src_of[bid.cpu(), slot.cpu()] = torch.arange(base.shape[0], dtype=torch.int32)
    return base, bid, slot, src_of.reshape(-1).to(dev), pad


def torch_route(base, bid, slot, pad):
    """the ops of transformer_decoder.noisy_rows, the draws from torch.rand"""
    import torch
    ratio = (~base).sum(1) * (NOISE / base.shape[1])
    pm = torch.ones(N, pad, base.shape[1], dtype=torch.bool, device=base.device)
    pm[(bid, slot)] = torch.logical_xor(base, torch.rand(*base.shape, device=base.device) < ratio[:, None])
    return pm


def time_routes(args):
    import torch
    from mp_former_amd import _lib, transformer_decoder as TD
    dev = torch.device("cuda:0")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; N = {N}, {PER_IMAGE} instances per image, noise_scale {NOISE}; "
          f"{args.reps} back-to-back masks per block, {args.rounds} alternated rounds, median")
    print("| level | scalar | rows R | bytes out | torch route us / mask | native us / mask | native GB/s (read + write) | count launch us |")
    print("|---|---|---|---|---|---|---|---|")
    for hw in LEVELS:
        for scalar in (1, 5):
            base, bid, slot, src_of, pad = setup(hw, scalar, dev)
            counts = TD.mp_open_counts(base)
            state = {"draw": 0}

            def native():
                state["draw"] += 4
                return TD.mp_noise_rows(base, src_of, N, pad, NOISE, 1234, state["draw"], counts)

            def torch_():
                return torch_route(base, bid, slot, pad)

            def block(fn, reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(reps):
                    fn()
                b.record()
                b.synchronize()
                return a.elapsed_time(b) * 1e3 / reps

            for fn in (torch_, native):
                block(fn, 20)
            native()
            assert _lib.last_kernel() == "mp_noise_rows_kernel", _lib.last_kernel()
            t_torch, t_native, t_count = [], [], []
            for _ in range(args.rounds):
                t_torch.append(block(torch_, args.reps))
                t_native.append(block(native, args.reps))
                t_count.append(block(lambda: TD.mp_open_counts(base), args.reps))
            tt, tn, tc = (statistics.median(x) for x in (t_torch, t_native, t_count))
            nbytes = N * pad * base.shape[1]
            moved = nbytes + base.numel()
            print(f"| {hw[0]} x {hw[1]} | {scalar} | {base.shape[0]} | {nbytes} | {tt:.1f} | {tn:.1f} | {moved / tn / 1e3:.0f} | {tc:.1f} |")


def child(args):
    """`masks` masks of one route at the finest level, scalar 5 (run under rocprofv3 by --launches)"""
    import torch
    from mp_former_amd import transformer_decoder as TD
    dev = torch.device("cuda:0")
    base, bid, slot, src_of, pad = setup(LEVELS[2], 5, dev)
    counts = TD.mp_open_counts(base) if args.child == "native" else None
    for i in range(args.masks):
        if args.child == "native":
            TD.mp_noise_rows(base, src_of, N, pad, NOISE, 1234, 4 * i, counts)
        else:
            torch_route(base, bid, slot, pad)
    torch.cuda.synchronize()


def launches(args):
    def calls(route, masks):
        with tempfile.TemporaryDirectory() as d:
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "p", "--",
                   sys.executable, os.path.abspath(__file__), "--child", route, "--masks", str(masks)]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                raise RuntimeError("rocprofv3 wrote no kernel statistics")
            out = {}
            for row in csv.DictReader(open(files[0])):
                out[row["Name"]] = out.get(row["Name"], 0) + int(row["Calls"])
            return out

    lo, hi = 10, 30
    print(f"# kernel launches per mask at 128 x 128, scalar 5: (calls with {hi} masks - calls with {lo} masks) / {hi - lo}")
    print("| route | launches / mask | kernels |")
    print("|---|---|---|")
    for route in ("torch", "native"):
        a, b = calls(route, lo), calls(route, hi)
        per = {k: (b.get(k, 0) - a.get(k, 0)) / (hi - lo) for k in b}
        per = {k: v for k, v in per.items() if v}
        short = lambda k: k.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0][:48]  # noqa: E731
        names = ", ".join(f"{v:g} x {short(k)}" for k, v in sorted(per.items(), key=lambda kv: -kv[1]))
        print(f"| {route} | {sum(per.values()):g} | {names} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="back-to-back masks per timed block (>= 100)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--child", choices=("torch", "native"))
    ap.add_argument("--masks", type=int, default=10)
    args = ap.parse_args()
    if args.launches:
        return launches(args)             # (the children open the GPU, this process does not)
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_mp_noise.py needs a GPU")
    if args.reps < 100 and not args.child:
        sys.exit("--reps must be at least 100")
    return child(args) if args.child else time_routes(args)


if __name__ == "__main__":
    main()
