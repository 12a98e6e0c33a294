#!/usr/bin/env python3
"""Forward + backward of one Swin block's attention core, native route (csrc/win_attn.hip) against the torch-op route
(swin.window_attention_torch under bf16 autocast, the reference's op sequence), at

    Swin-B, 1024^2   stage 1  (B, Hp, Wp, heads, ws) = (2, 264, 264, 4, 12)   and   stage 3  (2, 72, 72, 16, 12)
    Swin-T, window 7          (2, 259, 259, 3, 7)

with shift = ws // 2.  Device time: events around blocks of back-to-back forward + backward calls on warmed shapes, the two routes
alternated in one process, three repeats; the median and the torch route's spread over the repeats ((max - min) / median).  Then
the two kernels' own device time from the library's launch profiler (events around each kernel, a pass of its own) and their share
of the algorithmic-bytes roofline (qkv and out once in the forward; qkv, out, dout and dqkv once in the backward, over 8 TB/s; the
table-gradient fold, a launch of a few microseconds, is not in it).  Every shape runs in a fresh child process under its own time limit.

    python tools/bench_win_attn.py [--reps 20] [--rounds 3] [--timeout 240]

Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("Swin-B 1024^2 stage 1", 2, 264, 264, 4, 12), ("Swin-B 1024^2 stage 3", 2, 72, 72, 16, 12), ("Swin-T window 7", 2, 259, 259, 3, 7))
HBM_PEAK = 8.0e12       # bytes / s (MI355X spec)


def algorithmic_bytes(B, Hp, Wp, heads):
    """bf16 elements the algorithm must move: forward 4 C per token (qkv in, out out), backward 8 C (qkv, out, dout in, dqkv out)"""
    return B * Hp * Wp * heads * 32 * 12 * 2


def child(args):
    import torch
    from mp_former_amd import _lib, swin
    if not torch.cuda.is_available():
        sys.exit("bench_win_attn.py needs a GPU")
    dev = torch.device("cuda:0")
    _, B, Hp, Wp, heads, ws = SHAPES[args.child]
    shift, scale, C = ws // 2, 32 ** -0.5, heads * 32
    g = torch.Generator(device=dev).manual_seed(1)
    qkv = torch.randn(B, Hp, Wp, 3 * C, device=dev, generator=g).bfloat16().requires_grad_(True)
    table = (torch.randn((2 * ws - 1) ** 2, heads, device=dev, generator=g) * 0.5).requires_grad_(True)
    dout = torch.randn(B, Hp, Wp, C, device=dev, generator=g).bfloat16()

    def native():
        swin.window_attention(qkv, table, ws, shift, scale).backward(dout)

    def torch_():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = swin.window_attention_torch(qkv, table, ws, shift, scale)
        out.backward(dout)

    def block(fn):
        qkv.grad = table.grad = None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.reps

    # the two routes agree before anything is timed
    native()
    assert _lib.last_kernel() == "win_attn_bwd_kernel", _lib.last_kernel()
    gn = qkv.grad.float().clone()
    qkv.grad = None
    torch_()
    rel = float((qkv.grad.float() - gn).norm() / gn.norm())
    assert rel < 2e-2, f"routes disagree: relative difference of dqkv {rel}"
    for fn in (torch_, native):
        block(fn)
    tn, tt = [], []
    for _ in range(args.rounds):
        tt.append(block(torch_))
        tn.append(block(native))
    # the two kernels' own device time: the library's launch profiler (events around the kernel only), in a pass of its own
    _lib.profile_enable(True)
    for _ in range(args.reps):
        native()
    torch.cuda.synchronize()
    kern = {}
    for name in ("win_attn_fwd_kernel", "win_attn_bwd_kernel"):
        n, ms, _ = _lib.profile_get(name)
        kern[name] = ms * 1e3 / max(n, 1)
    _lib.profile_enable(False)
    print(json.dumps(dict(native_us=tn, torch_us=tt, dqkv_rel_diff=rel, kernel_us=kern)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="forward + backward calls per timed block")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per shape")
    ap.add_argument("--child", type=int)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    print("| shape | (B, Hp, Wp, heads, ws) | native fwd+bwd us | torch route fwd+bwd us | torch spread | native / torch | fwd kernel us | "
          "bwd kernel us | algorithmic MB | kernels' share of the bytes roofline |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for i, (name, B, Hp, Wp, heads, ws) in enumerate(SHAPES):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", str(i), "--reps", str(args.reps),
               "--rounds", str(args.rounds)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.exit(f"{name}: the child ended with status {r.returncode}; nothing further is started")
        z = json.loads(r.stdout.strip().splitlines()[-1])
        tn, tt = statistics.median(z["native_us"]), statistics.median(z["torch_us"])
        spread = (max(z["torch_us"]) - min(z["torch_us"])) / tt
        nbytes = algorithmic_bytes(B, Hp, Wp, heads)
        kf, kb = z["kernel_us"]["win_attn_fwd_kernel"], z["kernel_us"]["win_attn_bwd_kernel"]
        print(f"| {name} | ({B}, {Hp}, {Wp}, {heads}, {ws}) | {tn:.0f} | {tt:.0f} | {100 * spread:.1f} % | {tn / tt:.3f} | {kf:.0f} | {kb:.0f} | "
              f"{nbytes / 1e6:.0f} | {100 * nbytes / HBM_PEAK / ((kf + kb) * 1e-6):.1f} % |", flush=True)


if __name__ == "__main__":
    main()
