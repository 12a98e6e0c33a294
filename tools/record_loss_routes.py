"""Route table of the loss host layer (the entry points of csrc/loss.hip on the record of csrc/loss_host.h): which kernel every
entry point runs on the smallest problems that reach each host decision, what the profiler logs and what the kernels write.

    python tools/record_loss_routes.py [--out tests/golden/loss_routes.json]

runs CASES on cuda:0 and writes the fixture that tests/test_loss_routes_recorded_gpu.py compares the library against.  Record it
from the library BEFORE a change of the host layer; the test then pins the change.  A case is one or more steps (a call each) run
back to back in one process: the two-step cases call one kernel with a larger and then a smaller dynamic-LDS size, the path on
which a launcher that raises the LDS limit once per high-water mark must not lower it again.  Inputs are host draws of a generator
seeded by the step's parameters; every output buffer starts as the sentinel -7 (the clip workspace as 0xFF bytes).

Per case the fixture holds
    kernels   mpf_last_kernel after each step
    prof      the launch profiler's records of those names: name -> [launches, logged algorithmic bytes]
    hashes    SHA-256 of every output buffer ("<step>.<buffer>") on which two runs of the case agree: all of them but the fp32
              gradient of mpf_mask_loss_backward (global atomics), which the test holds to the fp64 restatement instead
"""
import argparse
import hashlib
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "loss_routes.json")

SENT = -7.0                        # exact in bf16
GT_HW = (40, 56)                   # 2240 pixels = 70 words: rows of 56 straddle the words of the bit-packed form
SLOTS, PAIR_SLOTS, PAIR_GT = 8, [5, 0, 3, 6, 2], [4, 0, 5, 2, 1]
BF16, F32 = "bf16", "f32"
TORCH = {BF16: torch.bfloat16, F32: torch.float32, "u8": torch.uint8}
COUNTS = (5, 0, 9)                 # targets per image: one image without any; 9 = two passes of 4 and a tail (LDS), 8 + 1 (generic)
ATOMIC = "grad_atomic"             # the one buffer that two runs need not reproduce


def _cost(hw, Q, P, G, dtype=BF16, counts=COUNTS, F=0):
    return dict(kind="cost", hw=hw, Q=Q, P=P, G=G, dtype=dtype, counts=counts, F=F)


def _pairs(kind, hw, P, dtype, packed=False, n=5, chunks=8):
    return dict(kind=kind, hw=hw, P=P, dtype=dtype, packed=packed, n=n, chunks=chunks)


def _cases():
    c = {}
    small, k132, k140 = (16, 24), (264, 256), (280, 256)
    # image cost
    c["cost bf16 grouped P=12800"] = [_cost(small, 6, 12800, 6)]
    c["cost bf16 grouped P=12801"] = [_cost(small, 6, 12801, 6)]
    c["cost bf16 132 KiB plane"] = [_cost(k132, 2, 1031, 2, counts=(5,))]
    c["cost bf16 140 KiB plane"] = [_cost(k140, 2, 1031, 2, counts=(5,))]
    c["cost bf16 odd group"] = [_cost(small, 7, 500, 7)]
    c["cost bf16 odd row count"] = [_cost(small, 3, 500, 2, counts=(5,))]
    c["cost f32 grouped"] = [_cost(small, 6, 500, 6, dtype=F32)]
    c["cost bf16 ungrouped P=20000 then P=9000"] = [_cost(small, 6, 20000, 1), _cost(small, 6, 9000, 1)]
    c["cost f32 ungrouped P=20000 then P=9000"] = [_cost(small, 6, 20000, 1, dtype=F32), _cost(small, 6, 9000, 1, dtype=F32)]
    c["cost bf16 132 KiB plane then 768-byte plane"] = [_cost(k132, 2, 1031, 2, counts=(5,)), _cost(small, 6, 500, 6)]
    # clip cost
    c["clip bf16 132 KiB plane"] = [_cost(k132, 2, 1031, 2, counts=(5,), F=2)]
    c["clip bf16 F=1"] = [_cost(small, 6, 500, 6, F=1)]
    c["clip bf16 F=3"] = [_cost(small, 6, 500, 6, F=3)]
    c["clip bf16 G=3"] = [_cost(small, 3, 500, 3, F=2)]
    c["clip bf16 G=5"] = [_cost(small, 5, 500, 5, F=2)]
    c["clip bf16 rows not a multiple of G"] = [_cost(small, 6, 500, 4, counts=(5,), F=2)]
    c["clip bf16 G=1"] = [_cost(small, 6, 500, 1, F=2)]
    c["clip bf16 P=12801"] = [_cost(small, 6, 12801, 6, F=2)]
    c["clip f32 P=9000"] = [_cost(small, 6, 9000, 6, dtype=F32, F=2)]
    c["clip f32"] = [_cost(small, 6, 500, 6, dtype=F32, F=3)]
    c["clip bf16 G=1 P=20000 then P=9000"] = [_cost(small, 2, 20000, 1, counts=(5,), F=2), _cost(small, 2, 9000, 1, counts=(5,), F=2)]
    c["clip bf16 128 KiB plane then 768-byte plane"] = [_cost((256, 256), 2, 1031, 2, counts=(5,), F=2), _cost(small, 6, 500, 6, F=2)]
    # mask-loss forward
    for packed in (False, True):
        gt = "bits" if packed else "bytes"
        c[f"forward bf16 {gt} chunks=256"] = [_pairs("forward", (32, 32), 1031, BF16, packed, chunks=256)]
        c[f"forward bf16 {gt} chunks=257"] = [_pairs("forward", (32, 32), 1031, BF16, packed, chunks=257)]
        c[f"forward bf16 {gt} 70-byte plane"] = [_pairs("forward", (5, 7), 300, BF16, packed)]
        c[f"forward bf16 {gt} 137.5 KiB plane"] = [_pairs("forward", (400, 176), 300, BF16, packed)]
        c[f"forward f32 {gt}"] = [_pairs("forward", (32, 32), 1031, F32, packed)]
        c[f"forward bf16 {gt} 128 KiB plane then 2 KiB plane"] = [_pairs("forward", (256, 256), 1031, BF16, packed, n=1),
                                                                _pairs("forward", (32, 32), 300, BF16, packed)]
        # dense backward: one band; three bands (134 / 134 / 132 rows), then one band again
        for dtype in (BF16, F32):
            c[f"dense {dtype} {gt} one band"] = [_pairs("dense", (32, 32), 1031, dtype, packed)]
            c[f"dense {dtype} {gt} three bands then one"] = [_pairs("dense", (400, 176), 300, dtype, packed), _pairs("dense", (32, 32), 300, dtype, packed)]
    for dtype in (BF16, F32):
        c[f"backward {dtype}"] = [_pairs("backward", (32, 32), 1031, dtype)]
    # importance selection: the steps of 16 / 37 / 40 keys per thread
    for M in (16384, 16385, 37888, 37889, 40960):
        c[f"sample_select M={M}"] = [dict(kind="sample_select", hw=small, M=M, k=M // 3)]
    c["sample_select 128 KiB plane then 768-byte plane"] = [dict(kind="sample_select", hw=(256, 256), M=700, k=100),
                                                            dict(kind="sample_select", hw=small, M=700, k=100)]
    c["select_uncertain"] = [dict(kind="select", M=5000, k=1250)]
    for dtype in (F32, BF16, "u8", "bits"):
        c[f"point_sample {dtype}"] = [dict(kind="point_sample", hw=(8, 20), P=1031, dtype=dtype)]
    c["pack_mask_bits"] = [dict(kind="pack", hw=(12, 40))]
    return c


CASES = _cases()


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _gen(step):
    return torch.Generator().manual_seed(zlib.crc32(repr(sorted(step.items())).encode()))


def _i32(a, dev):
    return torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev)


def _step_cost(s, dev, lib, call, st):
    from mp_former_amd import _lib
    g = _gen(s)
    (h, w), Q, P, G, counts, F = s["hw"], s["Q"], s["P"], s["G"], s["counts"], s["F"]
    N, Tmax, Fn, dt = len(counts), max(counts), max(F, 1), TORCH[s["dtype"]]
    maps = (torch.randn(N * Q, Fn, h, w, generator=g) * 3).to(dt).to(dev)
    coords = (torch.rand(N, P, 2, generator=g) * 1.1 - 0.05).to(dev)
    tsamp = torch.rand(sum(counts), Fn * P, generator=g).to(dev)
    offs = (torch.arange(N * Q, dtype=torch.int64) * Fn * h * w).to(dev)
    b = np.repeat(np.arange(N), Q)
    firsts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    crow, first, cnt = _i32(b, dev), _i32(firsts[b], dev), _i32(np.array(counts)[b], dev)
    cost = torch.full((N * Q, Tmax), SENT, dtype=torch.float32, device=dev)
    head = (maps.data_ptr(), _lib.DTYPE[dt], h, w, offs.data_ptr())
    tail = (coords.data_ptr(), crow.data_ptr(), tsamp.data_ptr(), first.data_ptr(), cnt.data_ptr(), cost.data_ptr(), N * Q, Tmax, P, 5.0, 2.0, G)
    if not F:
        call("mpf_match_cost", *head, *tail, st)
        return dict(cost=cost)
    ws = torch.full((lib.mpf_match_cost_clip_workspace_bytes(N * Q, F, Tmax),), 0xFF, dtype=torch.uint8, device=dev)
    call("mpf_match_cost_clip", *head, F, h * w, *tail, ws.data_ptr(), ws.numel(), st)
    return dict(cost=cost, workspace=ws)


def pairs_problem(s):
    """host tensors of a forward / dense / backward step: n pairs on n of SLOTS planes; with n = 5, pair 3 has an all-zero grad_sums
    row and every point of pair 4 lies outside the plane"""
    g = _gen(dict(s, kind="pairs", chunks=0))
    (h, w), (H, W), P, n = s["hw"], GT_HW, s["P"], s["n"]
    maps = (torch.randn(SLOTS, h, w, generator=g) * 2).to(TORCH[s["dtype"]])
    gt = torch.rand(6, H, W, generator=g) < 0.4
    coords = torch.rand(n, P, 2, generator=g) * 1.2 - 0.1
    gs = torch.tensor([[1.0, -2.0, 0.5, 0.0]]) * torch.arange(1, n + 1)[:, None]
    if n == 5:
        gs[3] = 0.0
        coords[4, :, 0] = 1.3 + 0.3 * torch.rand(P, generator=g)
    base = torch.randn(SLOTS, h, w, generator=g)
    return dict(maps=maps, gt=gt, coords=coords, gs=gs, base=base, slots=PAIR_SLOTS[:n], gt_rows=PAIR_GT[:n])


def _step_pairs(s, dev, lib, call, st):
    from mp_former_amd import _lib
    p = pairs_problem(s)
    (h, w), (H, W), P, n, dt = s["hw"], GT_HW, s["P"], s["n"], TORCH[s["dtype"]]
    maps, coords, gs = p["maps"].to(dev), p["coords"].to(dev), p["gs"].to(dev)
    gt = p["gt"].to(dev).view(torch.uint8)
    gdt = _lib.MPF_U8
    if s["packed"]:
        bits = torch.full((gt.numel() // 32,), -1, dtype=torch.int32, device=dev)
        _lib.call("mpf_pack_mask_bits", dev, gt.data_ptr(), bits.data_ptr(), gt.numel(), st)
        gt, gdt = bits, _lib.MPF_BITS
    po = (torch.tensor(p["slots"], dtype=torch.int64) * h * w).to(dev)
    rows = _i32(p["gt_rows"], dev)
    head = (maps.data_ptr(), _lib.DTYPE[dt], h, w, po.data_ptr(), gt.data_ptr())
    if s["kind"] == "forward":
        partial = torch.full((n, s["chunks"], 4), SENT, dtype=torch.float32, device=dev)
        call("mpf_mask_loss_forward", *head, gdt, H, W, rows.data_ptr(), coords.data_ptr(), partial.data_ptr(), n, P, s["chunks"], st)
        return dict(partial=partial)
    if s["kind"] == "dense":
        grad = torch.full((SLOTS, h, w), SENT, dtype=dt, device=dev)
        call("mpf_mask_loss_backward_dense", *head, gdt, H, W, rows.data_ptr(), coords.data_ptr(), gs.data_ptr(), grad.data_ptr(), _lib.DTYPE[dt],
             po.data_ptr(), n, P, st)
        return dict(grad=grad)
    grad = p["base"].to(dev)
    call("mpf_mask_loss_backward", *head, H, W, rows.data_ptr(), coords.data_ptr(), gs.data_ptr(), grad.data_ptr(), po.data_ptr(), n, P, st)
    return {ATOMIC: grad}


def _step_sample_select(s, dev, lib, call, st):
    from mp_former_amd import _lib
    g = _gen(s)
    (h, w), M, k, R = s["hw"], s["M"], s["k"], 2
    planes = (torch.randn(R, h, w, generator=g) * 3).bfloat16().to(dev)
    coords = torch.rand(R, M, 2, generator=g).to(dev)
    offs = (torch.arange(R, dtype=torch.int64) * h * w).to(dev)
    out = torch.full((R, k + 3, 2), SENT, dtype=torch.float32, device=dev)
    call("mpf_sample_select_uncertain", planes.data_ptr(), _lib.MPF_BF16, h, w, offs.data_ptr(), coords.data_ptr(), out.data_ptr(), R, M, k, k + 3, st)
    return dict(coords_out=out)


def _step_select(s, dev, lib, call, st):
    g = _gen(s)
    M, k, R = s["M"], s["k"], 3
    vals = (torch.round(torch.randn(R, M, generator=g) * 8) / 8).to(dev)           # ties at every threshold
    coords = torch.rand(R, M, 2, generator=g).to(dev)
    out = torch.full((R, k + 2, 2), SENT, dtype=torch.float32, device=dev)
    call("mpf_select_uncertain", vals.data_ptr(), coords.data_ptr(), out.data_ptr(), R, M, k, k + 2, st)
    return dict(coords_out=out)


def _step_point_sample(s, dev, lib, call, st):
    from mp_former_amd import _lib
    g = _gen(s)
    (h, w), P, R = s["hw"], s["P"], 5
    if s["dtype"] in (F32, BF16):
        src = (torch.randn(R, h, w, generator=g) * 3).to(TORCH[s["dtype"]]).to(dev)
        code = _lib.DTYPE[TORCH[s["dtype"]]]
    else:
        src, code = (torch.rand(R, h, w, generator=g) < 0.35).to(dev).view(torch.uint8), _lib.MPF_U8
        if s["dtype"] == "bits":
            bits = torch.full((src.numel() // 32,), -1, dtype=torch.int32, device=dev)
            _lib.call("mpf_pack_mask_bits", dev, src.data_ptr(), bits.data_ptr(), src.numel(), st)
            src, code = bits, _lib.MPF_BITS
    coords = (torch.rand(2, P, 2, generator=g) * 1.2 - 0.1).to(dev)
    offs = (torch.arange(R, dtype=torch.int64) * h * w).to(dev)
    out = torch.full((R, P), SENT, dtype=torch.float32, device=dev)
    call("mpf_point_sample", src.data_ptr(), code, h, w, offs.data_ptr(), coords.data_ptr(), _i32([0, 1, 0, 1, 1], dev).data_ptr(), out.data_ptr(), R, P, st)
    return dict(out=out)


def _step_pack(s, dev, lib, call, st):
    (h, w), R = s["hw"], 5
    masks = (torch.rand(R, h, w, generator=_gen(s)) < 0.35).to(dev).view(torch.uint8)
    bits = torch.full((masks.numel() // 32,), -1, dtype=torch.int32, device=dev)
    call("mpf_pack_mask_bits", masks.data_ptr(), bits.data_ptr(), masks.numel(), st)
    return dict(bits=bits)


_STEP = {"cost": _step_cost, "forward": _step_pairs, "dense": _step_pairs, "backward": _step_pairs, "sample_select": _step_sample_select,
         "select": _step_select, "point_sample": _step_point_sample, "pack": _step_pack}


def _run_once(steps, dev):
    """-> kernels, prof, {"<step>.<buffer>": device tensor}"""
    from mp_former_amd import _lib
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    kernels, bufs = [], {}

    def call(name, *args):
        _lib.call(name, dev, *args)
        kernels.append(_lib.last_kernel())

    try:
        _lib.profile_enable(True)
        for i, s in enumerate(steps):
            for name, t in _STEP[s["kind"]](s, dev, lib, call, st).items():
                bufs[f"{i}.{name}"] = t
        torch.cuda.synchronize(dev)
        prof = {}
        for name in sorted(set(kernels)):
            n, _, by = _lib.profile_get(name)
            if n:
                prof[name] = [n, by]
    finally:
        _lib.profile_enable(False)
    return kernels, prof, bufs


def run_case(steps, dev, hashed=None):
    """One case -> {"kernels", "prof", "hashes"} and the device buffers of the run.  ``hashed`` (the fixture's list): the buffers to
    hash; None = decide by running the case twice (the recorder)."""
    kernels, prof, bufs = _run_once(steps, dev)
    hashes = {k: _sha(t) for k, t in bufs.items() if hashed is None or k in hashed}
    if hashed is None:
        _, _, again = _run_once(steps, dev)
        hashes = {k: h for k, h in hashes.items() if _sha(again[k]) == h}
    return dict(kernels=kernels, prof=prof, hashes=hashes), bufs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from mp_former_amd import _lib
    out = {"device": torch.cuda.get_device_name(dev), "cases": {}}
    wrong = []
    for cid, steps in CASES.items():
        r, bufs = run_case(steps, dev)
        print(f"{cid:<52} {' | '.join(r['kernels'])}\n    prof {r['prof']} hashed {sorted(r['hashes'])}", flush=True)
        loose = sorted(k for k in bufs if k not in r["hashes"] and not k.endswith(ATOMIC))
        if loose:
            wrong.append(f"{cid}: two runs differ in {loose}")
        out["cases"][cid] = r
    print(f"library {_lib.LIB_PATH}; {len(CASES)} cases")
    if wrong:
        raise SystemExit("cases that do not reproduce:\n  " + "\n  ".join(wrong))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
