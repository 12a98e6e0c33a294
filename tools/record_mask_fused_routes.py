"""Route table of the fused mask product host layer (the entry points of csrc/mask_fused.hip on the record of
csrc/mask_fused_host.h): which kernel every entry point names on the smallest problems that reach each host decision, what the
profiler logs and what the kernels write.

    python tools/record_mask_fused_routes.py [--out tests/golden/mask_fused_routes.json]

runs CASES on cuda:0 and writes the fixture that tests/test_mask_fused_routes_recorded_gpu.py compares the library against.  Record
it from the library BEFORE a change of the host layer; the test then pins the change.  The problems are those of
tests/_mask_fused_cases.py and tests/_mask_fused_clip_cases.py (NaN poison around everything addressed), at these shapes:

  cost      all seven chunk widths TCH at Tmax = 2 TCH and 2 TCH + 1 (the next width; 129 targets are rejected); Q = 127 | 128 | 129
            with a group without targets; P = 1 (one tile), 33 (two tiles, one per workgroup), 330 (two tiles per workgroup) and
            4128 (three)
  clip      all seven TCH at F = 2; F = 1 and F = 3; F = 3 at 129 tiles per frame in runs of 7: workgroups whose run crosses a frame
            boundary
  forward   2 x 2 and 8 x 16 planes with the slot counts (1) and (48, 49, 0)
  backward  P1 and the cases at KS = 1 (P9) and 64 (P7), mgroups = 1 and 3 (P5): both gradients with d_embed bf16, with d_embed fp32,
            then d_embed NULL, then d_features NULL

A case is one or more calls run back to back in one process.  Every cost and clip case makes its call twice, so each of the 14
instantiations of the cost kernel is launched a first and a later time (its dynamic-LDS limit is raised once per process).  Output
buffers start as a sentinel, workspaces as 0xFF bytes and have exactly the queried size.

Per case the fixture holds
    kernels   mpf_last_kernel after each call
    prof      the launch profiler's records of the family: name -> [launches, logged algorithmic bytes, logged flops]
    hashes    SHA-256 of every output buffer and of the whole workspace ("<call>.<buffer>").  All kernels of the family are
              fixed-order without atomics: the recorder runs every case twice and refuses to write a fixture if two runs differ.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _mask_fused_cases as MC  # noqa: E402
import _mask_fused_clip_cases as KC  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "mask_fused_routes.json")
BF16, F32 = torch.bfloat16, torch.float32
PROF_NAMES = ("match_cost_fused_kernel", "pair_planes_fwd_kernel", "pair_planes_dfeat_kernel", "pair_planes_dembed_kernel")
# (d_embed dtype, d_features wanted, d_embed wanted) of the four backward calls of a case
BWD_CALLS = ((BF16, True, True), (F32, True, True), (BF16, True, False), (BF16, False, True))


def _cases():
    c = {}
    small = dict(L=1, N=2, Q=10, P=33, hw=(8, 12))
    for tch in (4, 8, 12, 16, 24, 32, 64):
        for Tmax in (2 * tch, 2 * tch + 1):
            if Tmax <= 128:
                c[f"cost Tmax={Tmax}"] = dict(kind="cost", seed=5000 + Tmax, counts=(Tmax, 3), **small)
        c[f"clip Tmax={2 * tch}"] = dict(kind="clip", seed=5400 + tch, F=2, counts=(2 * tch, 3), **small)
    for Q in (127, 128, 129):
        c[f"cost Q={Q}"] = dict(kind="cost", seed=5200 + Q, **dict(MC.COST_CASES["C2"], Q=Q))
    for name in ("C1", "C4", "C9", "C10"):
        c[f"cost P={MC.COST_CASES[name]['P']}"] = dict(kind="cost", seed=3000 + int(name[1:]), **MC.COST_CASES[name])
    for name in ("K1", "K2", "K4"):
        c[f"clip {name} F={KC.CLIP_CASES[name]['F']}"] = dict(kind="clip", seed=4000 + int(name[1:]), **KC.CLIP_CASES[name])
    c["clip F=3 crossing"] = dict(kind="clip", seed=4100, **dict(KC.CLIP_CASES["K6"], F=3))
    for hw in ((2, 2), (8, 16)):
        for counts in ((1,), (48, 49, 0)):
            c[f"forward {hw[0]}x{hw[1]} counts {counts}"] = dict(kind="forward", hw=hw, counts=counts)
    for name in ("P1", "P5", "P7", "P9"):
        c[f"backward {name}"] = dict(kind="backward", name=name)
    return c


CASES = _cases()


def geometry(case):
    """what the case is there for, from the mirrors of tests/_mask_fused_cases.py (checked by the recorded test)"""
    k = case["kind"]
    if k == "cost":
        G, Tmax = case["L"] * case["N"], max(case["counts"])
        m = MC.mc_geom(G, case["Q"], case["P"])
        return dict(TCH=MC.tch_of(Tmax), tiles_per_wg=m.tiles_per_wg, nwg=m.nwg)
    if k == "clip":
        m = KC.mc_geom_clip(case["L"] * case["N"], case["Q"], case["P"], case["F"])
        return dict(TCH=MC.tch_of(max(case["counts"])), tiles_per_wg=m.tiles_per_wg, nwg=m.nwg, crossing=m.crossing)
    if k == "backward":
        KP, mgroups, KS, steps = MC.PAIR_CASES[case["name"]]["geom"]
        return dict(KS=KS, mgroups=mgroups)
    return {}


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _i32(a, dev):
    return torch.from_numpy(np.asarray(a).astype(np.int32)).to(dev)


def _poison(n, dev):
    return torch.full((int(n),), 0xFF, dtype=torch.uint8, device=dev)


def _run_cost(case, dev, lib, call, st):
    clip = case["kind"] == "clip"
    kw = {k: v for k, v in case.items() if k not in ("kind", "geom")}
    cp = KC.clip_problem(**kw) if clip else MC.cost_problem(**kw)
    rows = cp.tsamp.shape[0]
    embed, ef, feat, coords, tsamp = cp.embed.to(dev), torch.from_numpy(cp.embed_first).to(dev), cp.feat.to(dev), cp.coords.to(dev), cp.tsamp.to(dev)
    gi, tf, tc = _i32(cp.group_clip if clip else cp.group_image, dev), _i32(cp.t_first, dev), _i32(cp.t_count, dev)
    out = {}
    for i in range(2):
        cost = torch.full((cp.G, cp.Q, cp.Tmax), MC.SENT_GRAD, dtype=F32, device=dev)
        tail = (coords.data_ptr(), tsamp.data_ptr(), rows, tf.data_ptr(), tc.data_ptr(), cost.data_ptr(), cp.G, cp.Q, cp.Tmax, cp.P)
        if clip:
            ws = _poison(lib.mpf_match_cost_fused_clip_workspace_bytes(cp.G, cp.Q, cp.Tmax, cp.P, cp.F, rows), dev)
            call("mpf_match_cost_fused_clip", embed.data_ptr(), ef.data_ptr(), cp.row_stride, feat.data_ptr(), cp.clip_stride, cp.frame_stride,
                 gi.data_ptr(), cp.h, cp.w, MC.C, *tail, cp.F, MC.W_MASK, MC.W_DICE, ws.data_ptr(), ws.numel(), st)
        else:
            ws = _poison(lib.mpf_match_cost_fused_workspace_bytes(cp.G, cp.Q, cp.Tmax, cp.P, rows), dev)
            call("mpf_match_cost_fused", embed.data_ptr(), ef.data_ptr(), cp.row_stride, feat.data_ptr(), cp.feat_stride, gi.data_ptr(), cp.h, cp.w,
                 MC.C, *tail, MC.W_MASK, MC.W_DICE, ws.data_ptr(), ws.numel(), st)
        out[f"{i}.cost"], out[f"{i}.workspace"] = cost, ws
    return out


def _run_pairs(case, dev, lib, call, st):
    from mp_former_amd import _lib
    fwd = case["kind"] == "forward"
    pb = MC.fwd_problem(case["hw"], case["counts"]) if fwd else MC.pair_case(case["name"])
    embed, feat, row_off, pos = pb.embed.to(dev), pb.feat.to(dev), pb.row_off.to(dev), pb.pair_of_slot.to(dev)
    first, count = _i32(pb.first, dev), _i32(pb.counts, dev)
    head = (embed.data_ptr(), row_off.data_ptr(), pos.data_ptr(), first.data_ptr(), count.data_ptr(), feat.data_ptr(), pb.feat_stride)
    if fwd:
        out = torch.full((pb.total, pb.HW), MC.SENT_OUT, dtype=BF16, device=dev)
        call("mpf_pair_planes_forward", *head, out.data_ptr(), pb.N, pb.HW, MC.C, st)
        return {"0.planes": out}
    G, out = pb.G.to(dev), {}
    for i, (dtype, want_dF, want_dE) in enumerate(BWD_CALLS):
        dF = torch.full((pb.N, pb.HW, MC.C), MC.SENT_GRAD, dtype=BF16, device=dev) if want_dF else None
        dE = torch.full((pb.R, pb.N, MC.C), MC.SENT_GRAD, dtype=dtype, device=dev) if want_dE else None
        ws = _poison(lib.mpf_pair_planes_backward_workspace_bytes(pb.N, pb.HW, pb.total, pb.max_count), dev)
        call("mpf_pair_planes_backward", G.data_ptr(), *head, _lib.ptr(dF), pb.HW * MC.C, _lib.ptr(dE), _lib.DTYPE[dtype], pb.N, pb.HW, MC.C,
             pb.total, pb.max_count, ws.data_ptr(), ws.numel(), st)
        out[f"{i}.workspace"] = ws
        if want_dF:
            out[f"{i}.d_features"] = dF
        if want_dE:
            out[f"{i}.d_embed"] = dE
    return out


def _run_once(case, dev):
    """-> kernels, prof, {"<call>.<buffer>": device tensor}"""
    from mp_former_amd import _lib
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    kernels = []

    def call(name, *args):
        _lib.call(name, dev, *args)
        kernels.append(_lib.last_kernel())

    try:
        _lib.profile_enable(True)
        bufs = (_run_cost if case["kind"] in ("cost", "clip") else _run_pairs)(case, dev, lib, call, st)
        torch.cuda.synchronize(dev)
        prof = {}
        for name in PROF_NAMES:
            n, _, by = _lib.profile_get(name)
            if n:
                prof[name] = [n, by, _lib.profile_get_flops(name)]
    finally:
        _lib.profile_enable(False)
    return kernels, prof, bufs


def run_case(case, dev):
    kernels, prof, bufs = _run_once(case, dev)
    return dict(kernels=kernels, prof=prof, hashes={k: _sha(t) for k, t in bufs.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from mp_former_amd import _lib
    out = {"device": torch.cuda.get_device_name(dev), "cases": {}}
    wrong = []
    for cid, case in CASES.items():
        r, again = run_case(case, dev), run_case(case, dev)
        print(f"{cid:<36} {geometry(case)} {' | '.join(r['kernels'])}\n    prof {r['prof']}", flush=True)
        if again != r:
            wrong.append(f"{cid}: two runs differ in {sorted(k for k in r['hashes'] if again['hashes'][k] != r['hashes'][k]) or 'kernels / prof'}")
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
