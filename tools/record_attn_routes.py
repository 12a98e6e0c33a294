"""Route table of the attention host layer (the entry points of csrc/attn.hip on the records of csrc/attn_host.h): which kernels
every entry point runs on the smallest problems that reach each host decision, what the profiler logs and what they write.

    python tools/record_attn_routes.py [--out tests/golden/attn_routes.json]

runs CASES on cuda:0 and writes the fixture that tests/test_attn_routes_gpu.py compares the library against.  Record it from the
library BEFORE a change of the host layer; the test then pins the change.  All cases use H = 2 heads (E = 64) and N = 2 images;
the inputs are host draws of a generator seeded by the case's shape and mask kind (so that the dense, strided and aux routes see
the same values), rounded to bf16.  Every output starts as NaN bytes, the workspace and aux as 0xFF bytes.

Per case the fixture holds
    kernels   mpf_last_kernel after each call of the case (one label for all AL / MK / OCC forms of a kernel: the label does not
              tell which form ran, and the forms write equal bits wherever more than one is valid)
    prof      the launch profiler's records of the three attention labels: name -> [launches, logged algorithmic bytes]
    hashes    SHA-256 of every buffer the calls write (the workspace after the forward and after the backward, the aux buffer
              whole, padding included) on which two runs of the case agree: no atomics, fixed merge order, so all of them
    and the case's own flags: gap_keeps_prefill (strided dK / dV), delta_same_bits (mpf_attn_delta against mpf_attn_bwd_prep).
EQUAL lists the cross-case equalities: the strided and aux routes against the dense route on the same values.
"""
import argparse
import hashlib
import json
import os
import sys
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "attn_routes.json")

N, H, HD, E = 2, 2, 32, 64
SCALE = HD ** -0.5
LQ = 33                          # two query tiles, LqP = 64
DEFAULTS = {"attn_occ": 4, "attn_nw": 8, "attn_kpw": 0}
PROF_NAMES = ("attn_fwd_kernel<2>", "attn_bwd_kv_kernel", "attn_bwd_q_kernel<2>")
FLAGS = ("gap_keeps_prefill", "delta_same_bits")


def _cases():
    c = []
    split1 = {"attn_kpw": 64, "attn_nw": 1}
    for mask in ("image", None):
        for occ in (4, 2):
            c.append(dict(id=f"dense Lk=72 mask {mask} occ {occ}", kind="attn", route="dense", Lk=72, mask=mask, opts={"attn_occ": occ}))
    c.append(dict(id="dense Lk=67 mask shared", kind="attn", route="dense", Lk=67, mask="shared"))
    c.append(dict(id="dense Lk=67 mask None", kind="attn", route="dense", Lk=67, mask=None))
    c.append(dict(id="dense Lk=72 mask at an odd address", kind="attn", route="dense", Lk=72, mask="image", odd=True))
    c.append(dict(id="dense Lk=72 kT vT off by 4 elements", kind="attn", route="dense", Lk=72, mask="image", offset_t=True))
    c.append(dict(id="dense Lk=136 3 splits", kind="attn", route="dense", Lk=136, mask="image", opts=split1, wg=3))
    c.append(dict(id="dense Lk=600 10 splits", kind="attn", route="dense", Lk=600, mask="image", opts=split1, wg=10))
    c.append(dict(id="strided Lk=72 mask image", kind="attn", route="strided", Lk=72, mask="image"))
    c.append(dict(id="aux Lk=72 mask image", kind="attn", route="aux", Lk=72, mask="image"))
    c.append(dict(id="aux Lk=67 mask shared", kind="attn", route="aux", Lk=67, mask="shared"))
    c.append(dict(id="aux Lk=72 mask None", kind="attn", route="aux", Lk=72, mask=None))
    for L, LP in ((72, 72), (67, 67), (33, 64)):
        for strided in (False, True):
            c.append(dict(id=f"transpose L={L} LP={LP}" + (" strided" if strided else ""), kind="transpose", L=L, LP=LP, strided=strided))
    c.append(dict(id="delta", kind="delta"))
    ids = [x["id"] for x in c]
    assert len(set(ids)) == len(ids)
    return c


CASES = _cases()
_DENSE = ("kT", "vT", "out", "lse", "qT", "doT", "delta", "dq", "dk", "dv")
# (case, case, the buffers that must hold equal bits)
EQUAL = [
    ("strided Lk=72 mask image", "dense Lk=72 mask image occ 4", _DENSE + ("ws_fwd", "ws_bwd")),
    ("aux Lk=72 mask image", "dense Lk=72 mask image occ 4", _DENSE),
    ("aux Lk=67 mask shared", "dense Lk=67 mask shared", _DENSE),
    ("aux Lk=72 mask None", "dense Lk=72 mask None occ 4", _DENSE),
] + [(f"transpose L={L} LP={LP} strided", f"transpose L={L} LP={LP}", ("aT", "bT")) for L, LP in ((72, 72), (67, 67), (33, 64))]


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _draw(seed, *shapes):
    g = torch.Generator().manual_seed(zlib.crc32(seed.encode()))
    return [torch.randn(s, generator=g).bfloat16() for s in shapes], g


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _packed(parts, width, dev):
    """[L, N, width] bf16 on the device, NaN except for the [L, N, E] tensors `parts` = {first column: tensor}"""
    buf = _nan(tuple(next(iter(parts.values())).shape[:2]) + (width,), torch.bfloat16, dev)
    for c0, t in parts.items():
        buf[..., c0:c0 + E] = t.to(dev)
    return buf


def wg_splits_of_library(lib, Lq, Lk):
    part = lib.mpf_attn_workspace_bytes(Lq, Lk, N, H) - lib.mpf_attn_bwd_aux_bytes(Lq, Lk, N, H, N)
    per_split = N * H * Lq * (HD + 2) * 4
    assert per_split >= 256 and part % 256 == 0
    return part // per_split


def _run_attn(case, dev, lib, call, st):
    Lq, Lk, route, kind = LQ, case["Lk"], case["route"], case["mask"]
    LqP = (Lq + 31) // 32 * 32
    (q, do, k, v), g = _draw(f"attn {Lq} {Lk} {kind}", (Lq, N, E), (Lq, N, E), (Lk, N, E), (Lk, N, E))
    mask = None
    if kind is not None:
        mask = torch.rand((N, Lq, Lk) if kind == "image" else (Lq, Lk), generator=g) < 0.5
        for qi in range(Lq):
            mask[..., qi, (7 * qi) % Lk] = False              # no fully masked row
    if "wg" in case:
        assert wg_splits_of_library(lib, Lq, Lk) == case["wg"], "the case does not reach the split class it is meant for"
    q, do = q.to(dev), do.to(dev)
    if route == "strided":                                   # K | V column halves of one buffer
        kv = _packed({0: k, E: v}, 2 * E, dev)
        kp, vp, row, img = kv.data_ptr(), kv.data_ptr() + 2 * E, N * 2 * E, 2 * E
    else:
        kd, vd = k.to(dev), v.to(dev)
        kp, vp, row, img = kd.data_ptr(), vd.data_ptr(), 0, 0
    if mask is None:
        md = None
    elif case.get("odd"):
        buf = torch.ones(mask.numel() + 16, dtype=torch.bool, device=dev)
        md = buf[1:1 + mask.numel()].view(mask.shape)
        md.copy_(mask)
        assert md.data_ptr() % 2 == 1
    else:
        md = mask.to(dev)
    mp, per = (None if md is None else md.data_ptr()), (1 if kind == "image" else 0)
    if case.get("offset_t"):                                 # views 8 bytes off a 16-byte boundary: the unaligned forms
        kT, vT = (_nan((N * E * Lk + 8,), torch.bfloat16, dev)[4:4 + N * E * Lk].view(N, E, Lk) for _ in range(2))
        assert kT.data_ptr() % 16 == 8 and vT.data_ptr() % 16 == 8
    else:
        kT, vT = (_nan((N, E, Lk), torch.bfloat16, dev) for _ in range(2))
    ws = torch.empty(lib.mpf_attn_workspace_bytes(Lq, Lk, N, H), dtype=torch.uint8, device=dev)
    out, lse = _nan((Lq, N, E), torch.bfloat16, dev), _nan((N, H, Lq), torch.float32, dev)
    qT, doT = (_nan((N, E, LqP), torch.bfloat16, dev) for _ in range(2))
    delta = _nan((N, H, Lq), torch.float32, dev)
    dq = _nan((Lq, N, E), torch.bfloat16, dev)
    res = {}
    if route == "strided":
        call("mpf_attn_transpose2_strided", kp, vp, row, img, kT.data_ptr(), vT.data_ptr(), Lk, Lk, N, E, st)
    else:
        call("mpf_attn_transpose2", kp, vp, kT.data_ptr(), vT.data_ptr(), Lk, Lk, N, E, st)
    ws.fill_(0xFF)
    tail = (Lq, Lk, N, H, HD, SCALE, ws.data_ptr(), ws.numel(), st)
    if route == "strided":
        call("mpf_attn_forward_kv", q.data_ptr(), kp, row, img, vT.data_ptr(), mp, per, out.data_ptr(), lse.data_ptr(), *tail)
    else:
        call("mpf_attn_forward", q.data_ptr(), kp, vT.data_ptr(), mp, per, out.data_ptr(), lse.data_ptr(), *tail)
    res["ws_fwd"] = _sha(ws)
    ws.fill_(0xFF)
    aux = None
    if route == "aux":
        mimgs = 0 if md is None else (N if per else 1)
        aux = torch.full((lib.mpf_attn_bwd_aux_bytes(Lq, Lk, N, H, mimgs),), 0xFF, dtype=torch.uint8, device=dev)
        call("mpf_attn_bwd_prep_aux", q.data_ptr(), do.data_ptr(), out.data_ptr(), lse.data_ptr(), mp, per, Lk, qT.data_ptr(), doT.data_ptr(),
             delta.data_ptr(), aux.data_ptr(), aux.numel(), Lq, LqP, N, H, st)
    else:
        call("mpf_attn_bwd_prep", q.data_ptr(), do.data_ptr(), out.data_ptr(), qT.data_ptr(), doT.data_ptr(), delta.data_ptr(), Lq, LqP, N, H, st)
    head = (kT.data_ptr(), qT.data_ptr(), do.data_ptr(), doT.data_ptr(), mp, per, lse.data_ptr(), delta.data_ptr(), dq.data_ptr())
    tail = (Lq, LqP, Lk, N, H, HD, SCALE, ws.data_ptr(), ws.numel())
    if route == "strided":                                   # dK | untouched columns | dV
        dkv = _nan((Lk, N, 3 * E), torch.bfloat16, dev)
        call("mpf_attn_backward_kv", q.data_ptr(), kp, vp, row, img, *head, dkv.data_ptr(), dkv.data_ptr() + 2 * 2 * E, N * 3 * E, 3 * E, *tail, st)
        dk, dv = dkv[..., :E], dkv[..., 2 * E:]
        res["gap_keeps_prefill"] = bool(torch.isnan(dkv[..., E:2 * E]).all())
    else:
        dk, dv = (_nan((Lk, N, E), torch.bfloat16, dev) for _ in range(2))
        if route == "aux":
            call("mpf_attn_backward_kv_aux", q.data_ptr(), kp, vp, 0, 0, *head, dk.data_ptr(), dv.data_ptr(), 0, 0, *tail, aux.data_ptr(), st)
        else:
            call("mpf_attn_backward", q.data_ptr(), kp, vp, *head, dk.data_ptr(), dv.data_ptr(), *tail, st)
    torch.cuda.synchronize(dev)
    res["ws_bwd"] = _sha(ws)
    if aux is not None:
        res["aux"] = _sha(aux)
    for name, t in dict(kT=kT, vT=vT, out=out, lse=lse, qT=qT, doT=doT, delta=delta, dq=dq, dk=dk, dv=dv).items():
        res[name] = _sha(t)
    return res


def _run_transpose(case, dev, lib, call, st):
    L, LP = case["L"], case["LP"]
    (a, b), _ = _draw(f"transpose {L}", (L, N, E), (L, N, E))
    aT, bT = (_nan((N, E, LP), torch.bfloat16, dev) for _ in range(2))
    if case["strided"]:
        ab = _packed({0: a, E: b}, 2 * E, dev)
        call("mpf_attn_transpose2_strided", ab.data_ptr(), ab.data_ptr() + 2 * E, N * 2 * E, 2 * E, aT.data_ptr(), bT.data_ptr(), L, LP, N, E, st)
    else:
        ad, bd = a.to(dev), b.to(dev)
        call("mpf_attn_transpose2", ad.data_ptr(), bd.data_ptr(), aT.data_ptr(), bT.data_ptr(), L, LP, N, E, st)
    torch.cuda.synchronize(dev)
    return dict(aT=_sha(aT), bT=_sha(bT))


def _run_delta(case, dev, lib, call, st):
    Lq, LqP = LQ, 64
    (q, do, out), _ = _draw("delta", (Lq, N, E), (Lq, N, E), (Lq, N, E))
    q, do, out = q.to(dev), do.to(dev), out.to(dev)
    qT, doT = (_nan((N, E, LqP), torch.bfloat16, dev) for _ in range(2))
    d_prep, d_own = (_nan((N, H, Lq), torch.float32, dev) for _ in range(2))
    call("mpf_attn_bwd_prep", q.data_ptr(), do.data_ptr(), out.data_ptr(), qT.data_ptr(), doT.data_ptr(), d_prep.data_ptr(), Lq, LqP, N, H, st)
    call("mpf_attn_delta", do.data_ptr(), out.data_ptr(), d_own.data_ptr(), Lq, N, H, st)
    torch.cuda.synchronize(dev)
    res = dict(qT=_sha(qT), doT=_sha(doT), delta=_sha(d_own))
    res["delta_same_bits"] = _sha(d_prep) == res["delta"] and bool(torch.isfinite(d_own).all())
    return res


def _run_once(case, dev):
    from mp_former_amd import _lib
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    kernels = []

    def call(name, *args):
        _lib.call(name, dev, *args)
        kernels.append(_lib.last_kernel())

    for k, v in dict(DEFAULTS, **case.get("opts", {})).items():
        _lib.set_option(k, v)
    try:
        _lib.profile_enable(True)
        res = {"attn": _run_attn, "transpose": _run_transpose, "delta": _run_delta}[case["kind"]](case, dev, lib, call, st)
        prof = {}
        for name in PROF_NAMES:
            n, _, by = _lib.profile_get(name)
            if n:
                prof[name] = [n, by]
    finally:
        _lib.profile_enable(False)
        for k, v in DEFAULTS.items():
            _lib.set_option(k, v)
    flags = {k: res.pop(k) for k in FLAGS if k in res}
    return dict(kernels=kernels, prof=prof, all=res, flags=flags)


def run_case(case, dev, hashed=None):
    """One case -> {"kernels", "prof", "hashes", flags...}.  ``hashed`` (the fixture's list): the buffers to hash; None = decide by
    running the case twice (the recorder)."""
    a = _run_once(case, dev)
    flags = a["flags"]
    if hashed is None:
        b = _run_once(case, dev)
        hashed = sorted(k for k, h in a["all"].items() if b["all"][k] == h)
        flags = {k: v and b["flags"][k] for k, v in flags.items()}
    return dict(kernels=a["kernels"], prof=a["prof"], hashes={k: a["all"][k] for k in hashed}, **flags)


def unequal(results):
    """the entries of EQUAL that do not hold in `results` = {case id: run_case's answer}"""
    return [(x, y, name) for x, y, names in EQUAL for name in names
            if name not in results[x]["hashes"] or results[x]["hashes"][name] != results[y]["hashes"].get(name)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from mp_former_amd import _lib
    out = {"device": torch.cuda.get_device_name(dev), "cases": {}}
    wrong = []
    for case in CASES:
        r = run_case(case, dev)
        print(f"{case['id']:<42} {' | '.join(r['kernels'])}\n    prof {r['prof']} hashed {sorted(r['hashes'])} "
              f"flags { {k: r[k] for k in FLAGS if k in r} }", flush=True)
        for flag in FLAGS:
            if not r.get(flag, True):
                wrong.append(f"{case['id']}: {flag} is false")
        out["cases"][case["id"]] = r
    for case in CASES:                                       # every buffer reproduces: no atomics, fixed merge order
        want = {"attn": set(_DENSE) | {"ws_fwd", "ws_bwd"} | ({"aux"} if case.get("route") == "aux" else set()), "transpose": {"aT", "bT"},
                "delta": {"qT", "doT", "delta"}}[case["kind"]]
        missing = want - set(out["cases"][case["id"]]["hashes"])
        if missing:
            wrong.append(f"{case['id']}: two runs differ in {sorted(missing)}")
    wrong += [f"{x} != {y} in {name}" for x, y, name in unequal(out["cases"])]
    print(f"library {_lib.LIB_PATH}; {len(CASES)} cases")
    if wrong:
        raise SystemExit("cases that break a contract of the family:\n  " + "\n  ".join(wrong))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
