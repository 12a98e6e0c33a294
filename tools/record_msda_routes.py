"""Route table of the multi-scale deformable attention (MSDA) host layer (csrc/msda_entry.hip in front of msda.hip, msda_block.hip
and msda_bwd_binned.hip): which kernels every entry point runs on the smallest problems that reach each route, and what they write.

    python tools/record_msda_routes.py [--out tests/golden/msda_routes.json]

runs CASES on cuda:0 and writes the fixture that tests/test_msda_routes_gpu.py compares the library against.  Record it from the
library BEFORE a change of the host layer; the test then pins the change.  All cases use M = 2 heads and N <= 2; the inputs are
host draws of a generator seeded by the case id.

Per case the fixture holds
    kernels   mpf_last_kernel after each call of the case
    prof      the launch profiler's records of the MSDA kernels: name -> [launches, logged algorithmic bytes]
    stats     the route counters of the blocked kernels (mpf_msda_stats) that two runs agree on
    hashes    SHA-256 of every output that the library reproduces bit for bit.  The recorder decides this by running the case
              twice, the second time with ``msda_bin_reverse = 1`` (another arrival order in the blocked backward).  grad_value is a
              candidate only on the sorted no-spill route: everywhere else it is a float-atomic sum or a sum in arrival order.
    bounds    names of the outputs compared with the library's own generic<double> result on the same inputs (every output that
              is not all-NaN by contract), under the bounds of tests/test_msda_gpu.py: out rtol 1e-4 / atol 1e-5, grad_attn 1e-4 /
              1e-4, grad_loc 1e-3 / 5e-3 away from pixel borders, grad_value rtol 1e-3 / atol 2e-4 max(1, max|ref| / 50) (the spill
              case: 2e-3 / 2e-3 max|ref|), grad_raw 2e-3 / 2e-3, loc 1e-6 / 1e-6, attn 1e-5 / 1e-6.  ``run_case`` returns the worst
              |got - ref| / (atol + rtol |ref|) per output, which must be <= 1.
    amax      per amax slot "tight" (slot >= max |output| and within one fp32 rounding of it, checked by the test) or its hash
    and the case's own flags: all_nan, geometry_ok, second_call_same_bits, gap_rows_zero, spill_entries_positive.
"""
import argparse
import ctypes
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

FIXTURE = os.path.join(ROOT, "tests", "golden", "msda_routes.json")

M = 2
LEVELS = {1: [(13, 7)], 2: [(6, 4), (3, 2)], 3: [(6, 4), (3, 2), (12, 9)], 4: [(4, 4), (8, 8), (16, 16), (32, 32)]}
FIVE = [(4, 4), (2, 2), (3, 3), (2, 3), (1, 2)]
SPILL = [(8, 8), (16, 16), (32, 32)]
DEFAULTS = {"msda_fwd_variant": 0, "msda_bwd_variant": 0, "msda_block_disable": 0, "msda_fuse_prep": 1, "msda_bwd_sorted": 0,
            "msda_bin_reverse": 0}
PROF_NAMES = ("msda_fwd_tiled_f32<32,1>", "msda_fwd_tiled_f32<32,2>", "msda_fwd_tiled_f32<32,4>", "msda_fwd_generic<float>",
              "msda_fwd_generic<double>", "msda_fwd_block_kernel", "msda_bwd_tiled_f32<32,1>", "msda_bwd_tiled_f32<32,2>",
              "msda_bwd_tiled_f32<32,4>", "msda_bwd_generic<float>", "msda_bwd_generic<double>", "msda_bwd_bin_kernel",
              "msda_sort_runs_kernel", "msda_bwd_tile_kernel", "msda_bwd_push_kernel", "msda_bwd_fill_kernel", "msda_bwd_pull_kernel",
              "amax")
U = 2.0 ** -23      # one fp32 rounding


def _cases():
    c = []
    three, tiny4 = LEVELS[3], [(2, 2)] * 4
    for d, plain in (("fwd", "forward"), ("bwd", "backward")):
        key = f"msda_{d}_variant"
        c.append(dict(id=f"{d} fp64 generic", entry=plain, lv=LEVELS[2], dtype="f64"))
        c.append(dict(id=f"{d} fp32 D=30 generic", entry=plain, lv=LEVELS[2], D=30))
        for v in (0, 3, 2, 4, 1):
            c.append(dict(id=f"{d} D=32 variant {v}", entry=plain, lv=three, opts={key: v}))
        for v in (2, 3):
            c.append(dict(id=f"{d} L*P=40 variant {v}", entry=plain, lv=tiny4, P=10, opts={key: v}))
        hs_entry = "forward_hs" if d == "fwd" else "backward_ws"
        for L in (1, 2, 3, 4):
            c.append(dict(id=f"{d} hs blocked L={L} Lq=S", entry=hs_entry, lv=LEVELS[L]))
            c.append(dict(id=f"{d} hs blocked L={L} Lq=300", entry=hs_entry, lv=LEVELS[L], Lq=300))
        c.append(dict(id=f"{d} hs block_disable", entry=hs_entry, lv=three, opts={"msda_block_disable": 1}))
        c.append(dict(id=f"{d} hs L=5", entry=hs_entry, lv=FIVE))
        dev = plain + "_dev"
        c.append(dict(id=f"{d} dev contiguous", entry=dev, lv=three))
        c.append(dict(id=f"{d} dev gap", entry=dev, lv=three, layout="gap"))
        c.append(dict(id=f"{d} dev overlap", entry=dev, lv=three, layout="overlap"))
        c.append(dict(id=f"{d} dev P=8 falls back", entry=dev, lv=three, P=8))
    c.append(dict(id="fwd hs P=8 declines", entry="forward_hs", lv=three, P=8))
    c.append(dict(id="fwd hs shapes sum != S declines", entry="forward_hs", lv=three, hs_wrong=True))
    c.append(dict(id="fwd raw_hs fused", entry="forward_raw_hs", lv=three, opts={"msda_fuse_prep": 1}))
    c.append(dict(id="fwd raw_hs prep + blocked", entry="forward_raw_hs", lv=three, opts={"msda_fuse_prep": 0}))
    c.append(dict(id="fwd raw without host shapes", entry="forward_raw", lv=three))
    c.append(dict(id="fwd dev second call same workspace", entry="forward_dev", lv=three, twice=True))
    c.append(dict(id="bwd hs sorted", entry="backward_ws", lv=three, opts={"msda_bwd_sorted": 1}))
    c.append(dict(id="bwd hs spill", entry="backward_ws", lv=SPILL, N=1, mode="point"))
    c.append(dict(id="bwd ws_raw binned", entry="backward_ws_raw", lv=three))
    c.append(dict(id="bwd ws_raw_o blocked amax", entry="backward_ws_raw_o", lv=three, slots=True))
    c.append(dict(id="bwd ws_raw_o blocked NULL slots", entry="backward_ws_raw_o", lv=three))
    c.append(dict(id="bwd ws_raw_o block_disable amax", entry="backward_ws_raw_o", lv=three, slots=True, opts={"msda_block_disable": 1}))
    ids = [x["id"] for x in c]
    assert len(set(ids)) == len(ids)
    return c


CASES = _cases()


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def _problem(case):
    """host draws of one case (fp64; cast to the case's dtype on upload)"""
    rng = np.random.default_rng(zlib.crc32(case["id"].encode()))
    lv = case["lv"]
    L, P, D, N = len(lv), case.get("P", 4), case.get("D", 32), case.get("N", 2)
    hw = [h * w for h, w in lv]
    starts = [int(sum(hw[:l])) for l in range(L)]
    S = sum(hw)
    if case.get("layout") == "gap":            # five rows that no level owns after level 0, three at the end
        starts = [s + (5 if l else 0) for l, s in enumerate(starts)]
        S += 8
    elif case.get("layout") == "overlap":
        starts[1] -= 3
    Lq = case.get("Lq", sum(hw))
    z = dict(N=N, S=S, M=M, D=D, L=L, Lq=Lq, P=P, lv=lv, starts=starts)
    z["value"] = rng.standard_normal((N, S, M, D))
    if case.get("mode") == "point":            # every sample on one spot: the runs of the tiles around it overflow
        z["loc"] = 0.37 + rng.uniform(0.0, 0.01, (N, Lq, M, L, P, 2))
    else:
        z["loc"] = rng.uniform(-0.15, 1.15, (N, Lq, M, L, P, 2))
    lg = rng.standard_normal((N, Lq, M, L * P))
    e = np.exp(lg - lg.max(-1, keepdims=True))
    z["attn"] = (e / e.sum(-1, keepdims=True)).reshape(N, Lq, M, L, P)
    z["go"] = rng.standard_normal((N, Lq, M * D))
    if case["entry"].startswith("forward_raw"):
        raw = rng.standard_normal((N * Lq, M * L * P * 3)).astype(np.float32).astype(np.float64)
        raw[:, :M * L * P * 2] *= 3.0
        ref = rng.uniform(0.0, 1.0, (Lq, 2)).astype(np.float32).astype(np.float64)
        z["raw"], z["ref"] = raw, ref
        wh = np.array([[w, h] for h, w in lv], dtype=np.float64)
        lgt = raw[:, M * L * P * 2:].reshape(N, Lq, M, L * P)
        e = np.exp(lgt - lgt.max(-1, keepdims=True))
        z["attn"] = (e / e.sum(-1, keepdims=True)).reshape(N, Lq, M, L, P)
        z["loc"] = ref[None, :, None, None, None, :] + raw[:, :M * L * P * 2].reshape(N, Lq, M, L, P, 2) / wh[None, None, None, :, None, :]
    # the fp32 entries see the fp32 rounding of the draws; the fp64 reference starts from the same numbers
    if case.get("dtype") != "f64":
        for k in ("value", "loc", "attn", "go"):
            z[k] = z[k].astype(np.float32).astype(np.float64)
    return z


def _smooth(z):
    """[N, Lq, M, L, P] mask of the sampling points away from integer pixel coordinates, where d out / d loc jumps"""
    sh = np.array(z["lv"], dtype=np.float64)
    x = z["loc"][..., 0] * sh[None, None, None, :, None, 1] - 0.5
    y = z["loc"][..., 1] * sh[None, None, None, :, None, 0] - 0.5
    return ~((np.abs(x - np.round(x)) < 1e-4) | (np.abs(y - np.round(y)) < 1e-4))


def _dev_t(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(dev)


def _sizes(z, dt):
    return (z["N"], z["S"], z["M"], z["D"], z["L"], z["Lq"], z["P"], dt)


def _reference(z, dev):
    """the library's generic<double> kernels on the same inputs -> numpy fp64 dict"""
    from mp_former_amd import _lib
    st = _lib.stream_ptr(dev)
    t = {k: _dev_t(z[k], dev) for k in ("value", "loc", "attn", "go")}
    shapes, lsi = _dev_t(np.array(z["lv"], dtype=np.int64), dev), _dev_t(np.array(z["starts"], dtype=np.int64), dev)
    out = torch.zeros((z["N"], z["Lq"], M * z["D"]), dtype=torch.float64, device=dev)
    gv, gl, ga = torch.zeros_like(t["value"]), torch.zeros_like(t["loc"]), torch.zeros_like(t["attn"])
    _lib.call("mpf_msda_forward", dev, t["value"].data_ptr(), shapes.data_ptr(), lsi.data_ptr(), t["loc"].data_ptr(), t["attn"].data_ptr(),
              out.data_ptr(), *_sizes(z, _lib.MPF_F64), st)
    assert _lib.last_kernel() == "msda_fwd_generic<double>"
    _lib.call("mpf_msda_backward", dev, t["value"].data_ptr(), shapes.data_ptr(), lsi.data_ptr(), t["loc"].data_ptr(), t["attn"].data_ptr(),
              t["go"].data_ptr(), gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), *_sizes(z, _lib.MPF_F64), st)
    assert _lib.last_kernel() == "msda_bwd_generic<double>"
    r = dict(out=out, gv=gv, gl=gl, ga=ga)
    r = {k: v.cpu().numpy() for k, v in r.items()}
    # the raw forms' chain rule (ops/modules/ms_deform_attn.py:103-117): loc = ref + off / (W, H), attn = softmax(logits)
    wh = np.array([[w, h] for h, w in z["lv"]], dtype=np.float64)
    g_off = r["gl"] / wh[None, None, None, :, None, :]
    a, g = z["attn"], r["ga"]
    g_lg = a * (g - (a * g).sum((-1, -2), keepdims=True))
    n = z["N"] * z["Lq"]
    r["graw"] = np.concatenate((g_off.reshape(n, -1), g_lg.reshape(n, -1)), 1)
    r["loc"], r["attn"] = z["loc"], z["attn"]
    return r


_TOL = {"out": (1e-4, 1e-5), "ga": (1e-4, 1e-4), "gl": (1e-3, 5e-3), "graw": (2e-3, 2e-3), "loc": (1e-6, 1e-6), "attn": (1e-5, 1e-6)}


def _worst(name, got, ref, z, case):
    """max |got - ref| / (atol + rtol |ref|) under the bound of `name`"""
    got = got.double().cpu().numpy().reshape(ref.shape)
    if name == "gv":
        mx = float(np.abs(ref).max())
        rtol, atol = (2e-3, 2e-3 * mx) if case.get("mode") == "point" else (1e-3, 2e-4 * max(1.0, mx / 50.0))
    else:
        rtol, atol = _TOL[name]
    ratio = np.abs(got - ref) / (atol + rtol * np.abs(ref))
    if name == "gl":
        ratio = ratio[_smooth(z)]
    elif name == "graw":
        n_off = M * z["L"] * z["P"] * 2
        off = ratio[:, :n_off].reshape(z["N"], z["Lq"], M, z["L"], z["P"], 2)[_smooth(z)]
        ratio = np.concatenate((off.reshape(-1), ratio[:, n_off:].reshape(-1)))
    return float(ratio.max()) if np.isfinite(ratio).all() else float("inf")


def _run_once(case, z, ref, dev, reverse):
    from mp_former_amd import _lib
    from mp_former_amd.gemm3 import amax_slots, amax_value
    lib, st, entry = _lib.lib(), _lib.stream_ptr(dev), case["entry"]
    f64 = case.get("dtype") == "f64"
    tdt, dt = (torch.float64, _lib.MPF_F64) if f64 else (torch.float32, _lib.MPF_F32)
    N, S, D, L, Lq, P = z["N"], z["S"], z["D"], z["L"], z["Lq"], z["P"]
    t = {k: _dev_t(z[k], dev, tdt) for k in ("value", "loc", "attn", "go")}
    shapes, lsi = _dev_t(np.array(z["lv"], dtype=np.int64), dev), _dev_t(np.array(z["starts"], dtype=np.int64), dev)
    hs_np = np.array(z["lv"], dtype=np.int64)
    if case.get("hs_wrong"):
        hs_np[0, 0] += 1
    hs = torch.from_numpy(hs_np)          # host memory
    new = lambda *shape: torch.full(shape, -7.0, dtype=tdt, device=dev)
    out, gv, gl, ga = new(N, Lq, M * D), new(N, S, M, D), new(N, Lq, M, L, P, 2), new(N, Lq, M, L, P)
    graw, loc_o, attn_o = new(N * Lq, M * L * P * 3), new(N, Lq, M, L, P, 2), new(N, Lq, M, L, P)
    sizes = _sizes(z, dt)
    head = (t["value"].data_ptr(), shapes.data_ptr(), lsi.data_ptr())
    la = (t["loc"].data_ptr(), t["attn"].data_ptr())
    res = dict(kernels=[], flags={})
    outputs, slots, ws = {}, None, None
    fwd_out = None
    if entry == "backward_ws_raw_o":      # the forward result the raw backward needs, before anything is counted
        fwd_out = torch.zeros((N, Lq, M * D), dtype=tdt, device=dev)
        _lib.call("mpf_msda_forward", dev, *head, *la, fwd_out.data_ptr(), *sizes, st)
    for k, v in dict(DEFAULTS, **case.get("opts", {})).items():
        _lib.set_option(k, v)
    _lib.set_option("msda_bin_reverse", 1 if reverse else 0)
    _lib.set_option("msda_stats", 1)
    try:
        _lib.msda_stats(reset=True)
        _lib.profile_enable(True)

        def call(name, *args):
            _lib.call(name, dev, *args)
            res["kernels"].append(_lib.last_kernel())

        if entry in ("forward", "forward_hs"):
            mid = (hs.data_ptr(),) if entry == "forward_hs" else ()
            call("mpf_msda_" + entry, *head, *mid, *la, out.data_ptr(), *sizes, st)
            outputs = dict(out=out)
        elif entry in ("forward_raw", "forward_raw_hs"):
            raw, rp = _dev_t(z["raw"], dev, tdt), _dev_t(z["ref"], dev, tdt)
            mid = (hs.data_ptr(),) if entry == "forward_raw_hs" else ()
            call("mpf_msda_" + entry, *head, *mid, raw.data_ptr(), rp.data_ptr(), loc_o.data_ptr(), attn_o.data_ptr(), out.data_ptr(),
                 *sizes, st)
            outputs = dict(out=out, loc=loc_o, attn=attn_o)
        elif entry == "forward_dev":
            need = lib.mpf_msda_dev_workspace_bytes(N, S, M, L, Lq, P, 0)
            ws = torch.zeros(max(need, 1024), dtype=torch.uint8, device=dev)
            call("mpf_msda_forward_dev", *head, *la, out.data_ptr(), *sizes, ws.data_ptr(), ws.numel(), st)
            outputs = dict(out=out)
            if case.get("twice"):
                again = new(N, Lq, M * D)
                call("mpf_msda_forward_dev", *head, *la, again.data_ptr(), *sizes, ws.data_ptr(), ws.numel(), st)
                res["flags"]["second_call_same_bits"] = _sha(again) == _sha(out)
        elif entry == "backward":
            call("mpf_msda_backward", *head, *la, t["go"].data_ptr(), gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), *sizes, st)
            outputs = dict(gv=gv, gl=gl, ga=ga)
        elif entry == "backward_dev":
            need = lib.mpf_msda_dev_workspace_bytes(N, S, M, L, Lq, P, 1)
            ws = torch.zeros(max(need, 1024), dtype=torch.uint8, device=dev)
            call("mpf_msda_backward_dev", *head, *la, t["go"].data_ptr(), gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), *sizes,
                 ws.data_ptr(), ws.numel(), st)
            outputs = dict(gv=gv, gl=gl, ga=ga)
        else:
            need = lib.mpf_msda_backward_workspace_bytes(N, M, L, Lq, P, hs.data_ptr())
            assert need > 0, case["id"]
            wsb = torch.zeros(need, dtype=torch.uint8, device=dev)
            body = (t["value"].data_ptr(), hs.data_ptr(), *la, t["go"].data_ptr())
            if entry == "backward_ws":
                call("mpf_msda_backward_ws", *body, gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), *sizes, wsb.data_ptr(), need, st)
                outputs = dict(gv=gv, gl=gl, ga=ga)
            elif entry == "backward_ws_raw":
                call("mpf_msda_backward_ws_raw", *body, gv.data_ptr(), graw.data_ptr(), *sizes, wsb.data_ptr(), need, st)
                outputs = dict(gv=gv, graw=graw)
            else:
                slots = amax_slots(2, dev) if case.get("slots") else None
                call("mpf_msda_backward_ws_raw_o", *body, fwd_out.data_ptr(), gv.data_ptr(), graw.data_ptr(), *sizes, wsb.data_ptr(), need,
                     _lib.ptr(slots[0]) if slots is not None else None, _lib.ptr(slots[1]) if slots is not None else None, st)
                outputs = dict(gv=gv, graw=graw)
        torch.cuda.synchronize()
        res["prof"] = {}
        for name in PROF_NAMES:
            n, _, by = _lib.profile_get(name)
            if n:
                res["prof"][name] = [n, by]
        res["stats"] = _lib.msda_stats(reset=True)
    finally:
        _lib.profile_enable(False)
        _lib.set_option("msda_stats", 0)
        for k, v in DEFAULTS.items():
            _lib.set_option(k, v)
    if ws is not None:
        geo = (ctypes.c_int * 10)()
        _lib.check(lib.mpf_msda_dev_geometry(ws.data_ptr(), geo, 10), "mpf_msda_dev_geometry")
        fell_back = "block" not in res["kernels"][0]
        if not fell_back:
            res["flags"]["geometry_ok"] = int(geo[0])
    nan = case.get("layout") == "overlap"
    if nan:
        res["flags"]["all_nan"] = all(bool(torch.isnan(v).all()) for v in outputs.values())
    if case.get("layout") == "gap" and "gv" in outputs:
        owned = np.zeros(S, dtype=bool)
        for (h, w), s0 in zip(z["lv"], z["starts"]):
            owned[s0:s0 + h * w] = True
        res["flags"]["gap_rows_zero"] = bool((outputs["gv"][:, torch.from_numpy(~owned).to(dev)] == 0).all())
    if case.get("mode") == "point":
        res["flags"]["spill_entries_positive"] = res["stats"]["spill_entries"] > 0
    res["all"] = {k: _sha(v) for k, v in outputs.items()}
    res["bounds"] = {} if nan else {k: _worst(k, v, ref[k], z, case) for k, v in outputs.items()}
    res["amax"] = {}
    if slots is not None:
        for name, slot, data in (("graw_amax", slots[0], graw), ("gv_amax", slots[1], gv)):
            got, true = float(amax_value(slot)), float(data.abs().max())
            res["amax"][name] = dict(tight=bool(true <= got <= true * (1.0 + U)), sha=_sha(amax_value(slot).reshape(1)))
    return res


def _gv_candidate(case):
    return case.get("opts", {}).get("msda_bwd_sorted") == 1 and case.get("mode") != "point"


def run_case(case, dev, hashed=None):
    """One case -> {"kernels", "prof", "stats", "hashes", "bounds", "amax", flags...}.  ``hashed`` (the fixture's list): the outputs to
    hash; None = decide by running twice, the second time with msda_bin_reverse = 1 (the recorder)."""
    z = _problem(case)
    ref = _reference(z, dev)
    a = _run_once(case, z, ref, dev, reverse=False)
    stats = a["stats"]
    if hashed is None:
        b = _run_once(case, z, ref, dev, reverse=True)
        hashed = sorted(k for k, h in a["all"].items() if b["all"][k] == h and (k != "gv" or _gv_candidate(case)))
        stats = {k: v for k, v in stats.items() if b["stats"][k] == v}
        for k, v in a["amax"].items():
            v["tight"] = v["tight"] and b["amax"][k]["tight"]
    amax = {k: ("tight" if v["tight"] else v["sha"]) for k, v in a["amax"].items()}
    return dict(kernels=a["kernels"], prof=a["prof"], stats=stats, hashes={k: a["all"][k] for k in hashed}, bounds=a["bounds"], amax=amax,
                **a["flags"])


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
        print(f"{case['id']:<42} {' | '.join(r['kernels']):<60} hashed {sorted(r['hashes'])} "
              f"bounds { {k: round(v, 3) for k, v in r['bounds'].items()} } amax {r['amax']} stats {r['stats']}", flush=True)
        off = {k: v for k, v in r["bounds"].items() if not v <= 1.0}
        if off:
            wrong.append(f"{case['id']}: outside the bounds against generic<double> (|got - ref| / bound): {off}")
        for flag in ("all_nan", "second_call_same_bits", "gap_rows_zero", "spill_entries_positive"):
            if not r.get(flag, True):
                wrong.append(f"{case['id']}: {flag} is false")
        if case.get("layout") == "overlap" and r.get("geometry_ok") != 0:
            wrong.append(f"{case['id']}: geometry ok = {r.get('geometry_ok')}")
        r["bounds"] = sorted(r["bounds"])          # (the ratios vary from run to run: the fixture keeps the names)
        out["cases"][case["id"]] = r
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
