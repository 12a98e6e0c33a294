"""Route table of the 256-column residual LayerNorm host layer (csrc/elementwise.hip: mpf_res_ln256_*, mpf_ln_partial_reduce):
the bits every entry point writes for the smallest row counts that reach each code path.

    python tools/record_res_ln_routes.py [--out tests/golden/res_ln_routes.json]

runs CASES on cuda:0 and writes the fixture that tests/test_res_ln_routes_gpu.py compares the library against.  Record it from
the library BEFORE a change of the host layer; the test then pins the change.  The inputs are host draws of a generator seeded
by the case id and the grid rule does not read the CU count, so every hash is device-independent.

Row counts (grid rule: rows per workgroup = ceil(rows / 1024) rounded up to 4, workgroups = ceil(rows / that)):
    1, 5         three of a workgroup's four waves idle; a ragged last workgroup
    125          32 workgroups: the 16-deep unrolled loop of the last-arriving workgroup runs once and leaves a tail
    901          226 workgroups: the 8-deep loop of ln_partial_reduce_kernel runs for slice 0 only
    1024, 1025   the switch of resln.py between _det and _ws; 4 rows per workgroup still
    4097         8 rows per workgroup

Per case the fixture holds the kernel name (mpf_last_kernel) and the SHA-256 of every output that is a function of the inputs:
s_out / y32 / y16 / y_plus / mean / rstd and the bound slots forward; ds32 / ds16, dgamma / dbeta, the workgroups' partial sums
and the value of the amax slot backward.  dgamma / dbeta of mpf_res_ln256_backward are float-atomic sums that no build
reproduces bit for bit: they are checked against the fp64 sum of the partials that _partial writes for the same inputs, within
the rounding of an fp32 sum of that many terms in any order (``sums``: worst |got - exact| / bound, must be <= 1; the fixture
keeps the names).  _det: the ticket word read back after the call (must be zero) and whether a second call on the same
workspace wrote the same bits.
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

FIXTURE = os.path.join(ROOT, "tests", "golden", "res_ln_routes.json")

ROWS = (1, 5, 125, 901, 1024, 1025, 4097)
BACKWARDS = ("atomics", "ws", "ws_amax", "partial", "partial_amax", "det")
OPERANDS = ("gy_plus", "gy16", "gy16+gy_plus", "gy32", "gy32+gy_plus", "gy32+gy16", "gy32+gy16+gy_plus")     # switch order 1..7
DS = ("ds32", "ds16", "ds32+ds16")
EPS = 1e-5
U = 2.0 ** -24      # unit roundoff of fp32


def grid_rule(rows):
    """(rows per workgroup, workgroups) of the backward kernels, restated"""
    rpb = (-(-rows // 1024) + 3) // 4 * 4
    return rpb, -(-rows // rpb)


def _cases():
    c = []
    for e in BACKWARDS:
        for i, ops in enumerate(OPERANDS):
            c.append(dict(id=f"bwd {e} 125 {ops}", entry=e, rows=125, ops=ops, ds=DS[i % 3]))
        for rows in ROWS:
            if not (e == "det" and rows > 1025):
                c.append(dict(id=f"bwd {e} rows {rows}", entry=e, rows=rows, ops="gy32", ds="ds32"))
    c.append(dict(id="bwd partial_amax 125 no amax slot", entry="partial_amax", rows=125, ops="gy32", ds="ds32", no_amax=True))
    c.append(dict(id="reduce 3 slots, stride > slot", entry="reduce", rows=125, n_ln=3, pad_bytes=256))
    for t in ("none", "f32", "bf16"):
        for padd in (False, True):
            for rows in (1, 5, 4097):
                c.append(dict(id=f"fwd t={t}{' +padd' if padd else ''} rows {rows}", entry="fwd", rows=rows, t=t, padd=padd))
    c.append(dict(id="fwd_b y_bound", entry="fwd_b", rows=5, t="bf16", padd=False))
    c.append(dict(id="fwd_b y_bound +padd, no yplus_bound", entry="fwd_b", rows=5, t="none", padd=True))
    c.append(dict(id="fwd_b y_bound + yplus_bound", entry="fwd_b", rows=5, t="f32", padd=True, yplus_bound=True))
    ids = [x["id"] for x in c]
    assert len(set(ids)) == len(ids)
    return c


CASES = _cases()


def _sha(t):
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


class _Inputs:
    """host draws of one case, in call order, moved to the device"""

    def __init__(self, cid, dev):
        self.rng = np.random.default_rng(zlib.crc32(cid.encode()))
        self.dev = dev

    def f32(self, *shape, scale=1.0, shift=0.0):
        return torch.from_numpy(self.rng.standard_normal(shape, dtype=np.float32) * np.float32(scale) + np.float32(shift)).to(self.dev)

    def bf16(self, *shape):
        return self.f32(*shape).to(torch.bfloat16)

    def positive(self, *shape):
        return torch.from_numpy(self.rng.uniform(0.5, 2.0, shape).astype(np.float32)).to(self.dev)


def _amax_sha(slot):
    from mp_former_amd.gemm3 import amax_value
    return _sha(amax_value(slot).reshape(1))


def _run_forward(case, x):
    from mp_former_amd import _lib, gemm3 as g
    dev, rows = x.dev, case["rows"]
    xin = x.f32(rows, 256)
    t = {"none": None, "f32": x.f32, "bf16": x.bf16}[case["t"]]
    t = t(rows, 256) if t else None
    gamma, beta = x.f32(256, shift=1.0), x.f32(256, scale=0.1)
    padd = x.f32(3, 256) if case["padd"] else None
    new = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    s_out, y32, y16, mean, rstd = new(rows, 256), new(rows, 256), new(rows, 256, dtype=torch.bfloat16), new(rows), new(rows)
    y_plus = new(rows, 256) if case["padd"] else None
    args = (xin.data_ptr(), _lib.ptr(t), _lib.DTYPE[t.dtype] if t is not None else 0, gamma.data_ptr(), beta.data_ptr(), s_out.data_ptr(),
            y32.data_ptr(), y16.data_ptr(), mean.data_ptr(), rstd.data_ptr(), rows, EPS, _lib.ptr(padd), 3 if case["padd"] else 0,
            _lib.ptr(y_plus))
    out = {}
    if case["entry"] == "fwd_b":
        y_bound = g.amax_slots(1, dev)[0]
        yplus_bound = g.amax_slots(1, dev)[0] if case.get("yplus_bound") else None
        padd_amax = g.amax(padd) if yplus_bound is not None else None
        _lib.call("mpf_res_ln256_forward_b", dev, *args, y_bound.data_ptr(), _lib.ptr(padd_amax), _lib.ptr(yplus_bound), _lib.stream_ptr(dev))
        kernel = _lib.last_kernel()
        out["y_bound"] = _amax_sha(y_bound)
        if yplus_bound is not None:
            out["yplus_bound"] = _amax_sha(yplus_bound)
    else:
        _lib.call("mpf_res_ln256_forward", dev, *args, _lib.stream_ptr(dev))
        kernel = _lib.last_kernel()
    out.update(s_out=_sha(s_out), y32=_sha(y32), y16=_sha(y16), mean=_sha(mean), rstd=_sha(rstd))
    if y_plus is not None:
        out["y_plus"] = _sha(y_plus)
    return kernel, out, {}


def _reduce(part, stride_bytes, rows, n_ln):
    from mp_former_amd import _lib
    out = torch.zeros((n_ln, 2, 256), dtype=torch.float32, device=part.device)
    _lib.call("mpf_ln_partial_reduce", part.device, part.data_ptr(), stride_bytes, rows, n_ln, out.data_ptr(), _lib.stream_ptr(part.device))
    return out


def _run_reduce(case, x):
    rows, n = case["rows"], case["n_ln"]
    slot = grid_rule(rows)[1] * 512
    stride = slot + case["pad_bytes"] // 4
    part = x.f32(n, stride)
    out = _reduce(part, stride * 4, rows, n)
    return None, {"out": _sha(out)}, {}          # (the entry point names no kernel: mpf_last_kernel is the previous call's)


def _run_backward(case, x):
    from mp_former_amd import _lib, gemm3 as g
    dev, rows, entry = x.dev, case["rows"], case["entry"]
    ops = case["ops"].split("+")
    s, mean, rstd, gamma = x.f32(rows, 256), x.f32(rows, scale=0.1), x.positive(rows), x.f32(256, shift=1.0)
    gy32 = x.f32(rows, 256) if "gy32" in ops else None
    gy16 = x.bf16(rows, 256) if "gy16" in ops else None
    gy_plus = x.f32(rows, 256) if "gy_plus" in ops else None
    new = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
    ds32 = new(rows, 256) if "ds32" in case["ds"] else None
    ds16 = new(rows, 256, dtype=torch.bfloat16) if "ds16" in case["ds"] else None
    st, lib = _lib.stream_ptr(dev), _lib.lib()
    floats = grid_rule(rows)[1] * 512                      # of the partial sums: [workgroup][dgamma | dbeta][256]
    nbytes = lib.mpf_res_ln256_backward_workspace_bytes(rows)
    assert nbytes == floats * 4
    head = (s.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(), _lib.ptr(gy32), _lib.ptr(gy16), _lib.ptr(gy_plus))
    dgb = new(2, 256)
    out, sums, extra = {}, {}, {}

    def partials(d32, d16, amax):
        part = new(floats)
        _lib.call("mpf_res_ln256_backward_partial_amax", dev, *head, _lib.ptr(d32), _lib.ptr(d16), rows, part.data_ptr(), nbytes,
                  _lib.ptr(amax), st)
        return part

    if entry == "atomics":
        _lib.call("mpf_res_ln256_backward", dev, *head, _lib.ptr(ds32), _lib.ptr(ds16), dgb[0].data_ptr(), dgb[1].data_ptr(), rows, st)
        kernel = _lib.last_kernel()
        # the float-atomic sums against the fp64 sum of the partials of the same inputs: an fp32 sum of `blocks` terms in any
        # order is within blocks * u * sum|term| of the exact one
        part = partials(new(rows, 256), None, None).view(-1, 2, 256).double()
        bound = part.shape[0] * U * part.abs().sum(0) + 1e-37
        sums["dgamma_dbeta"] = float(((dgb.double() - part.sum(0)).abs() / bound).max())
    elif entry in ("ws", "ws_amax"):
        ws = new(floats)
        tail = ()
        if entry == "ws_amax":
            slot = g.amax_slots(1, dev)[0]
            tail = (slot.data_ptr(),)
        _lib.call("mpf_res_ln256_backward_" + entry, dev, *head, _lib.ptr(ds32), _lib.ptr(ds16), dgb[0].data_ptr(), dgb[1].data_ptr(), rows,
                  ws.data_ptr(), nbytes, *tail, st)
        kernel = _lib.last_kernel()
        out.update(partials=_sha(ws), dgamma_dbeta=_sha(dgb))
        if entry == "ws_amax":
            out["ds_amax"] = _amax_sha(slot)
    elif entry in ("partial", "partial_amax"):
        part = new(floats)
        tail = ()
        if entry == "partial_amax":
            slot = None if case.get("no_amax") else g.amax_slots(1, dev)[0]
            tail = (_lib.ptr(slot),)
        _lib.call("mpf_res_ln256_backward_" + entry, dev, *head, _lib.ptr(ds32), _lib.ptr(ds16), rows, part.data_ptr(), nbytes, *tail, st)
        kernel = _lib.last_kernel()
        out.update(partials=_sha(part), dgamma_dbeta=_sha(_reduce(part, nbytes, rows, 1)))
        if entry == "partial_amax" and slot is not None:
            out["ds_amax"] = _amax_sha(slot)
    else:
        det_bytes = lib.mpf_res_ln256_backward_det_workspace_bytes(rows)
        assert det_bytes == 256 + nbytes
        ws = new(64 + floats)                              # ticket word (zero on entry), partials from byte 256
        call = lambda o: _lib.call("mpf_res_ln256_backward_det", dev, *head, _lib.ptr(ds32), _lib.ptr(ds16), o.data_ptr(), rows,
                                   ws.data_ptr(), det_bytes, st)
        call(dgb)
        kernel = _lib.last_kernel()
        out.update(partials=_sha(ws[64:]), dgamma_dbeta=_sha(dgb))
        extra["ticket_after"] = int(ws[:1].view(torch.int32).item())
        first = [_sha(t) for t in (ds32, ds16, dgb) if t is not None]
        for t in (ds32, ds16):
            if t is not None:
                t.fill_(-1.0)
        again = new(2, 256)
        call(again)
        extra["second_call_same_bits"] = first == [_sha(t) for t in (ds32, ds16, again) if t is not None]
    if ds32 is not None:
        out["ds32"] = _sha(ds32)
    if ds16 is not None:
        out["ds16"] = _sha(ds16)
    return kernel, out, dict(sums=sums, **extra)


_RUN = {"fwd": _run_forward, "fwd_b": _run_forward, "reduce": _run_reduce}


def run_case(case, dev):
    """-> {"kernel", "hashes": {buffer: sha256}, "sums": {buffer: |got - exact| / bound}[, "ticket_after", "second_call_same_bits"]}"""
    kernel, hashes, extra = _RUN.get(case["entry"], _run_backward)(case, _Inputs(case["id"], dev))
    torch.cuda.synchronize()
    return dict({"kernel": kernel, "hashes": hashes, "sums": {}}, **extra)


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
        print(f"{case['id']:<50} {r['kernel'] or '-':<28}{len(r['hashes'])} hashes {r['sums'] or ''}", flush=True)
        off = {k: v for k, v in r["sums"].items() if not v <= 1.0}
        if off:
            wrong.append(f"{case['id']}: atomic sums outside the rounding of an fp32 sum (|got - exact| / bound): {off}")
        if r.get("ticket_after", 0) != 0 or not r.get("second_call_same_bits", True):
            wrong.append(f"{case['id']}: ticket {r['ticket_after']}, second call same bits {r['second_call_same_bits']}")
        r["sums"] = sorted(r["sums"])            # (the ratios vary from run to run: the fixture keeps the names)
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
