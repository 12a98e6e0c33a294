"""What the MSDA host layer answers without touching a device: the two workspace-size queries over a list of level geometries, and
the status code and mpf_last_error text of every entry point for each single argument fault that is rejected before any HIP call.

    python tools/record_msda_host.py [--out tests/golden/msda_host.json]

needs no GPU (the library loads on a CPU-only machine).  Record the fixture from the library BEFORE a change of the host layer;
tests/test_msda_host_cpu.py then compares the built library with it, codes and texts exactly.

The pointers handed to the entry points are made-up addresses: nothing may dereference them, so every recorded status must be one of
the library's own negative codes (a positive one is a HIP error: the call got as far as the runtime).  Faults left out on purpose,
because the call goes on to a launch: a NULL ``host_spatial_shapes`` of the forward forms and NULL amax slots (both optional), and
batch / spatial_size / num_heads / num_query = 0 on the ``_dev`` pair with a workspace that is large enough.
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "msda_host.json")

F32, F64 = 0, 1
PTR = 0x7f0000001000          # a made-up, 256-byte aligned address
BASE = [(6, 4), (3, 2), (12, 9)]
GEOMETRIES = {
    "1 level 13x7": [(13, 7)],
    "2 levels": [(6, 4), (3, 2)],
    "3 levels odd": BASE,
    "4 levels": [(4, 4), (8, 8), (16, 16), (32, 32)],
    "5 levels": [(4, 4), (2, 2), (3, 3), (2, 3), (1, 2)],
    "8 levels": [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1), (3, 5), (5, 3), (7, 7)],
    "encoder B": [(32, 32), (64, 64), (128, 128)],
    "thin 1x64, 64x1": [(1, 64), (64, 1)],
    "level with H = 0": [(6, 4), (0, 2)],
    "level with W < 0": [(6, 4), (3, -2)],
}


def _hs(lv):
    return (ctypes.c_int64 * (2 * len(lv)))(*[v for hw in lv for v in hw])


def size_queries(lib):
    """-> {id: bytes} of mpf_msda_backward_workspace_bytes and mpf_msda_dev_workspace_bytes (forward and backward)"""
    out = {}
    for name, lv in GEOMETRIES.items():
        hs, L, S = _hs(lv), len(lv), sum(h * w for h, w in lv)
        for N, Mh in ((1, 2), (2, 8)):
            for Lq in (S, 300):
                for P in (4, 2, 8, 5, 10):            # 8 levels x 5 points and 4 levels x 10 points: L * P > 32
                    tag = f"{name} N={N} M={Mh} Lq={Lq} P={P}"
                    out["ws " + tag] = lib.mpf_msda_backward_workspace_bytes(N, Mh, L, Lq, P, ctypes.addressof(hs))
                    if S > 0:
                        for b in (0, 1):
                            out[f"dev{b} " + tag] = lib.mpf_msda_dev_workspace_bytes(N, S, Mh, L, Lq, P, b)
    hs, S = _hs(BASE), 138
    good = dict(N=2, M=2, L=3, Lq=138, P=4)
    for k in good:
        for v in (0, -1):
            a = dict(good, **{k: v})
            out[f"ws {k}={v}"] = lib.mpf_msda_backward_workspace_bytes(a["N"], a["M"], a["L"], a["Lq"], a["P"], ctypes.addressof(hs))
            for b in (0, 1):
                out[f"dev{b} {k}={v}"] = lib.mpf_msda_dev_workspace_bytes(a["N"], S, a["M"], a["L"], a["Lq"], a["P"], b)
    for v in (0, -1):
        for b in (0, 1):
            out[f"dev{b} S={v}"] = lib.mpf_msda_dev_workspace_bytes(2, v, 2, 3, 138, 4, b)
    out["ws NULL host shapes"] = lib.mpf_msda_backward_workspace_bytes(2, 2, 3, 138, 4, None)
    return out


# entry -> (names of the required pointers in call order, names of the optional ones, with "hs" = host shapes (real host memory),
#           tail after the 8 size / dtype words)
ENTRIES = {
    "mpf_msda_forward": (["value", "spatial_shapes", "level_start_index", "sampling_loc", "attn_weight", "output"], "plain"),
    "mpf_msda_forward_hs": (["value", "spatial_shapes", "level_start_index", "?hs", "sampling_loc", "attn_weight", "output"], "plain"),
    "mpf_msda_forward_raw": (["value", "spatial_shapes", "level_start_index", "raw", "ref_points", "loc_out", "attn_out", "output"], "raw"),
    "mpf_msda_forward_raw_hs": (["value", "spatial_shapes", "level_start_index", "?hs", "raw", "ref_points", "loc_out", "attn_out", "output"],
                                "raw"),
    "mpf_msda_forward_dev": (["value", "spatial_shapes", "level_start_index", "sampling_loc", "attn_weight", "output"], "dev"),
    "mpf_msda_backward": (["value", "spatial_shapes", "level_start_index", "sampling_loc", "attn_weight", "grad_output", "grad_value",
                           "grad_sampling_loc", "grad_attn_weight"], "plain"),
    "mpf_msda_backward_ws": (["value", "hs", "sampling_loc", "attn_weight", "grad_output", "grad_value", "grad_sampling_loc",
                              "grad_attn_weight"], "ws"),
    "mpf_msda_backward_ws_raw": (["value", "hs", "sampling_loc", "attn_weight", "grad_output", "grad_value", "grad_raw"], "ws"),
    "mpf_msda_backward_ws_raw_o": (["value", "hs", "sampling_loc", "attn_weight", "grad_output", "output", "grad_value", "grad_raw"], "ws_o"),
    "mpf_msda_backward_dev": (["value", "spatial_shapes", "level_start_index", "sampling_loc", "attn_weight", "grad_output", "grad_value",
                               "grad_sampling_loc", "grad_attn_weight"], "dev"),
}
SIZES = ("batch", "spatial_size", "num_heads", "channels", "num_levels", "num_query", "num_point")
GOOD = dict(batch=2, spatial_size=138, num_heads=2, channels=32, num_levels=3, num_query=138, num_point=4, dtype=F32)


def _call(lib, entry, hs, ptrs=None, sizes=None, ws=PTR, ws_bytes=1 << 30):
    names, kind = ENTRIES[entry]
    ptrs = ptrs or {}
    a = []
    for n in names:
        key = n.lstrip("?")
        a.append(ptrs[key] if key in ptrs else (ctypes.addressof(hs) if key == "hs" else PTR))
    s = dict(GOOD, **(sizes or {}))
    a += [s[k] for k in SIZES] + [s["dtype"]]
    if kind in ("ws", "ws_o", "dev"):
        a += [ws, ws_bytes]
    if kind == "ws_o":
        a += [None, None]
    a.append(None)                       # stream
    code = getattr(lib, entry)(*a)
    return [code, lib.mpf_last_error().decode()]


def faults(lib):
    """-> {"<entry>: <fault>": [status, mpf_last_error text]}"""
    out = {}
    hs = _hs(BASE)
    for entry, (names, kind) in ENTRIES.items():
        put = lambda what, r: out.__setitem__(f"{entry}: {what}", r)
        for n in names:
            if not n.startswith("?"):
                put(f"NULL {n}", _call(lib, entry, hs, ptrs={n: None}))
        put("dtype 99", _call(lib, entry, hs, sizes={"dtype": 99}))
        for k in SIZES:
            if kind == "dev" and k in ("batch", "spatial_size", "num_heads", "num_query"):
                continue
            put(f"{k} = 0", _call(lib, entry, hs, sizes={k: 0}))
        if kind in ("ws", "ws_o", "raw"):
            put("channels = 30", _call(lib, entry, hs, sizes={"channels": 30}))
            put("dtype MPF_F64", _call(lib, entry, hs, sizes={"dtype": F64}))
        else:
            put("num_levels = 17", _call(lib, entry, hs, sizes={"num_levels": 17}))
        if kind == "raw":
            put("L * P = 33", _call(lib, entry, hs, sizes={"num_point": 11}))
        if kind in ("ws", "ws_o"):
            put("NULL workspace", _call(lib, entry, hs, ws=None))
        if kind == "dev":
            need = lib.mpf_msda_dev_workspace_bytes(*[GOOD[k] for k in ("batch", "spatial_size", "num_heads", "num_levels", "num_query",
                                                                          "num_point")], 1 if "backward" in entry else 0)
            assert need > 1024
            put("NULL workspace", _call(lib, entry, hs, ws=None, ws_bytes=need))
            put("workspace one byte short", _call(lib, entry, hs, ws_bytes=need - 1))
            put("workspace misaligned", _call(lib, entry, hs, ws=PTR + 16, ws_bytes=need))
    reached = {k: v for k, v in out.items() if v[0] >= 0}
    assert not reached, f"not rejected before the runtime: {reached}"
    return out


def record(lib):
    return {"sizes": size_queries(lib), "faults": faults(lib)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    from mp_former_amd import _lib
    out = record(_lib.lib())
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"library {_lib.LIB_PATH}: {len(out['sizes'])} sizes, {len(out['faults'])} faults -> {args.out}")


if __name__ == "__main__":
    main()
