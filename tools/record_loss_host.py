"""What the loss host layer (csrc/loss_host.h and the entry points of csrc/loss.hip) answers without touching a device:
mpf_match_cost_clip_workspace_bytes over a table of (n_rows, F, Tmax), zeros and negatives included, and for all ten entry points the
status code and mpf_last_error text of every single argument fault that is rejected before any HIP call, plus the "nothing to do"
zero returns (n = 0, k = 0, no pixels).

    python tools/record_loss_host.py [--out tests/golden/loss_host.json]

needs no GPU (the library loads on a CPU-only machine).  Record the fixture from the library BEFORE a change of the host layer;
tests/test_loss_host_cpu.py then compares the built library with it, codes and texts exactly.

The pointers handed to the entry points are made-up addresses: nothing may dereference them, so every recorded status must be zero
(nothing to do) or one of the library's own negative codes (a positive one is a HIP error: the call got as far as the runtime).
Faults left out on purpose, because the entry accepts them and goes on to a launch: a NULL coord_rows of mpf_point_sample
(optional); H = 0 or W = 0 on mpf_mask_loss_backward_dense with byte masks (never checked there); rows_per_group <= 0 or odd on
mpf_match_cost (it selects the generic kernel); n > 65535 on mpf_select_uncertain, mpf_sample_select_uncertain and the two cost
entries (their rows are grid.x); a plane that does not fit LDS on the mask-loss forward and the cost entries (generic kernel);
P_out > k on the two selections.  The one double fault recorded is dtype = grad_dtype = 99 on the dense backward: a bad map dtype
alone is answered by the gradient-dtype rule, which comes first.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "loss_host.json")

PTR = 0x7f0000001000          # a made-up, 256-byte aligned address
F32, F64, BF16, U8, BITS = 0, 1, 2, 3, 4
INT_MAX = 0x7fffffff

# entry -> its arguments in call order.  "?name": an optional pointer; names of GOOD: that value; "ws_bytes": the size query's
# answer; everything else is a required pointer.
_MAP = ["pred", "dtype", "h", "w", "pred_rows"]
_GT = ["gt", "gt_dtype", "H", "W", "gt_rows"]
_COST = ["coords", "coord_rows", "tsamp", "t_first", "t_count", "cost", "n_rows", "Tmax", "P", "w_mask", "w_dice", "rows_per_group"]
ENTRIES = {
    "mpf_point_sample": ["src", "dtype", "h", "w", "rows", "coords", "?coord_rows", "out", "n", "P", "stream"],
    "mpf_pack_mask_bits": ["masks", "bits", "n_pixels", "stream"],
    "mpf_mask_loss_forward": _MAP + _GT + ["coords", "partial", "n", "P", "chunks", "stream"],
    "mpf_mask_loss_backward": _MAP + ["gt", "H", "W", "gt_rows", "coords", "grad_sums", "grad_pred", "grad_offs", "n", "P", "stream"],
    "mpf_mask_loss_backward_dense": _MAP + _GT + ["coords", "grad_sums", "grad", "grad_dtype", "grad_offs", "n", "P", "stream"],
    "mpf_select_uncertain": ["vals", "coords_in", "coords_out", "n", "M", "k", "P_out", "stream"],
    "mpf_match_cost": _MAP + _COST + ["stream"],
    "mpf_match_cost_clip": _MAP + ["F", "stride_f"] + _COST + ["workspace", "ws_bytes", "stream"],
    "mpf_sample_select_uncertain": _MAP + ["coords_in", "coords_out", "n", "M", "k", "P_out", "stream"],
}
# 16 x 24 maps (768-byte bf16 planes), 8 x 20 masks (160 pixels = 5 words), three frames 384 elements apart
GOOD = dict(dtype=BF16, h=16, w=24, gt_dtype=U8, H=8, W=20, grad_dtype=BF16, n=4, P=100, chunks=8, M=700, k=100, P_out=103, n_pixels=64,
            n_rows=12, Tmax=5, w_mask=5.0, w_dice=5.0, rows_per_group=6, F=3, stride_f=384, stream=None)
WS_TABLE = [(n, F, T) for n in (-1, 0, 1, 12, 600) for F in (-1, 0, 1, 3, 65535) for T in (-1, 0, 1, 5, 100)]


def workspace_sizes(lib):
    """-> {"n_rows=.. F=.. Tmax=..": bytes} of mpf_match_cost_clip_workspace_bytes"""
    return {f"n_rows={n} F={F} Tmax={T}": lib.mpf_match_cost_clip_workspace_bytes(n, F, T) for n, F, T in WS_TABLE}


def _call(lib, entry, **over):
    """one call of `entry` with GOOD values and made-up pointers, `over` replacing arguments by name -> [status, text]"""
    s = {k: over.get(k, v) for k, v in GOOD.items()}
    s["ws_bytes"] = over.get("ws_bytes", lib.mpf_match_cost_clip_workspace_bytes(s["n_rows"], s["F"], s["Tmax"]))
    a = []
    for n in ENTRIES[entry]:
        key = n.lstrip("?")
        a.append(s[key] if key in s else over.get(key, None if n.startswith("?") else PTR))
    code = getattr(lib, entry)(*a)
    return [code, lib.mpf_last_error().decode() if code else ""]


# entry -> {fault: the arguments it replaces}, beyond the NULLs (one per required pointer) that faults() adds
def _size_faults(*keys):
    return {f"{k} = {v}": {k: v} for k in keys for v in (0, -1) if not (k in ("n", "n_rows", "k") and v == 0)}


_DT = {f"dtype = {v}": {"dtype": v} for v in (F64, U8, BITS, 99)}
_GT_DT = {"gt_dtype = MPF_BF16": {"gt_dtype": BF16}, "gt_dtype = 99": {"gt_dtype": 99}, "bits of 5 x 7 masks": {"gt_dtype": BITS, "H": 5, "W": 7}}
_ROWS = {"65536 rows": {"n": 65536}, "nothing to do: n = 0": {"n": 0}}
_SELECT = {"k = M + 1": {"k": 701, "P_out": 800}, "P_out = k - 1": {"P_out": 99}, "nothing to do: k = 0": {"k": 0}, "nothing to do: n = 0": {"n": 0}}
_POINTS = {"P = 38401": {"P": 38401}, "nothing to do: n_rows = 0": {"n_rows": 0}}
FAULTS = {
    "mpf_point_sample": {"dtype = 1": {"dtype": F64}, "dtype = 99": {"dtype": 99}, **_size_faults("n", "P", "h", "w"), **_ROWS},
    "mpf_pack_mask_bits": {"n_pixels = 35": {"n_pixels": 35}, "n_pixels = -32": {"n_pixels": -32}, "nothing to do: n_pixels = 0": {"n_pixels": 0}},
    "mpf_mask_loss_forward": {**_DT, **_GT_DT, **_size_faults("n", "P", "h", "w", "H", "W", "chunks"), **_ROWS},
    "mpf_mask_loss_backward": {**_DT, **_size_faults("n", "P", "h", "w", "H", "W"), **_ROWS},
    "mpf_mask_loss_backward_dense": {**_DT, **_GT_DT, "grad_dtype = MPF_F32": {"grad_dtype": F32}, "dtype = grad_dtype = 99": {"dtype": 99, "grad_dtype": 99},
                                     "dtype = grad_dtype = MPF_U8": {"dtype": U8, "grad_dtype": U8}, **_size_faults("n", "P", "h", "w"),
                                     "w = 16385": {"w": 16385}, **_ROWS},
    "mpf_select_uncertain": {**_size_faults("n", "M", "k"), **_SELECT},
    "mpf_match_cost": {**_DT, **_size_faults("n_rows", "Tmax", "P", "h", "w"), **_POINTS},
    "mpf_match_cost_clip": {**_DT, **_size_faults("n_rows", "Tmax", "P", "h", "w", "F", "rows_per_group"), **_POINTS, "F = 65536": {"F": 65536},
                            "stride_f = h * w - 1": {"stride_f": 383}, "cost matrix too large": {"n_rows": INT_MAX, "Tmax": INT_MAX, "ws_bytes": 0},
                            "workspace one byte short": {"ws_bytes": 12 * 3 * 17 * 4 - 1}, "nothing to do: n_rows = 0, NULL workspace": {"n_rows": 0, "workspace": None}},
    "mpf_sample_select_uncertain": {"dtype = 0": {"dtype": F32}, "dtype = 99": {"dtype": 99}, **_size_faults("n", "M", "k", "h", "w"), **_SELECT,
                                    "M = 40961": {"M": 40961}, "132 KiB plane": {"h": 264, "w": 256}, "70-byte plane": {"h": 5, "w": 7}},
}


def faults(lib):
    """-> {"<entry>: <fault>": [status, mpf_last_error text ("" with status 0)]}"""
    out = {}
    assert lib.mpf_match_cost_clip_workspace_bytes(12, 3, 5) == 12 * 3 * 17 * 4
    for entry, names in ENTRIES.items():
        for n in names:
            if n not in GOOD and n != "ws_bytes" and not n.startswith("?"):
                out[f"{entry}: NULL {n}"] = _call(lib, entry, **{n: None})
        for what, over in FAULTS[entry].items():
            out[f"{entry}: {what}"] = _call(lib, entry, **over)
    reached = {k: v for k, v in out.items() if v[0] > 0}
    assert not reached, f"not rejected before the runtime: {reached}"
    zero = {k for k, v in out.items() if v[0] == 0}
    assert zero == {k for k in out if "nothing to do" in k}, zero
    return out


def record(lib):
    return {"workspace": workspace_sizes(lib), "faults": faults(lib)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    from mp_former_amd import _lib
    out = record(_lib.lib())
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"library {_lib.LIB_PATH}: {len(out['workspace'])} sizes, {len(out['faults'])} faults -> {args.out}")


if __name__ == "__main__":
    main()
