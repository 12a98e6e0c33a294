"""What the attention host layer (csrc/attn.hip behind csrc/attn_host.h) answers without touching a device: the two size queries
over a table of shapes under three settings of the split options, the return code of every attention option value, and the status
code and mpf_last_error text of all ten entry points for each single argument fault that is rejected before any HIP call.

    python tools/record_attn_host.py [--out tests/golden/attn_host.json]

needs no GPU (the library loads on a CPU-only machine).  Record the fixture from the library BEFORE a change of the host layer;
tests/test_attn_host_cpu.py then compares the built library with it, codes and texts exactly.

The pointers handed to the entry points are made-up addresses: nothing may dereference them, so every recorded status must be one of
the library's own negative codes (a positive one is a HIP error: the call got as far as the runtime).  Faults left out on purpose,
because the entry accepts them and goes on to a launch: a NULL mask, lse of the forward and aux of the backward (all optional);
V^T, K^T or the forward's workspace at + 8 bytes (they select the unaligned form / are not checked); strides of 12 on
mpf_attn_transpose2_strided (only the sign is checked); LqP = Lq and LqP = round32(Lq) + 32 on mpf_attn_bwd_prep (any LqP >= Lq
is accepted there).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "attn_host.json")

PTR = 0x7f0000001000          # a made-up, 256-byte aligned address
HD = 32
OPTION_DEFAULTS = {"attn_occ": 4, "attn_nw": 8, "attn_kpw": 0}
OPTION_SETTINGS = {"policy": {}, "kpw 64 nw 1": {"attn_kpw": 64, "attn_nw": 1}, "kpw 512 nw 3": {"attn_kpw": 512, "attn_nw": 3}}
OPTION_VALUES = {"attn_occ": (2, 3, 4), "attn_nw": (0, 1, 8, 9), "attn_kpw": (0, 63, 64, 100, 512)}
LQS, LKS, NHS = (1, 32, 33, 100, 120, 300), (1, 8, 256, 257, 1024, 1025, 4096, 16384), ((1, 2), (2, 8), (8, 8))
# (Lq, Lk, N, H) -> workgroup splits of the library's own policy: every arm of attn_split
POLICY_SPLITS = {(100, 1024, 2, 8): 1, (100, 1025, 2, 8): 2, (120, 16384, 2, 8): 8, (300, 16384, 8, 8): 4}


def round32(x):
    return (x + 31) // 32 * 32


def _set(lib, options):
    for k, v in dict(OPTION_DEFAULTS, **options).items():
        assert lib.mpf_set_option(k.encode(), v) == 0, (k, v)


def wg_splits(lib, Lq, Lk, N, H):
    """workgroup splits from the library's own sizes (as wg_splits_of_library of tests/test_attn_keys_gpu.py)"""
    part = lib.mpf_attn_workspace_bytes(Lq, Lk, N, H) - lib.mpf_attn_bwd_aux_bytes(Lq, Lk, N, H, N)
    return part // (N * H * Lq * (HD + 2) * 4)


def size_queries(lib):
    """-> {id: bytes} of mpf_attn_workspace_bytes and mpf_attn_bwd_aux_bytes under the three option settings"""
    out = {}
    try:
        for setting, options in OPTION_SETTINGS.items():
            _set(lib, options)
            for Lq in LQS:
                for Lk in LKS:
                    for N, H in NHS:
                        tag = f"{setting}: Lq={Lq} Lk={Lk} N={N} H={H}"
                        out["ws " + tag] = lib.mpf_attn_workspace_bytes(Lq, Lk, N, H)
                        for mi in sorted({0, 1, N}):
                            out[f"aux {tag} mask_images={mi}"] = lib.mpf_attn_bwd_aux_bytes(Lq, Lk, N, H, mi)
            good = dict(Lq=33, Lk=72, N=2, H=2, mask_images=2)
            for k in good:
                for v in (0, -1):
                    a = dict(good, **{k: v})
                    out[f"aux {setting}: {k}={v}"] = lib.mpf_attn_bwd_aux_bytes(a["Lq"], a["Lk"], a["N"], a["H"], a["mask_images"])
                    if k != "mask_images":
                        out[f"ws {setting}: {k}={v}"] = lib.mpf_attn_workspace_bytes(a["Lq"], a["Lk"], a["N"], a["H"])
        _set(lib, {})
        for shape, splits in POLICY_SPLITS.items():
            assert wg_splits(lib, *shape) == splits, (shape, wg_splits(lib, *shape))
    finally:
        _set(lib, {})
    return out


def options(lib):
    """-> {"key=value": return code of mpf_set_option}"""
    try:
        return {f"{k}={v}": lib.mpf_set_option(k.encode(), v) for k, vals in OPTION_VALUES.items() for v in vals}
    finally:
        _set(lib, {})


# entry -> its arguments in call order.  "?name": an optional pointer; names of GOOD: that size word; "ws_bytes" / "aux_bytes": the
# size query's answer; everything else is a required pointer.
_BWD_HEAD = ["q", "k", "v"]
_BWD_MID = ["kT", "qT", "dout", "doutT", "?mask", "mask_per_image", "lse", "delta", "dq", "dk", "dv"]
_BWD_TAIL = ["Lq", "LqP", "Lk", "N", "H", "head_dim", "scale", "workspace", "ws_bytes"]
ENTRIES = {
    "mpf_attn_forward": ["q", "k", "vt", "?mask", "mask_per_image", "out", "?lse", "Lq", "Lk", "N", "H", "head_dim", "scale", "workspace",
                         "ws_bytes", "stream"],
    "mpf_attn_forward_kv": ["q", "k", "k_row_stride", "k_img_stride", "vt", "?mask", "mask_per_image", "out", "?lse", "Lq", "Lk", "N", "H",
                            "head_dim", "scale", "workspace", "ws_bytes", "stream"],
    "mpf_attn_backward": _BWD_HEAD + _BWD_MID + _BWD_TAIL + ["stream"],
    "mpf_attn_backward_kv": _BWD_HEAD + ["kv_row_stride", "kv_img_stride"] + _BWD_MID + ["dkv_row_stride", "dkv_img_stride"] + _BWD_TAIL
                            + ["stream"],
    "mpf_attn_backward_kv_aux": _BWD_HEAD + ["kv_row_stride", "kv_img_stride"] + _BWD_MID + ["dkv_row_stride", "dkv_img_stride"] + _BWD_TAIL
                                + ["?aux", "stream"],
    "mpf_attn_transpose2": ["a", "b", "aT", "bT", "L", "LP", "N", "E", "stream"],
    "mpf_attn_transpose2_strided": ["a", "b", "in_row_stride", "in_img_stride", "aT", "bT", "L", "LP", "N", "E", "stream"],
    "mpf_attn_bwd_prep": ["q", "dout", "out", "qT", "doT", "delta", "Lq", "LqP", "N", "H", "stream"],
    "mpf_attn_bwd_prep_aux": ["q", "dout", "out", "lse", "?mask", "mask_per_image", "Lk", "qT", "doT", "delta", "aux", "aux_bytes", "Lq", "LqP",
                              "N", "H", "stream"],
    "mpf_attn_delta": ["dout", "out", "delta", "Lq", "N", "H", "stream"],
}
# Lq = 33: two query tiles, LqP = 64; a per-image mask, so that the workspace the backward asks for is the size query's answer
GOOD = dict(Lq=33, LqP=64, Lk=72, N=2, H=2, head_dim=HD, scale=0.17, mask_per_image=1, L=33, LP=64, E=64, stream=None,
            k_row_stride=0, k_img_stride=0, kv_row_stride=0, kv_img_stride=0, dkv_row_stride=0, dkv_img_stride=0, in_row_stride=0,
            in_img_stride=0)


def _call(lib, entry, **over):
    """one call of `entry` with GOOD values and made-up pointers, `over` replacing arguments by name -> [status, text]"""
    s = {k: over.get(k, v) for k, v in GOOD.items()}
    s["ws_bytes"] = over.get("ws_bytes", lib.mpf_attn_workspace_bytes(GOOD["Lq"], GOOD["Lk"], GOOD["N"], GOOD["H"]))
    s["aux_bytes"] = over.get("aux_bytes", lib.mpf_attn_bwd_aux_bytes(GOOD["Lq"], GOOD["Lk"], GOOD["N"], GOOD["H"], GOOD["N"]))
    a = []
    for n in ENTRIES[entry]:
        key = n.lstrip("?")
        a.append(s[key] if key in s else over.get(key, None if n == "?aux" else PTR))
    code = getattr(lib, entry)(*a)
    return [code, lib.mpf_last_error().decode()]


def faults(lib):
    """-> {"<entry>: <fault>": [status, mpf_last_error text]}"""
    out = {}
    need = lib.mpf_attn_workspace_bytes(GOOD["Lq"], GOOD["Lk"], GOOD["N"], GOOD["H"])
    aux_need = lib.mpf_attn_bwd_aux_bytes(GOOD["Lq"], GOOD["Lk"], GOOD["N"], GOOD["H"], GOOD["N"])
    assert need > aux_need > 1024
    for entry, names in ENTRIES.items():
        put = lambda what, r: out.__setitem__(f"{entry}: {what}", r)
        fwd, bwd, prep_aux = "forward" in entry, "backward" in entry, entry == "mpf_attn_bwd_prep_aux"
        for n in names:
            if n not in GOOD and n not in ("ws_bytes", "aux_bytes") and not n.startswith("?"):
                put(f"NULL {n}", _call(lib, entry, **{n: None}))
        if "head_dim" in names:
            put("head_dim = 16", _call(lib, entry, head_dim=16))
        for k in ("Lq", "Lk", "N", "H", "L", "E"):
            if k in names:
                put(f"{k} = 0", _call(lib, entry, **{k: 0}))
        if "LqP" in names:
            put("LqP = Lq - 1", _call(lib, entry, LqP=GOOD["Lq"] - 1))
            if entry != "mpf_attn_bwd_prep":
                put("LqP = Lq", _call(lib, entry, LqP=GOOD["Lq"]))
                put("LqP = round32(Lq) + 32", _call(lib, entry, LqP=round32(GOOD["Lq"]) + 32))
        if "LP" in names:
            put("LP = L - 1", _call(lib, entry, LP=GOOD["L"] - 1))
        for n in names:
            if n.endswith("_stride"):
                put(f"{n} = -8", _call(lib, entry, **{n: -8}))
                if entry != "mpf_attn_transpose2_strided":
                    put(f"{n} = 12", _call(lib, entry, **{n: 12}))
        for n in (("k",) if fwd else ("k", "v", "dk", "dv") if bwd else ()):
            put(f"{n} at + 8 bytes", _call(lib, entry, **{n: PTR + 8}))
        if fwd or bwd:
            put("workspace one byte short", _call(lib, entry, ws_bytes=need - 1))
        if bwd:
            put("workspace at + 8 bytes", _call(lib, entry, workspace=PTR + 8))
        if entry == "mpf_attn_backward_kv_aux":
            put("with aux: workspace one byte short of the partials", _call(lib, entry, aux=PTR, ws_bytes=need - aux_need - 1))
            put("aux at + 8 bytes", _call(lib, entry, aux=PTR + 8))
        if prep_aux:
            put("aux one byte short", _call(lib, entry, aux_bytes=aux_need - 1))
            put("aux at + 8 bytes", _call(lib, entry, aux=PTR + 8))
    reached = {k: v for k, v in out.items() if v[0] >= 0}
    assert not reached, f"not rejected before the runtime: {reached}"
    return out


def record(lib):
    return {"sizes": size_queries(lib), "options": options(lib), "faults": faults(lib)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    from mp_former_amd import _lib
    out = record(_lib.lib())
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"library {_lib.LIB_PATH}: {len(out['sizes'])} sizes, {len(out['options'])} options, {len(out['faults'])} faults -> {args.out}")


if __name__ == "__main__":
    main()
