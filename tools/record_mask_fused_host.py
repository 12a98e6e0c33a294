"""What the fused mask product host layer (csrc/mask_fused_host.h and the entry points of csrc/mask_fused.hip) answers without
touching a device: the three workspace size queries over tables of their arguments, zeros and negatives included, and for the four
launching entries (mpf_match_cost_fused, mpf_match_cost_fused_clip, mpf_pair_planes_forward, mpf_pair_planes_backward) the status
code and mpf_last_error text of every single argument fault that is rejected before any HIP call.

    python tools/record_mask_fused_host.py [--out tests/golden/mask_fused_host.json]

needs no GPU (the library loads on a CPU-only machine).  Record the fixture from the library BEFORE a change of the host layer;
tests/test_mask_fused_host_cpu.py then compares the built library with it, codes and texts exactly.

Size tables: every single and every pairwise variation of a typical call over -1, 0, 1, typical and large values of each argument,
with the sizes at which tiles_per_wg (P = 16384 | 16385 and 32768 | 32769 at one group; 3 | 4 and 7 | 8 groups at P = 4128), KS
(8 | 9, 16 | 17, 256 | 257 and 512 | 513 images at 65536 pixels; pixel counts that are 67, 96 and 3 steps of 64) and mgroups / KP
(64 | 65, 128 | 129, 256 | 257 slots) change.  The library this table was first recorded from computed its geometry in `int`, so the
tables stop short of the values on which that arithmetic overflowed (undefined behaviour, nothing to record): P > INT_MAX - 31,
Q > INT_MAX - 127, G * ceil(Q / 128) >= 2^31, F * ceil(P / 32) > INT_MAX - 511 (the round-up of tiles over at most 512 workgroups),
max_count > INT_MAX - 127 and N * ceil(max_count / 128) >= 2^31 (`_overflowed`).

The pointers handed to the entry points are made-up addresses: nothing may dereference them, so every recorded status must be one
of the library's own negative codes (a positive one is a HIP error: the call got as far as the runtime).  Left out on purpose,
because the entry accepts them and goes on to a launch: a NULL pair_of_slot (the identity), d_features and / or d_embed NULL on
mpf_pair_planes_backward (that gradient is not computed; d_embed_dtype is then not looked at), tsamp_rows = 0 on the image size
query (it is in the size table; the entry itself rejects it).  "frame stride one element short" is also a stride that is no
multiple of 8, which is answered first; "frame stride 8 short" is the overlap alone.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "mask_fused_host.json")

PTR = 0x7f0000001000          # a made-up, 256-byte aligned address
BF16 = 2
INT_MAX = 0x7fffffff

# ---- size queries: name -> (argument names, typical call, values per argument) ---------------------------------------------------------
_COST_VALUES = dict(G=(-1, 0, 1, 3, 4, 7, 8, 20, 65535, 65536), Q=(-1, 0, 1, 100, 128, 129, 1 << 24), Tmax=(-1, 0, 1, 20, 128, 129, 1 << 20),
                    P=(-1, 0, 1, 32, 33, 4128, 12544, 16384, 16385, 32768, 32769, INT_MAX - 31), tsamp_rows=(-1, 0, 1, 200, INT_MAX))
QUERIES = {
    "mpf_match_cost_fused_workspace_bytes": (("G", "Q", "Tmax", "P", "tsamp_rows"), dict(G=1, Q=100, Tmax=20, P=4128, tsamp_rows=200),
                                             _COST_VALUES),
    "mpf_match_cost_fused_clip_workspace_bytes": (("G", "Q", "Tmax", "P", "F", "tsamp_rows"), dict(G=1, Q=100, Tmax=20, P=4128, F=3, tsamp_rows=200),
                                                  dict(_COST_VALUES, F=(-1, 0, 1, 2, 3, 5, 65535, 65536, INT_MAX))),
    "mpf_pair_planes_backward_workspace_bytes": (("N", "HW", "total_slots", "max_count"), dict(N=2, HW=65536, total_slots=500, max_count=100),
                                                 dict(N=(-1, 0, 1, 2, 8, 9, 16, 17, 256, 257, 512, 513, 65535, 65536, 1 << 24),
                                                      HW=(-1, 0, 1, 128, 192, 8576, 12288, 65536, INT_MAX),
                                                      total_slots=(-1, 0, 1, 500, INT_MAX),
                                                      max_count=(-1, 0, 1, 64, 65, 128, 129, 256, 257, 1 << 24, INT_MAX - 127))),
}


def _overflowed(a):
    """the calls on which `int` geometry overflows (see the docstring): not recorded"""
    ceil = lambda x, d: (x + d - 1) // d          # noqa: E731
    if "N" in a:
        return a["max_count"] > INT_MAX - 127 or a["N"] * ceil(max(a["max_count"], 0), 128) >= 2 ** 31
    return (a["P"] > INT_MAX - 31 or a["Q"] > INT_MAX - 127 or a["G"] * ceil(max(a["Q"], 0), 128) >= 2 ** 31
            or a.get("F", 1) * ceil(a["P"], 32) > INT_MAX - 511)


def _variations(typical, values):
    """the typical call, every single and every pairwise variation of it"""
    names = list(typical)
    out = [dict(typical)]
    for i, a in enumerate(names):
        for va in values[a]:
            one = dict(typical, **{a: va})
            out.append(one)
            for b in names[i + 1:]:
                out.extend(dict(one, **{b: vb}) for vb in values[b])
    return out


def workspace_sizes(lib):
    """-> {query: {"G=.. Q=..": bytes}}"""
    out = {}
    for query, (names, typical, values) in QUERIES.items():
        fn, table = getattr(lib, query), {}
        for a in _variations(typical, values):
            # (the positive sizes of a call that has a non-positive one are never looked at: the answer is 0 before any arithmetic)
            if min(a.values()) > 0 and _overflowed(a):
                continue
            table[" ".join(f"{n}={a[n]}" for n in names)] = fn(*(a[n] for n in names))
        out[query] = table
    return out


# ---- single faults: entry -> its arguments in call order.  "?name": an optional pointer; names of GOOD: that value; "ws_bytes":
# the size query's answer; everything else is a required pointer -------------------------------------------------------------------------
_COST_TAIL = ["coords", "tsamp", "tsamp_rows", "t_first", "t_count", "cost", "G", "Q", "Tmax", "P"]
ENTRIES = {
    "mpf_match_cost_fused": ["embed", "embed_first", "embed_row_stride", "features", "feat_img_stride", "group_image", "h", "w", "channels"]
                            + _COST_TAIL + ["w_mask", "w_dice", "workspace", "ws_bytes", "stream"],
    "mpf_match_cost_fused_clip": ["embed", "embed_first", "embed_row_stride", "features", "feat_clip_stride", "feat_frame_stride", "group_clip", "h",
                                  "w", "channels"] + _COST_TAIL + ["F", "w_mask", "w_dice", "workspace", "ws_bytes", "stream"],
    "mpf_pair_planes_forward": ["embed", "row_off", "?pair_of_slot", "slot_first", "slot_count", "features", "feat_img_stride", "out", "N", "HW",
                                "channels", "stream"],
    "mpf_pair_planes_backward": ["grad_planes", "embed", "row_off", "?pair_of_slot", "slot_first", "slot_count", "features", "feat_img_stride",
                                 "?d_features", "dfeat_img_stride", "?d_embed", "d_embed_dtype", "N", "HW", "channels", "total_slots", "max_count",
                                 "workspace", "ws_bytes", "stream"],
}
# 8 x 12 planes of 256 channels (24 576 elements), three frames back to back; two images of 256 pixels with ten slots
GOOD = dict(embed_row_stride=768, feat_img_stride=24576, feat_clip_stride=3 * 24576, feat_frame_stride=24576, h=8, w=12, channels=256,
            tsamp_rows=40, G=6, Q=100, Tmax=5, P=100, F=3, w_mask=5.0, w_dice=5.0, dfeat_img_stride=65536, d_embed_dtype=BF16, N=2, HW=256,
            total_slots=10, max_count=6, stream=None)
_GOOD_OF = {"mpf_pair_planes_forward": dict(feat_img_stride=65536), "mpf_pair_planes_backward": dict(feat_img_stride=65536)}


def _ws_bytes(lib, entry, s):
    if entry == "mpf_match_cost_fused":
        return lib.mpf_match_cost_fused_workspace_bytes(s["G"], s["Q"], s["Tmax"], s["P"], s["tsamp_rows"])
    if entry == "mpf_match_cost_fused_clip":
        return lib.mpf_match_cost_fused_clip_workspace_bytes(s["G"], s["Q"], s["Tmax"], s["P"], s["F"], s["tsamp_rows"])
    return lib.mpf_pair_planes_backward_workspace_bytes(s["N"], s["HW"], s["total_slots"], s["max_count"])


def _call(lib, entry, **over):
    """one call of `entry` with GOOD values and made-up pointers, `over` replacing arguments by name -> [status, text].
    ws_bytes = -1: one byte less than the size query's answer"""
    s = dict(GOOD, **_GOOD_OF.get(entry, {}))
    s.update({k: v for k, v in over.items() if k in s})
    s["ws_bytes"] = _ws_bytes(lib, entry, s) + over.get("ws_bytes", 0)
    a = []
    for n in ENTRIES[entry]:
        key = n.lstrip("?")
        a.append(s[key] if key in s else over.get(key, PTR))
    code = getattr(lib, entry)(*a)
    return [code, lib.mpf_last_error().decode() if code else ""]


def _sizes(*keys):
    return {f"{k} = {v}": {k: v} for k in keys for v in (0, -1)}


def _unaligned(*keys):
    return {f"{k} % 8 != 0": {k: GOOD[k] + 4} for k in keys}


_COST = {"channels = 255": {"channels": 255}, "Tmax = 129": {"Tmax": 129}, "G = 65536": {"G": 65536}, "G * Q * Tmax >= 2^31": {"Q": 1 << 29},
         "workspace one byte short": {"ws_bytes": -1}}
FAULTS = {
    "mpf_match_cost_fused": {**_COST, **_sizes("G", "Q", "Tmax", "P", "h", "w", "tsamp_rows"), **_unaligned("embed_row_stride", "feat_img_stride")},
    "mpf_match_cost_fused_clip": {**_COST, **_sizes("G", "Q", "Tmax", "P", "F", "h", "w", "tsamp_rows"),
                                  **_unaligned("embed_row_stride", "feat_clip_stride", "feat_frame_stride"), "F = 65536": {"F": 65536},
                                  "F * P >= 2^31": {"F": 65535, "P": 32769}, "frame stride one element short": {"feat_frame_stride": 24575},
                                  "frame stride 8 short": {"feat_frame_stride": 24568}},
    "mpf_pair_planes_forward": {"channels = 255": {"channels": 255}, **_sizes("N", "HW"), "N = 65536": {"N": 65536}, "HW % 4 != 0": {"HW": 258},
                                "feat_img_stride % 8 != 0": {"feat_img_stride": 65540}},
    "mpf_pair_planes_backward": {"channels = 255": {"channels": 255}, **_sizes("N", "HW", "total_slots", "max_count"), "N = 65536": {"N": 65536},
                                 "HW % 128 != 0": {"HW": 192}, "feat_img_stride % 8 != 0": {"feat_img_stride": 65540},
                                 "dfeat_img_stride % 8 != 0": {"dfeat_img_stride": 65540}, "d_embed_dtype = 99": {"d_embed_dtype": 99},
                                 "workspace one byte short": {"ws_bytes": -1}},
}


def faults(lib):
    """-> {"<entry>: <fault>": [status, mpf_last_error text]}"""
    out = {}
    for entry, names in ENTRIES.items():
        for n in names:
            if n not in GOOD and n != "ws_bytes" and not n.startswith("?"):
                out[f"{entry}: NULL {n}"] = _call(lib, entry, **{n: None})
        for what, over in FAULTS[entry].items():
            out[f"{entry}: {what}"] = _call(lib, entry, **over)
    reached = {k: v for k, v in out.items() if v[0] >= 0}
    assert not reached, f"not rejected before the runtime: {reached}"
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
    print(f"library {_lib.LIB_PATH}: {sum(len(t) for t in out['workspace'].values())} sizes, {len(out['faults'])} faults -> {args.out}")


if __name__ == "__main__":
    main()
