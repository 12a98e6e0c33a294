"""What the small-row GEMM host layer (csrc/small_gemm_host.h, the entry points of csrc/small_gemm.hip and the size queries of
csrc/decoder_layer.hip) answers without touching a device: for the five entries (mpf_small_gemm_bf16, mpf_small_gemm_bf16_blocked,
mpf_small_gemm_bf16_group, mpf_transpose_group_bf16, mpf_tall_gemm_bf16) the status code and mpf_last_error text of every single
argument fault that is rejected before any HIP call, the 0 of the empty problems, and for the blocked and the tall entry every pair
of those faults (their check order is part of the contract); the three scratch size queries over tables of their arguments.

    python tools/record_small_gemm_host.py [--out tests/golden/small_gemm_host.json]

needs no GPU (the library loads on a CPU-only machine).  Record the fixture from the library BEFORE a change of the host layer;
tests/test_small_gemm_host_cpu.py then compares the built library with it, codes, texts and sizes exactly.

The pointers handed to the entry points are made-up addresses: nothing may dereference them.  A case named as a fault must come back
negative (one of the library's own codes; a positive one is a HIP error: the call got as far as the runtime); only a case that
holds an empty problem (I = 0, J = 0, n_items = 0, M = 0, N = 0) may come back 0, and no case may launch: `record` checks both.  A
pair is two faults on different arguments.  Left out on purpose: geometry that does not fit a launch (the library these tables were
first recorded from computed it in `int` without a check, there is nothing to record).
"""
import argparse
import ctypes
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "small_gemm_host.json")
PTR = 0x7f0000001000          # a made-up, 256-byte aligned address

# ---- entry -> its arguments in call order; GOOD: an accepted call (pointers not named there are PTR; "?name": optional, absent) -------
ENTRIES = {
    "mpf_small_gemm_bf16": ["a", "a_rs", "a_ks", "?gate", "b", "b_rs", "b_ks", "bias", "c_in", "ldcin", "c", "ldc", "rowsum_a", "I", "J", "Kc",
                            "relu", "stream"],
    "mpf_small_gemm_bf16_blocked": ["a", "a_rs", "a_ks", "a_blk", "a_bs", "?gate", "b", "b_rs", "b_ks", "bias", "c_in", "ldcin", "c", "ldc",
                                    "c_blk", "c_bs", "rowsum_a", "I", "J", "Kc", "relu", "stream"],
    "mpf_tall_gemm_bf16": ["a", "lda", "b", "ldb", "bias", "c", "ldc", "M", "N", "K", "stream"],
}
GOOD = dict(a_rs=64, a_ks=1, a_blk=0, a_bs=0, b_rs=64, b_ks=1, ldcin=16, ldc=16, c_blk=0, c_bs=0, I=16, J=16, Kc=64, relu=0, stream=None,
            lda=64, ldb=64, M=16, N=16, K=64)
EMPTY = {"I": 0, "J": 0, "M": 0, "N": 0, "n_items": 0}          # argument -> the value that makes the problem empty

_PLAIN = {
    "I = -1": {"I": -1}, "J = -1": {"J": -1}, "Kc = -1": {"Kc": -1}, "I = 0": {"I": 0}, "J = 0": {"J": 0},
    "NULL a": {"a": None}, "NULL b": {"b": None}, "NULL c": {"c": None}, "Kc = 0": {"Kc": 0},
    "a: no unit stride": {"a_ks": 2}, "b: no unit stride": {"b_ks": 2},
    "Kc % 8 != 0": {"Kc": 12}, "a_rs % 8 != 0": {"a_rs": 68}, "a 8 bytes off": {"a": PTR + 8}, "gate 8 bytes off": {"gate": PTR + 8},
    "b_rs % 8 != 0": {"b_rs": 68}, "b 8 bytes off": {"b": PTR + 8},
    "J % 4 != 0": {"J": 18}, "ldc % 4 != 0": {"ldc": 18}, "c 4 bytes off": {"c": PTR + 4}, "bias 4 bytes off": {"bias": PTR + 4},
    "ldcin % 4 != 0": {"ldcin": 18}, "c_in 4 bytes off": {"c_in": PTR + 4},
}
FAULTS = {
    "mpf_small_gemm_bf16": _PLAIN,
    "mpf_small_gemm_bf16_blocked": {"a_blk = -32": {"a_blk": -32}, "c_blk = -64": {"c_blk": -64}, "a_blk = 48": {"a_blk": 48}, "c_blk = 32": {"c_blk": 32},
                                    "blocked contraction, Kc = 40": {"a_blk": 32, "Kc": 40}, "c_blk with c_in": {"c_blk": 64}, **_PLAIN},
    "mpf_tall_gemm_bf16": {"M = 0": {"M": 0}, "N = 0": {"N": 0}, "NULL a": {"a": None}, "NULL b": {"b": None}, "NULL c": {"c": None},
                           "M = -1": {"M": -1}, "N = -1": {"N": -1}, "K = 0": {"K": 0}, "K = -32": {"K": -32}, "K = 40": {"K": 40},
                           "lda % 8 != 0": {"lda": 68}, "ldb % 8 != 0": {"ldb": 68}, "ldc % 4 != 0": {"ldc": 18}, "a 8 bytes off": {"a": PTR + 8},
                           "b 8 bytes off": {"b": PTR + 8}, "c 4 bytes off": {"c": PTR + 4}, "65 536 row tiles": {"M": 65536 * 128}},
}
PAIRED = ("mpf_small_gemm_bf16_blocked", "mpf_tall_gemm_bf16")

# ---- the two grouped entries: an accepted call of two items, faults as (arguments of the call, fields of item 1) -------------------------
_ROW = dict(a=PTR, gate=None, b=PTR, c=PTR, rowsum_a=PTR, a_rs=1, a_ks=16, a_bs=0, b_rs=1, b_ks=16, ldc=16, a_blk=0, I=16, J=16, Kc=32)
_CT = dict(_ROW, a_rs=64, a_ks=1, b_rs=64, b_ks=1)
_TR = dict(src=PTR, gate=None, dst=PTR, ld=16, R=8, C=16)
GROUP_FAULTS = {
    "n_items = -1": ({"n_items": -1}, {}), "n_items = 9": ({"n_items": 9}, {}), "n_items = 0": ({"n_items": 0}, {}), "NULL items": ({"items": None}, {}),
    "a_rs = 2 on row-contiguous operands": ({}, {"a_rs": 2}), "b_rs = 2 on row-contiguous operands": ({}, {"b_rs": 2}),
    "mixed operand forms": ({}, _CT), "mixed operand forms (contiguous group)": ({"form": "ct"}, _ROW), "gate on contiguous operands": ({"form": "ct"}, {"gate": PTR}),
    "a_blk = 48": ({}, {"a_blk": 48}), "I = -1": ({}, {"I": -1}), "NULL a": ({}, {"a": None}), "NULL c": ({}, {"c": None}), "Kc = 0": ({}, {"Kc": 0}),
    "Kc % 8 != 0 (contiguous group)": ({"form": "ct"}, {"Kc": 12}), "a 8 bytes off (contiguous group)": ({"form": "ct"}, {"a": PTR + 8}),
    "J % 4 != 0": ({}, {"J": 18}), "c 4 bytes off": ({}, {"c": PTR + 4}), "Kc % 32 disagrees": ({}, {"Kc": 33}),
    "Kc % 32 disagrees (contiguous group)": ({"form": "ct"}, {"Kc": 40}), "all items empty": ({"all": {"I": 0}}, {"I": 0}),
}
TRANSPOSE_FAULTS = {
    "n_items = -1": ({"n_items": -1}, {}), "n_items = 17": ({"n_items": 17}, {}), "n_items = 0": ({"n_items": 0}, {}), "NULL items": ({"items": None}, {}),
    "Rp = 0": ({"Rp": 0}, {}), "Rp = -8": ({"Rp": -8}, {}), "Rp = 12": ({"Rp": 12}, {}), "NULL src": ({}, {"src": None}), "NULL dst": ({}, {"dst": None}),
    "R = 0": ({}, {"R": 0}), "R > Rp": ({}, {"R": 9}), "C = 0": ({}, {"C": 0}), "C % 8 != 0": ({}, {"C": 12}), "ld % 8 != 0": ({}, {"ld": 20}),
    "src 8 bytes off": ({}, {"src": PTR + 8}), "dst 8 bytes off": ({}, {"dst": PTR + 8}), "gate 8 bytes off": ({}, {"gate": PTR + 8}),
}

# ---- size queries: name -> (argument names, typical call, values per argument) ---------------------------------------------------------
_LAYER = (("Qt", "N", "H", "S", "ffn_dim", "backward"), dict(Qt=33, N=2, H=8, S=200, ffn_dim=2048, backward=1),
          dict(Qt=(-1, 0, 1, 31, 32, 33, 230), N=(-1, 0, 1, 3), H=(-1, 0, 8), S=(-1, 0, 1, 77, 1024), ffn_dim=(-1, 0, 32, 2048), backward=(0, 1)))
QUERIES = {"mpf_decoder_layer_scratch_bytes": _LAYER, "mpf_decoder_layer_pos_scratch_bytes": _LAYER,
           "mpf_next_attn_mask_scratch_bytes": (("N", "Q"), dict(N=2, Q=100), dict(N=(-1, 0, 1, 2, 65536), Q=(-1, 0, 1, 31, 32, 33, 100, 65536)))}


def _status(lib, code):
    return [code, lib.mpf_last_error().decode() if code else ""]


def _call(lib, entry, over):
    a = []
    for n in ENTRIES[entry]:
        key = n.lstrip("?")
        a.append(over[key] if key in over else GOOD[key] if key in GOOD else None if n.startswith("?") else PTR)
    return _status(lib, getattr(lib, entry)(*a))


def _items(cls, n, base, last):
    arr = (cls * max(n, 1))()
    for t, it in enumerate(arr):
        for k, v in dict(base, **(last if t == n - 1 else {})).items():
            setattr(it, k, v)
    return arr


def _call_group(lib, call, item):
    from mp_former_amd.small_linear import MpfSmallGemmItem
    n = call.get("n_items", 2)
    base = dict(_CT if call.get("form") == "ct" else _ROW, **call.get("all", {}))
    arr = _items(MpfSmallGemmItem, min(max(n, 0), 9), base, item) if "items" not in call else None
    return _status(lib, lib.mpf_small_gemm_bf16_group(arr, n, None))


def _call_transpose(lib, call, item):
    from mp_former_amd.small_linear import MpfTransposeItem
    n = call.get("n_items", 2)
    arr = _items(MpfTransposeItem, min(max(n, 0), 17), _TR, item) if "items" not in call else None
    return _status(lib, lib.mpf_transpose_group_bf16(arr, n, call.get("Rp", 8), None))


def _holds_empty(*overs):
    return any(o.get(k) == v for o in overs for k, v in EMPTY.items()) or any("all" in o for o in overs)


def faults(lib):
    """-> {"<entry>: <fault>[ + <fault>]": [status, mpf_last_error text]}"""
    out, may_be_zero = {}, set()
    for entry, table in FAULTS.items():
        cases = [((name,), over) for name, over in table.items()]
        if entry in PAIRED:
            cases += [((n1, n2), dict(o1, **o2)) for (n1, o1), (n2, o2) in itertools.combinations(table.items(), 2) if not set(o1) & set(o2)]
        for names, over in cases:
            key = f"{entry}: " + " + ".join(names)
            out[key] = _call(lib, entry, over)
            if _holds_empty(over):
                may_be_zero.add(key)
    for entry, fn, table in (("mpf_small_gemm_bf16_group", _call_group, GROUP_FAULTS), ("mpf_transpose_group_bf16", _call_transpose, TRANSPOSE_FAULTS)):
        for name, (call, item) in table.items():
            key = f"{entry}: {name}"
            out[key] = fn(lib, call, item)
            if _holds_empty(call, item):
                may_be_zero.add(key)
    reached = {k: v for k, v in out.items() if v[0] > 0 or (v[0] == 0 and k not in may_be_zero)}
    assert not reached, f"not rejected before the runtime: {reached}"
    for k in may_be_zero:
        single = " + " not in k
        assert out[k][0] == 0 or not single, f"an empty problem did not return 0: {k} {out[k]}"
    return out


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


def scratch_sizes(lib):
    """-> {query: {"Qt=.. N=..": bytes}}"""
    out = {}
    for query, (names, typical, values) in QUERIES.items():
        fn = getattr(lib, query)
        out[query] = {" ".join(f"{n}={a[n]}" for n in names): fn(*(a[n] for n in names)) for a in _variations(typical, values)}
    return out


def record(lib):
    return {"scratch": scratch_sizes(lib), "faults": faults(lib)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    from mp_former_amd import _lib
    out = record(_lib.lib())
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"library {_lib.LIB_PATH}: {sum(len(t) for t in out['scratch'].values())} sizes, {len(out['faults'])} faults -> {args.out}")


if __name__ == "__main__":
    main()
