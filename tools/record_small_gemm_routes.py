"""Route table of the small-row GEMM host layer (the entry points of csrc/small_gemm.hip on the records of csrc/small_gemm_host.h,
and the decoder layer of csrc/decoder_layer.hip that sequences them): which kernel every entry names on the smallest problems that
reach each host decision, what the profiler logs and what the kernels write.

    python tools/record_small_gemm_routes.py [--out tests/golden/small_gemm_routes.json]

runs CASES on cuda:0 and writes the fixture that tests/test_small_gemm_routes_recorded_gpu.py compares the library against.  Record
it from the library BEFORE a change of the host layer; the test then pins the change.  Operands and poison are those of
tests/test_small_gemm_forms_gpu.py (NaN around everything addressed, results start as the sentinel 3.0), the layer problems those of
tests/test_decoder_layer_direct_gpu.py and tests/_decoder_layer_pos_common.py.  The cases:

  gemm      mpf_small_gemm_bf16: the six (I, J) that pin the tile-width rule at Kc = 32; the four operand forms x gate x Kc = 32 | 40
            (33 where no operand is contraction-contiguous)
  blocked   one blocked-contraction, one row-blocked and one column-blocked problem of the forms test
  group     row-contiguous operands: 1 and 8 problems, an empty one in the middle, Kc = 33 (masked) and 64; contraction-contiguous
            operands on the transposed copies of the 8 problems (16 matrices in one transpose launch, gated, R < Rp) at Rp = 64 and
            the masked Rp = 40, and of one problem (2 matrices)
  transpose mpf_transpose_group_bf16 with n_items = 1: one gated 33 x 40 matrix, rows 48 apart, into Rp = 64 (the 15 unused slots)
  tall      M = 1023 | 1024 x K = 64 | 256 | 768 x bias at N = 128, N = 130, tall_ws = 0, tall_ws_wgs = 3, every call made twice
            (the first and a later launch of one instantiation), and K = 256 after K = 768
  layer     the two smallest layer problems x decoder_dw_group 0 | 1 | 2 x packed | unpacked x with | without positions, forward and
            backward; the forward also with decoder_row_chain = 0

Per case the fixture holds
    kernels   mpf_last_kernel after each call
    prof      the launch profiler's records: name -> [launches, logged algorithmic bytes, logged flops] ("": all launches)
    hashes    SHA-256 of every output buffer in full, canary regions and rowsums included, and for the layer of the scratch
              workspace (0xFF before the call; the queried bytes are hashed, a 256-byte canary behind them must stay) after the
              forward and after the backward
The recorder runs every case twice: a buffer whose bits differ between the two runs is left out of the hashes and listed under
"unstable" (none so far: every kernel the cases reach is fixed-order without atomics).
"""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FIXTURE = os.path.join(ROOT, "tests", "golden", "small_gemm_routes.json")
BF16 = torch.bfloat16
PROF_NAMES = ("small_gemm_kernel", "small_gemm_group_kernel", "tall_gemm_bf16_kernel", "")
TILE_WIDTH = ((228, 256, 1), (1008, 256, 2), (1024, 256, 4), (2048, 64, 2), (4096, 4, 4), (16, 4, 1))       # (I, J, nj)
LAYER_CASES = ((1, 1, 8, 32, False, None), (7, 3, 77, 96, False, None))


def _cases():
    c = {}
    for I, J, nj in TILE_WIDTH:
        c[f"gemm {I}x{J} nj{nj}"] = dict(kind="gemm", I=I, J=J, Kc=32, ac=True, bc=True, bias=True, rowsum=True)
    for ac, bc in ((True, True), (True, False), (False, False), (False, True)):
        for gate in (False, True):
            for Kc in (32, 40 if ac or bc else 33):
                c[f"gemm a{'c' if ac else 'r'}b{'c' if bc else 'r'}{' gate' if gate else ''} Kc={Kc}"] = dict(
                    kind="gemm", I=17, J=40, Kc=Kc, ac=ac, bc=bc, gate=gate, rowsum=gate)
    c["blocked contraction"] = dict(kind="gemm", I=17, J=40, Kc=96, ac=True, bc=False, a_blk=32)
    c["blocked rows"] = dict(kind="gemm", I=96, J=40, Kc=33, ac=False, bc=False, a_blk=32, gate=True, rowsum=True)
    c["blocked columns"] = dict(kind="gemm", I=17, J=192, Kc=96, ac=True, bc=True, c_blk=64)
    c["group rows 1 item Kc=33"] = dict(kind="group", R=33, which=(2,))
    c["group rows 8 items Kc=33"] = dict(kind="group", R=33, which=tuple(range(8)))
    c["group rows 8 items Kc=64"] = dict(kind="group", R=64, which=tuple(range(8)))
    c["group rows empty item in the middle"] = dict(kind="group", R=33, which=tuple(range(8)), hole=4)
    c["group copies 8 items Rp=64"] = dict(kind="group", R=33, which=tuple(range(8)), Rp=64)
    c["group copies 8 items Rp=40"] = dict(kind="group", R=33, which=tuple(range(8)), Rp=40)
    c["group copies 1 item Rp=64"] = dict(kind="group", R=33, which=(1,), Rp=64)
    c["transpose 1 matrix gated R=33 Rp=64"] = dict(kind="transpose", R=33, C=40, ld=48, Rp=64)
    for M in (1023, 1024):
        for K in (64, 256, 768):
            for bias in (False, True):
                c[f"tall M={M} K={K}{' bias' if bias else ''}"] = dict(kind="tall", calls=((M, 128, K, bias),) * 2)
    c["tall N=130"] = dict(kind="tall", calls=((1024, 130, 256, True),) * 2)
    c["tall tall_ws=0"] = dict(kind="tall", calls=((1024, 128, 256, True),) * 2, options={"tall_ws": 0})
    c["tall tall_ws_wgs=3"] = dict(kind="tall", calls=((1024, 128, 256, True),) * 2, options={"tall_ws_wgs": 3})
    c["tall K=256 after K=768"] = dict(kind="tall", calls=((1024, 128, 768, False), (1024, 128, 256, False)))
    for i, case in enumerate(LAYER_CASES):
        for pos in (False, True):
            for packed in (True, False):
                name = f"layer {i}{' pos' if pos else ''} {'packed' if packed else 'unpacked'}"
                for v in (0, 1, 2):
                    c[f"{name} dw_group={v}"] = dict(kind="layer", case=case, pos=pos, packed=packed, options={"decoder_dw_group": v})
                c[f"{name} row_chain=0 forward"] = dict(kind="layer", case=case, pos=pos, packed=packed, forward_only=True,
                                                        options={"decoder_row_chain": 0})
    return c


CASES = _cases()
DEFAULTS = {"tall_ws": 1, "tall_ws_wgs": 0, "decoder_dw_group": 2, "decoder_row_chain": 1}


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _run_gemm(case, dev, L, call):
    import test_small_gemm_forms_gpu as T
    I, J, Kc, ac, bc = (case[k] for k in ("I", "J", "Kc", "ac", "bc"))
    a_blk, c_blk = case.get("a_blk", 0), case.get("c_blk", 0)
    g = torch.Generator().manual_seed(7000 + 31 * I + 7 * J + Kc + 2 * ac + bc)
    A, B = torch.randn(I, Kc, generator=g).bfloat16(), torch.randn(J, Kc, generator=g).bfloat16()
    a_off, a_rs, a_ks, a_bs, a_size = T._addr(I, Kc, ac, a_blk)
    b_off, b_rs, b_ks, _, b_size = T._addr(J, Kc, bc)
    a_buf, b_buf = T._filled(a_size, a_off, A, float("nan")), T._filled(b_size, b_off, B, float("nan"))
    g_buf = T._filled(a_size, a_off, T._plant_gate(torch.randn(I, Kc, generator=g).bfloat16()), float("nan")) if case.get("gate") else None
    bias = T._filled(J + 8, torch.arange(J), torch.randn(J, generator=g).bfloat16(), float("nan")) if case.get("bias") else None
    ldc = (c_blk or J) + 12
    c_bs = I * ldc + 24 if c_blk else 0
    c_size = (I - 1) * ldc + ((J - 1) // c_blk * c_bs + (J - 1) % c_blk if c_blk else J - 1) + 1 + 64
    c_buf = T._filled(c_size, None, None, T.SENT)
    rs_buf = T._filled(I + 16, None, None, T.SENT) if case.get("rowsum") else None
    p = L.ptr
    if a_blk or c_blk:
        call("mpf_small_gemm_bf16_blocked", a_buf.data_ptr(), a_rs, a_ks, a_blk, a_bs, p(g_buf), b_buf.data_ptr(), b_rs, b_ks, p(bias), None, 0,
             c_buf.data_ptr(), ldc, c_blk, c_bs, p(rs_buf), I, J, Kc, 0)
    else:
        call("mpf_small_gemm_bf16", a_buf.data_ptr(), a_rs, a_ks, p(g_buf), b_buf.data_ptr(), b_rs, b_ks, p(bias), None, 0, c_buf.data_ptr(), ldc,
             p(rs_buf), I, J, Kc, 0)
    return {"c": c_buf, **({"rowsum_a": rs_buf} if rs_buf is not None else {})}


def _run_group(case, dev, L, call):
    import test_small_gemm_forms_gpu as T
    from mp_former_amd.small_linear import MpfSmallGemmItem, MpfTransposeItem
    R, which, Rp = case["R"], case["which"], case.get("Rp")
    P = T._GroupProblem(R, 5000 + R)
    outs = P.outputs(which)
    n = len(which)
    items = (MpfSmallGemmItem * n)()
    bufs = {}
    if Rp is None:
        for it, t in zip(items, which):
            P.item(it, t, outs[t])
        if "hole" in case:
            items[case["hole"]].J = 0
    else:
        tr = (MpfTransposeItem * (2 * n))()
        for s, t in enumerate(which):
            I, J, gated = T.GROUP[t]
            (dy, ld_a), (x, ld_b), gate = P.ops[t]
            dyT, xT = T._filled(I * Rp + 64, None, None, T.SENT), T._filled(J * Rp + 64, None, None, T.SENT)
            a, b, it, (dw, db) = tr[2 * s], tr[2 * s + 1], items[s], outs[t]
            a.src, a.gate, a.dst, a.ld, a.R, a.C = dy.data_ptr(), (gate[0].data_ptr() if gate else None), dyT.data_ptr(), ld_a, R, I
            b.src, b.gate, b.dst, b.ld, b.R, b.C = x.data_ptr(), None, xT.data_ptr(), ld_b, R, J
            it.a, it.gate, it.b, it.c, it.rowsum_a = dyT.data_ptr(), None, xT.data_ptr(), dw.data_ptr(), db.data_ptr()
            it.a_rs, it.a_ks, it.a_bs, it.b_rs, it.b_ks, it.ldc = Rp, 1, 0, Rp, 1, J + 12
            it.a_blk, it.I, it.J, it.Kc = 0, I, J, Rp
            bufs[f"{t}.dyT"], bufs[f"{t}.xT"] = dyT, xT
        call("mpf_transpose_group_bf16", tr, 2 * n, Rp)
    call("mpf_small_gemm_bf16_group", items, n)
    for t, (dw, db) in outs.items():
        bufs[f"{t}.dw"], bufs[f"{t}.db"] = dw, db
    bufs["keep"] = P            # (the operands live as long as the launches)
    return bufs


def _run_transpose(case, dev, L, call):
    import test_small_gemm_forms_gpu as T
    from mp_former_amd.small_linear import MpfTransposeItem
    R, C, ld, Rp = (case[k] for k in ("R", "C", "ld", "Rp"))
    g = torch.Generator().manual_seed(9000 + R + C)
    off = torch.arange(R).view(-1, 1) * ld + torch.arange(C).view(1, -1)
    src = T._filled(R * ld + 64, off, torch.randn(R, C, generator=g).bfloat16(), float("nan"))
    gate = T._filled(R * ld + 64, off, T._plant_gate(torch.randn(R, C, generator=g).bfloat16()), float("nan"))
    dst = T._filled(C * Rp + 64, None, None, T.SENT)
    items = (MpfTransposeItem * 1)()
    items[0].src, items[0].gate, items[0].dst, items[0].ld, items[0].R, items[0].C = src.data_ptr(), gate.data_ptr(), dst.data_ptr(), ld, R, C
    call("mpf_transpose_group_bf16", items, 1, Rp)
    return {"dst": dst, "keep": (src, gate)}


def _run_tall(case, dev, L, call):
    bufs = {}
    for i, (M, N, K, bias) in enumerate(case["calls"]):
        g = torch.Generator().manual_seed(8000 + M + 3 * N + K)
        A, B = torch.randn(M, K, generator=g).bfloat16().to(dev), (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16().to(dev)
        bv = torch.randn(N + 8, generator=g).bfloat16().to(dev) if bias else None
        ldc = N + 4 - N % 4 if N % 4 else N + 4
        C = torch.full((M * ldc + 64,), 3.0, dtype=BF16, device=dev)
        call("mpf_tall_gemm_bf16", A.data_ptr(), K, B.data_ptr(), K, L.ptr(bv), C.data_ptr(), ldc, M, N, K)
        bufs[f"{i}.c"], bufs[f"{i}.keep"] = C, (A, B, bv)
    return bufs


def _run_layer(case, dev, L, call):
    import _decoder_layer_pos_common as PC
    import test_decoder_layer_direct_gpu as D
    from mp_former_amd import decoder_layer as DL
    assert LAYER_CASES == tuple(D.CASES[:2]) == tuple(PC.CASES[:2])            # the two smallest cases of the direct tests
    Qt, N, S, F_, _, _ = case["case"]
    pos, packed = case["pos"], case["packed"]
    query =L.lib().mpf_decoder_layer_pos_scratch_bytes if pos else L.lib().mpf_decoder_layer_scratch_bytes
    fwd_bytes, bwd_bytes = query(Qt, N, D.H, S, F_, 0), query(Qt, N, D.H, S, F_, 1)
    key = ("decoder_scratch", dev, L.stream_ptr(dev))
    saved = L._scratch.get(key)
    # the layer's scratch: exactly the queried size, 0xFF, behind it a canary that must stay
    assert DL._scratch_bytes(L.lib(), Qt, N, D.H, S, F_, pos)[0] == max(fwd_bytes, bwd_bytes)
    sc = torch.full((max(fwd_bytes, bwd_bytes) + 256,), 0xFF, dtype=torch.uint8, device=dev)
    L._scratch[key] = sc
    try:
        P = PC.problem(case["case"]) if pos else D._problem(case["case"])
        T = (PC.forward_native if pos else D._forward_native)(P, dev, packed)
        torch.cuda.synchronize(dev)
        call(None)
        x3, xb3, x3h = T["outs"]
        bufs = {"x3": x3.detach().clone(), "xb3": xb3.detach().clone(), "forward.scratch": sc[:fwd_bytes].clone()}
        if not case.get("forward_only"):
            torch.autograd.backward([x3, xb3, x3h], [P[s].to(dev) for s in D.SEEDS])
            torch.cuda.synchronize(dev)
            call(None)
            bufs["backward.scratch"] = sc[:bwd_bytes].clone()
            for name in ("x0", "xb0", "qpos", "Kp", "Vp"):
                if name in T and T[name].grad is not None:
                    bufs["d_" + name] = T[name].grad
            for name, t in zip(D.NAMES, T["params"]):
                bufs["d_" + name] = t.grad
        assert L._scratch[key] is sc and bool((sc[-256:] == 0xFF).all())
        return bufs
    finally:
        if saved is None:
            del L._scratch[key]
        else:
            L._scratch[key] = saved


def _run_once(case, dev):
    """-> kernels, prof, {buffer name: device tensor}"""
    from mp_former_amd import _lib as L
    st = L.stream_ptr(dev)
    kernels = []

    def call(name, *args):
        if name is not None:
            L.call(name, dev, *args, st)
        kernels.append(L.last_kernel())

    try:
        for k, v in case.get("options", {}).items():
            L.set_option(k, v)
        L.profile_enable(True)
        run = {"gemm": _run_gemm, "group": _run_group, "transpose": _run_transpose, "tall": _run_tall, "layer": _run_layer}[case["kind"]]
        bufs = run(case, dev, L, call)
        torch.cuda.synchronize(dev)
        prof = {}
        for name in PROF_NAMES:
            n, _, by = L.profile_get(name)
            if n:
                prof[name] = [n, by, L.profile_get_flops(name)]
    finally:
        L.profile_enable(False)
        for k in case.get("options", {}):
            L.set_option(k, DEFAULTS[k])
    return kernels, prof, {k: t for k, t in bufs.items() if isinstance(t, torch.Tensor)}


def run_case(case, dev):
    kernels, prof, bufs = _run_once(case, dev)
    return dict(kernels=kernels, prof=prof, hashes={k: _sha(t) for k, t in bufs.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=FIXTURE)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    from mp_former_amd import _lib
    out = {"device": torch.cuda.get_device_name(dev), "cases": {}, "unstable": {}}
    for cid, case in CASES.items():
        r, again = run_case(case, dev), run_case(case, dev)
        print(f"{cid:<44} {' | '.join(r['kernels'])}\n    prof {r['prof']}", flush=True)
        if (again["kernels"], again["prof"], sorted(again["hashes"])) != (r["kernels"], r["prof"], sorted(r["hashes"])):
            raise SystemExit(f"{cid}: kernels or profiler records of two runs differ")
        unstable = sorted(k for k in r["hashes"] if again["hashes"][k] != r["hashes"][k])
        if unstable:
            print(f"    UNSTABLE between two runs, left out: {unstable}", flush=True)
            out["unstable"][cid] = unstable
            for k in unstable:
                del r["hashes"][k]
        out["cases"][cid] = r
    print(f"library {_lib.LIB_PATH}; {len(CASES)} cases; unstable: {out['unstable']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
