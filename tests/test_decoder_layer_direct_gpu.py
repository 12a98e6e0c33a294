"""``decoder_layer()`` (mp_former_amd/decoder_layer.py, csrc/decoder_layer.hip) called directly: forward and every gradient of
ONE layer against a plain fp64 torch reference that shares no kernel with it, at the smallest shapes that reach each branch
(one row, ragged query / key counts, strided key / value column blocks, the packed dK / dV buffer, all three gradient operands),
plus the exact properties of the two masks.  The whole-head step tests compare losses and whole-model gradient norms against the
op-by-op path, which launches the same kernels: a wrong arena offset, image stride, column block or LayerNorm gradient row passes
there and fails here."""
import math

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu

H, HD, E = 8, 32, 256
EPS = 1e-5
NAMES = ("ca_wq", "ca_bq", "ca_wo", "ca_bo", "ca_gamma", "ca_beta",
         "sa_wq", "sa_bq", "sa_wk", "sa_bk", "sa_wv", "sa_bv", "sa_wo", "sa_bo", "sa_gamma", "sa_beta",
         "ff_w1", "ff_b1", "ff_w2", "ff_b2", "ff_gamma", "ff_beta")
SEEDS = ("g_x3", "g_xb3", "g_x3h")
ACTS = ("d_x0", "d_xb0", "d_k_c", "d_v_c")

# (Qt, N, S, ffn_dim, MP-isolation mask_s, K/V layout: None = dense | (column block j of [S, N, 3 * 256], through split_cols))
CASES = [(1, 1, 8, 32, False, None),
         (7, 3, 77, 96, False, None),
         (33, 2, 200, 2048, True, (1, False)),
         (114, 2, 1024, 2048, True, (2, True)),
         (230, 1, 64, 256, False, None),
         (40, 3, 2040, 2048, True, (0, True))]
VARIANT_CASE = (33, 2, 200, 2048, True, None)


# ---- the reference -------------------------------------------------------------------------------------------------------------
def _mha(q, k, v, mask):
    """softmax(q k^T / sqrt(32), masked) v per head; q [Lq, N, 256], k / v [Lk, N, 256], mask [N, Lq, Lk] / [Lq, Lk] / None"""
    Lq, N, _ = q.shape
    Lk = k.shape[0]
    qh = q.reshape(Lq, N, H, HD).permute(1, 2, 0, 3)
    kh = k.reshape(Lk, N, H, HD).permute(1, 2, 0, 3)
    vh = v.reshape(Lk, N, H, HD).permute(1, 2, 0, 3)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(HD)
    if mask is not None:
        s = s.masked_fill(mask[:, None] if mask.dim() == 3 else mask, float("-inf"))
    return (torch.softmax(s, -1) @ vh).permute(2, 0, 1, 3).reshape(Lq, N, E)


def ref_layer(x0, xb0, k_c, v_c, mask_c, mask_s, params, eps):
    """One post-norm decoder layer in fp64, no intermediate rounding (the math transformer_decoder._layer_by_ops states).  x0: the
    residual stream, xb0: the operand copy the cross-attention query is projected from — independent inputs.  -> x3"""
    p = params
    assert all(t.dtype == torch.float64 for t in (x0, xb0, k_c, v_c, *p.values()))
    t = _mha(xb0 @ p["ca_wq"].T + p["ca_bq"], k_c, v_c, mask_c) @ p["ca_wo"].T + p["ca_bo"]
    y1 = F.layer_norm(x0 + t, (E,), p["ca_gamma"], p["ca_beta"], eps)
    t = _mha(y1 @ p["sa_wq"].T + p["sa_bq"], y1 @ p["sa_wk"].T + p["sa_bk"], y1 @ p["sa_wv"].T + p["sa_bv"], mask_s)
    y2 = F.layer_norm(y1 + t @ p["sa_wo"].T + p["sa_bo"], (E,), p["sa_gamma"], p["sa_beta"], eps)
    t = torch.relu(y2 @ p["ff_w1"].T + p["ff_b1"]) @ p["ff_w2"].T + p["ff_b2"]
    return F.layer_norm(y2 + t, (E,), p["ff_gamma"], p["ff_beta"], eps)


def yard_layer(x0, xb0, k_c, v_c, mask_c, mask_s, params, eps):
    """The yardstick: torch's own bf16 composition of the same layer.  F.linear on bf16; attention as nn.MultiheadAttention runs it
    under autocast (q scaled, bf16 scores, softmax in fp32, probabilities cast to bf16, bf16 product with v); F.layer_norm in fp32
    on the fp32 residual; a bf16 result wherever the op-by-op path stores one.  -> (x3 fp32, xb3 bf16)"""
    p = params

    def mha(q, k, v, mask):
        Lq, N, _ = q.shape
        Lk = k.shape[0]
        qh = (q * (1.0 / math.sqrt(HD))).reshape(Lq, N, H, HD).permute(1, 2, 0, 3)
        kh = k.reshape(Lk, N, H, HD).permute(1, 2, 0, 3)
        vh = v.reshape(Lk, N, H, HD).permute(1, 2, 0, 3)
        s = (qh @ kh.transpose(-1, -2)).float()
        if mask is not None:
            s = s.masked_fill(mask[:, None] if mask.dim() == 3 else mask, float("-inf"))
        return (torch.softmax(s, -1).bfloat16() @ vh).permute(2, 0, 1, 3).reshape(Lq, N, E)

    t = F.linear(mha(F.linear(xb0, p["ca_wq"], p["ca_bq"]), k_c, v_c, mask_c), p["ca_wo"], p["ca_bo"])
    y1 = F.layer_norm(x0 + t.float(), (E,), p["ca_gamma"], p["ca_beta"], eps)
    b1 = y1.bfloat16()
    t = mha(F.linear(b1, p["sa_wq"], p["sa_bq"]), F.linear(b1, p["sa_wk"], p["sa_bk"]), F.linear(b1, p["sa_wv"], p["sa_bv"]), mask_s)
    y2 = F.layer_norm(y1 + F.linear(t, p["sa_wo"], p["sa_bo"]).float(), (E,), p["sa_gamma"], p["sa_beta"], eps)
    t = F.linear(torch.relu(F.linear(y2.bfloat16(), p["ff_w1"], p["ff_b1"])), p["ff_w2"], p["ff_b2"])
    x3 = F.layer_norm(y2 + t.float(), (E,), p["ff_gamma"], p["ff_beta"], eps)
    return x3, x3.bfloat16()


# ---- problems --------------------------------------------------------------------------------------------------------------------
def _problem(case, seed=0):
    """Everything of a case on the CPU from one seeded generator; bf16 tensors are drawn, rounded to bf16 and kept in bf16, so the
    fp64 reference (which widens them) and the kernels see the same numbers."""
    Qt, N, S, F_, mp, kv = case
    g = torch.Generator().manual_seed(100000 * seed + 1000 * Qt + 10 * S + N)

    def r(*shape, scale=1.0):
        return torch.randn(*shape, generator=g) * scale

    P = {"case": case, "x0": r(Qt, N, E), "xb0": r(Qt, N, E).bfloat16()}
    ncol = 3 * E if kv is not None else E
    P["Kp"], P["Vp"] = r(S, N, ncol, scale=1.5).bfloat16(), r(S, N, ncol).bfloat16()
    # as test_attn_gpu._problem("3d"): ~70 % blocked, a row with one open key, an open row, a row whose first half is blocked
    m = torch.rand(N, Qt, S, generator=g) < 0.7
    m[:, 0] = True
    m[:, 0, 5] = False
    if Qt > 1:
        m[:, 1] = False
    if Qt > 2:
        m[:, 2, :S // 2] = True
    m &= ~m.all(-1, keepdim=True)                      # decoder invariant: no fully blocked row
    P["mask_c"] = m
    P["mask_s"] = None
    if mp:
        P["mask_s"] = torch.zeros(Qt, Qt, dtype=torch.bool)
        P["mask_s"][Qt // 3:, :Qt // 3] = True         # MP isolation: the matching part does not see the padding rows

    def w(o, i):
        return r(o, i, scale=i ** -0.5).bfloat16()

    def b(n):
        return r(n, scale=0.2).bfloat16()

    prm = {}
    for blk in ("ca", "sa"):
        for n in (("wq", "wo") if blk == "ca" else ("wq", "wk", "wv", "wo")):
            prm[f"{blk}_{n}"], prm[f"{blk}_b{n[1]}"] = w(E, E), b(E)
    prm["ff_w1"], prm["ff_b1"], prm["ff_w2"], prm["ff_b2"] = w(F_, E), b(F_), w(E, F_), b(E)
    for blk in ("ca", "sa", "ff"):                    # per-norm gammas / betas far from (1, 0): a swapped d_ln row is an O(1) error
        prm[blk + "_gamma"], prm[blk + "_beta"] = 1 + r(E, scale=0.3), r(E, scale=0.2)
    P["params"] = {n: prm[n] for n in NAMES}
    P["g_x3"], P["g_xb3"], P["g_x3h"] = r(Qt, N, E), r(Qt, N, E).bfloat16(), r(Qt, N, E)
    return P


def _block(P, t):
    kv = P["case"][5]
    return t if kv is None else t[..., kv[0] * E:(kv[0] + 1) * E]


def _run_torch(fn, P, dev, wide):
    """ref_layer (wide: fp64) or yard_layer on a problem with all three gradient seeds -> {name: tensor}"""
    def leaf(t):
        t = t.to(dev)
        return (t.double() if wide else t).detach().clone().requires_grad_(True)

    def mask(t):
        return t.to(dev) if t is not None else None

    x0, xb0 = leaf(P["x0"]), leaf(P["xb0"])
    k_c, v_c = leaf(_block(P, P["Kp"]).contiguous()), leaf(_block(P, P["Vp"]).contiguous())
    prm = {n: leaf(t) for n, t in P["params"].items()}
    g32, g16 = P["g_x3"].to(dev), P["g_xb3"].to(dev)
    out = fn(x0, xb0, k_c, v_c, mask(P["mask_c"]), mask(P["mask_s"]), prm, EPS)
    if wide:
        x3 = xb3 = out
        x3.backward(g32.double() + P["g_x3h"].to(dev).double() + g16.double())
    else:
        x3, xb3 = out
        torch.autograd.backward([x3, xb3], [g32 + P["g_x3h"].to(dev), g16])
    res = {"x3": x3.detach(), "xb3": xb3.detach(), "d_x0": x0.grad, "d_xb0": xb0.grad, "d_k_c": k_c.grad, "d_v_c": v_c.grad}
    res.update({"d_" + n: t.grad for n, t in prm.items()})
    return res


def _param_leaves(prm, dev, packed=True):
    """the 22 parameters on the device as leaves.  packed: q / k / v weights (and biases) of the self-attention are row blocks of ONE
    tensor, as the decoder hands them over (one blocked GEMM each way); otherwise every tensor apart from the others (three GEMMs)"""
    out = {n: t.to(dev) for n, t in prm.items()}
    for names in (("sa_wq", "sa_wk", "sa_wv"), ("sa_bq", "sa_bk", "sa_bv")):
        if packed:
            cat = torch.cat([out[n] for n in names])
            for i, n in enumerate(names):
                out[n] = cat[i * E:(i + 1) * E]
        else:
            numel = out[names[0]].numel()
            buf = torch.empty(3, numel + 64, dtype=torch.bfloat16, device=dev)
            for i, n in enumerate(names):
                buf[i, :numel].copy_(out[n].flatten())
                out[n] = buf[i, :numel].view(out[n].shape)
    return [out[n].requires_grad_(True) for n in NAMES]


def _forward_native(P, dev, packed=True):
    from mp_former_amd.decoder_layer import PARAM_NAMES, decoder_layer, split_cols
    assert PARAM_NAMES == NAMES
    kv = P["case"][5]
    T = {"x0": P["x0"].to(dev).requires_grad_(True), "xb0": P["xb0"].to(dev).requires_grad_(True),
         "Kp": P["Kp"].to(dev).requires_grad_(True), "Vp": P["Vp"].to(dev).requires_grad_(True)}
    pack = None
    if kv is None:
        k_c, v_c = T["Kp"], T["Vp"]
    elif kv[1]:
        (k_c, hk), (v_c, hv) = split_cols(T["Kp"], 3)[kv[0]], split_cols(T["Vp"], 3)[kv[0]]
        pack = (hk, hv)
    else:
        k_c, v_c = _block(P, T["Kp"]), _block(P, T["Vp"])
    T["params"] = _param_leaves(P["params"], dev, packed)
    mask_s = P["mask_s"].to(dev) if P["mask_s"] is not None else None
    T["outs"] = decoder_layer(T["x0"], T["xb0"], k_c, v_c, P["mask_c"].to(dev), mask_s, H, EPS, T["params"], pack)
    return T


def _run_native(P, dev, seeds=SEEDS, packed=True):
    """the native layer on a problem, backward with the given subset of the three gradient operands -> {name: tensor}"""
    T = _forward_native(P, dev, packed)
    x3, xb3, x3h = T["outs"]
    outs = dict(zip(SEEDS, (x3, xb3, x3h)))
    torch.autograd.backward([outs[s] for s in seeds], [P[s].to(dev) for s in seeds])
    res = {"x3": x3.detach(), "xb3": xb3.detach(), "alias": x3h.data_ptr() == x3.data_ptr(), "d_x0": T["x0"].grad, "d_xb0": T["xb0"].grad,
           "d_Kp": T["Kp"].grad, "d_Vp": T["Vp"].grad, "d_k_c": _block(P, T["Kp"].grad), "d_v_c": _block(P, T["Vp"].grad)}
    res.update({"d_" + n: t.grad for n, t in zip(NAMES, T["params"])})
    return res


_cache = {}


def _shared(case, what):
    """fp64 reference, bf16 yardstick and native results of a case, computed once for the tests that need them (read only)"""
    key = (case, what)
    if key not in _cache:
        dev = torch.device("cuda:0")
        P = _cache.setdefault((case, "problem"), _problem(case))
        if what == "ref":
            _cache[key] = _run_torch(ref_layer, P, dev, True)
        elif what == "yard":
            _cache[key] = _run_torch(yard_layer, P, dev, False)
        elif what == "native":
            # (the second case runs the three-GEMM form of the self-attention projections, every other one the packed form)
            _cache[key] = _run_native(P, dev, packed=case != CASES[1])
    return _cache[key]


# ---- metrics ---------------------------------------------------------------------------------------------------------------------
def _seed_scale(P):
    """median row norm of the total gradient seed: every gradient of the layer is linear in it with O(1) factors"""
    return float((P["g_x3"].double() + P["g_x3h"].double() + P["g_xb3"].double()).norm(dim=-1).median())


def _row_stats(a, ref):
    """relative L2 per row (last dimension) against ref, rows of small norm measured against 0.25 x the median row norm
    -> (median, 99th percentile, max)"""
    a, ref = a.double().reshape(-1, a.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    d, rn = (a - ref).norm(dim=-1), ref.norm(dim=-1)
    rel = d / torch.maximum(rn, 0.25 * rn.median()).clamp_min(1e-300)
    p99 = rel.kthvalue(max(1, int(0.99 * rel.numel()))).values
    return float(rel.median()), float(p99), float(rel.max())


def _rel_l2(a, ref):
    return float((a.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300))


def _stats(a, ref):
    """activations and their gradients [L, N, 256]: per (row, image); 2-D weights: per tensor and per output row; vectors: per tensor"""
    out = [] if a.dim() == 3 else [("l2", _rel_l2(a, ref))]
    if a.dim() >= 2:
        out += list(zip(("row median", "row p99", "row max"), _row_stats(a, ref)))
    return out


def _judge(tag, name, got, ref, yard, yard_ref, G):
    """-> list of failures of tensor ``name`` of the dict ``got`` (against ``ref``) at the bar  2 x (the yardstick's statistic) + 2^-9.
    The yardstick is torch's bf16 composition of the layer (``yard``) measured against its fp64 reference (``yard_ref``) with the
    same statistic; the factor 2 allows for a different fp32 summation order flipping bf16 roundings, 2^-9 is half a bf16 ulp
    relative to the row / tensor.  Two kinds of tensor have a vanishing fp64 reference and with it no relative error:
    - d_sa_bk, in every case: a key bias shifts all scores of a query alike, its gradient is zero.  What both sides hold is rounding
      residue of the column sums of dk (bf16 dk rows; delta = sum(dO . O) taken from the bf16-rounded output, so the dS of a query
      do not sum to zero exactly).  Its sibling d_sa_bq is the column sum of dq over the same rows, out of the same attention
      backward with the same rounding points: the ABSOLUTE error the bar grants d_sa_bq is the one it grants d_sa_bk.
    - Qt = 1: the only query row has ONE open key, its softmax is the constant 1, so dq = dk = 0 exactly and with them d_xb0,
      d_ca_wq, d_ca_bq (likewise the self-attention over one row).  The native value is fp32 round-off of terms that cancel
      (dS = P (dP - delta), the two sums in different orders): at most 2^-16 of the seed's scale per element — 2^-23 with 2^7 for
      the lengths of the sums and the O(1) factors behind them — or 2 x what the yardstick holds there."""
    g, r, y, yr = got[name], ref[name], yard[name], yard_ref[name]
    if not torch.isfinite(g.float()).all():
        return [f"{tag} {name}: not finite"]
    if name == "d_sa_bk" and float(yard_ref["d_sa_bq"].abs().max()) >= 2.0 ** -16 * G:
        scale = float(yard_ref["d_sa_bq"].double().norm())
        e = float((g.double() - r.double()).norm()) / scale
        e_y = float(y.double().norm()) / scale
        bar = 2 * _rel_l2(yard["d_sa_bq"], yard_ref["d_sa_bq"]) + 2.0 ** -9
        print(f"[layer] {tag} {name}: zero gradient, residue / |d_sa_bq| {e:.5f} (torch bf16 {e_y:.5f}, bar {bar:.4f})")
        return [] if e <= bar else [f"{tag} {name}: residue {e:.4f} of |d_sa_bq| > {bar:.4f}"]
    if G > 0 and float(yr.abs().max()) < 2.0 ** -16 * G:
        m, my = float(g.double().abs().max()), float(y.double().abs().max())
        print(f"[layer] {tag} {name}: reference vanishes, native max-abs {m:.2e} (torch bf16 {my:.2e})")
        return [] if m <= max(2 * my, 2.0 ** -16 * G) else [f"{tag} {name}: {m:.3e} where the reference vanishes (torch bf16 {my:.3e})"]
    stats = [(k, a, b) for (k, a), (_, b) in zip(_stats(g, r), _stats(y, yr))]
    print(f"[layer] {tag} {name}: " + "  ".join(f"{k} {a:.4f} (torch bf16 {b:.4f})" for k, a, b in stats))
    return [f"{tag} {name} {k}: native {a:.4f} > 2 x {b:.4f} + 2^-9" for k, a, b in stats if not a <= 2 * b + 2.0 ** -9]


def _tag(case):
    Qt, N, S, F_, mp, kv = case
    return f"Qt {Qt} N {N} S {S} F {F_}"


# ---- 1a: the reference against torch's fp64 modules (CPU) -------------------------------------------------------------------------
@pytest.mark.parametrize("mp", [False, True])
def test_cpu_reference_matches_fp64_torch_modules(mp):
    """ref_layer against nn.MultiheadAttention / nn.LayerNorm / nn.Linear in fp64 with the same parameters (xb0 = x0: the modules
    have one input).  The cross-attention module gets identity key / value projections: k_c / v_c are the projected ones."""
    import torch.nn as nn
    Qt, N, S, F_ = 7, 3, 20, 96
    P = _problem((Qt, N, S, F_, mp, None), seed=1)
    g = torch.Generator().manual_seed(5)
    prm = {n: torch.randn(t.shape, generator=g, dtype=torch.float64).mul_(0.3 if t.dim() == 1 else t.shape[1] ** -0.5).requires_grad_(True)
           for n, t in P["params"].items()}
    x, k_c, v_c = (torch.randn(s, N, E, generator=g, dtype=torch.float64).requires_grad_(True) for s in (Qt, S, S))
    go = torch.randn(Qt, N, E, generator=g, dtype=torch.float64)
    ref_layer(x, x, k_c, v_c, P["mask_c"], P["mask_s"], prm, EPS).backward(go)
    want = {"x": x.grad, "k_c": k_c.grad, "v_c": v_c.grad, **{n: t.grad for n, t in prm.items()}}

    ca, sa = (nn.MultiheadAttention(E, H, dropout=0.0).double() for _ in range(2))
    n1, n2, n3 = (nn.LayerNorm(E, eps=EPS).double() for _ in range(3))
    l1, l2 = nn.Linear(E, F_).double(), nn.Linear(F_, E).double()
    eye, zero = torch.eye(E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    d = {n: t.detach() for n, t in prm.items()}
    with torch.no_grad():
        ca.in_proj_weight.copy_(torch.cat([d["ca_wq"], eye, eye]))
        ca.in_proj_bias.copy_(torch.cat([d["ca_bq"], zero, zero]))
        sa.in_proj_weight.copy_(torch.cat([d["sa_wq"], d["sa_wk"], d["sa_wv"]]))
        sa.in_proj_bias.copy_(torch.cat([d["sa_bq"], d["sa_bk"], d["sa_bv"]]))
        for m, blk in ((ca, "ca"), (sa, "sa")):
            m.out_proj.weight.copy_(d[blk + "_wo"])
            m.out_proj.bias.copy_(d[blk + "_bo"])
        for m, blk in ((n1, "ca"), (n2, "sa"), (n3, "ff")):
            m.weight.copy_(d[blk + "_gamma"])
            m.bias.copy_(d[blk + "_beta"])
        l1.weight.copy_(d["ff_w1"]); l1.bias.copy_(d["ff_b1"]); l2.weight.copy_(d["ff_w2"]); l2.bias.copy_(d["ff_b2"])
    xm, km, vm = (t.detach().clone().requires_grad_(True) for t in (x, k_c, v_c))
    mc = P["mask_c"][:, None].expand(N, H, Qt, S).reshape(N * H, Qt, S)        # nn.MultiheadAttention: batch index n * H + h
    y1 = n1(xm + ca(xm, km, vm, attn_mask=mc, need_weights=False)[0])
    y2 = n2(y1 + sa(y1, y1, y1, attn_mask=P["mask_s"], need_weights=False)[0])
    y3 = n3(y2 + l2(torch.relu(l1(y2))))
    y3.backward(go)
    got = {"x": xm.grad, "k_c": km.grad, "v_c": vm.grad,
           "ca_wq": ca.in_proj_weight.grad[:E], "ca_bq": ca.in_proj_bias.grad[:E],
           "sa_wq": sa.in_proj_weight.grad[:E], "sa_wk": sa.in_proj_weight.grad[E:2 * E], "sa_wv": sa.in_proj_weight.grad[2 * E:],
           "sa_bq": sa.in_proj_bias.grad[:E], "sa_bk": sa.in_proj_bias.grad[E:2 * E], "sa_bv": sa.in_proj_bias.grad[2 * E:],
           "ca_wo": ca.out_proj.weight.grad, "ca_bo": ca.out_proj.bias.grad, "sa_wo": sa.out_proj.weight.grad, "sa_bo": sa.out_proj.bias.grad,
           "ca_gamma": n1.weight.grad, "ca_beta": n1.bias.grad, "sa_gamma": n2.weight.grad, "sa_beta": n2.bias.grad,
           "ff_gamma": n3.weight.grad, "ff_beta": n3.bias.grad,
           "ff_w1": l1.weight.grad, "ff_b1": l1.bias.grad, "ff_w2": l2.weight.grad, "ff_b2": l2.bias.grad}
    assert set(got) == set(want) and len(got) == 3 + len(NAMES)
    with torch.no_grad():
        out = ref_layer(x, x, k_c, v_c, P["mask_c"], P["mask_s"], prm, EPS)
    assert float((out - y3.detach()).abs().max()) <= 1e-10 * float(y3.detach().abs().max())
    for n in want:
        # (a key bias shifts all scores of a query alike: its gradient is zero, ~1e-16 on both sides — measured on the query bias's scale)
        scale = float(got["sa_bq" if n == "sa_bk" else n].abs().max())
        assert float((want[n] - got[n]).abs().max()) <= 1e-10 * scale, n
    assert float(want["sa_bk"].abs().max()) <= 1e-10 * float(want["sa_bq"].abs().max())


# ---- 1b: parity against fp64 -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", CASES, ids=_tag)
def test_layer_matches_fp64_reference(case):
    """x3, xb3, the four activation gradients and the 22 parameter gradients of the native layer against fp64 autograd through
    ref_layer, all three gradient operands present (the reference's seed is their sum).  Measured on an MI355X over the six cases
    (native | torch bf16; the lines this test prints):
      x3 / xb3 rows            median 0.0025-0.0032 | 0.0025-0.0035, p99 <= 0.0037 | 0.0041, max <= 0.0040 | 0.0042
      d_x0 / d_xb0 rows        median 0.0025-0.017  | 0.0025-0.023,  p99 <= 0.11   | 0.093,  max <= 0.12   | 0.12
      d_k_c / d_v_c rows       median <= 0.023      | <= 0.027,      p99 <= 0.094  | 0.105,  max <= 0.59   | 0.52
      parameter tensors (l2)   <= 0.028 | <= 0.033 (d_ff_w1 / d_ff_b1, behind the ReLU gate: <= 0.049 | 0.046)
      weight rows              median 0.003-0.026 | 0.003-0.028, p99 <= 0.14 | 0.12, max <= 0.28 | 0.19 (d_ff_w1: max <= 0.57 | 0.75)
      d_sa_bk (zero gradient)  residue max-abs 0.03-0.08 | 0.02-0.04 (1.6e-7 | 0 at Qt = 1)
    i.e. the native layer sits where torch's own bf16 composition sits, tensor by tensor.  The gradients are an order of magnitude
    further from fp64 than the forward on both sides: three LayerNorm backwards and two softmax backwards on bf16 operands; single
    key rows and weight rows reach tens of percent where a ReLU gate or a near-empty key column makes the row a small difference."""
    P = _cache.setdefault((case, "problem"), _problem(case))
    ref, yard, got = _shared(case, "ref"), _shared(case, "yard"), _shared(case, "native")
    G, tag = _seed_scale(P), _tag(case)
    # exact: the third result is the first, xb3 is the bf16 copy of x3
    assert got["alias"]
    assert torch.equal(got["xb3"], got["x3"].bfloat16())
    bad = []
    for n in ("x3", "xb3") + ACTS + tuple("d_" + n for n in NAMES):
        bad += _judge(tag, n, got, ref, yard, ref, 0.0 if n in ("x3", "xb3") else G)
    if case[5] is not None:                 # the column blocks of the packed gradient that are not this layer's: zero, not stale
        j = case[5][0]
        for n in ("d_Kp", "d_Vp"):
            others = [got[n][..., c * E:(c + 1) * E] for c in range(3) if c != j]
            assert all(bool((o == 0).all()) for o in others), n
    assert not bad, "\n".join(bad)


# ---- 1c: the fused layer against the op-by-op path -----------------------------------------------------------------------------
def _run_by_ops(P, dev):
    """The layer as transformer_decoder._layer_by_ops composes it (masked_mha_w, res_ln, linear, one autograd node per op) under
    autocast.  The cross-attention keys / values arrive projected here, so its masked_mha_w is spelled out without the two
    projections; the self-attention is masked_mha_w itself with the q / k / v row blocks."""
    from types import SimpleNamespace
    from mp_former_amd.attention import attention_core
    from mp_former_amd.resln import res_ln
    from mp_former_amd.transformer_decoder import linear, masked_mha_w
    x0, xb0 = P["x0"].to(dev).requires_grad_(True), P["xb0"].to(dev).requires_grad_(True)
    k_c, v_c = (_block(P, P[n]).contiguous().to(dev).requires_grad_(True) for n in ("Kp", "Vp"))
    prm = dict(zip(NAMES, _param_leaves(P["params"], dev)))
    mask_c = P["mask_c"].to(dev)
    mask_s = P["mask_s"].to(dev) if P["mask_s"] is not None else None

    def norm(blk):
        return SimpleNamespace(weight=prm[blk + "_gamma"], bias=prm[blk + "_beta"], eps=EPS, elementwise_affine=True)

    with torch.autocast("cuda", dtype=torch.bfloat16):
        t2 = linear(attention_core(linear(xb0, prm["ca_wq"], prm["ca_bq"]), k_c, v_c, mask_c, H), prm["ca_wo"], prm["ca_bo"])
        out, xb = res_ln(norm("ca"), x0, t2, want32=True, want16=True)
        t2 = masked_mha_w(xb, xb, xb, (prm["sa_wq"], prm["sa_wk"], prm["sa_wv"]), (prm["sa_bq"], prm["sa_bk"], prm["sa_bv"]),
                          prm["sa_wo"], prm["sa_bo"], H, mask_s)
        out, xb = res_ln(norm("sa"), out, t2, want32=True, want16=True)
        t2 = linear(linear(xb, prm["ff_w1"], prm["ff_b1"], relu=True), prm["ff_w2"], prm["ff_b2"])
        x3, xb3 = res_ln(norm("ff"), out, t2, want32=True, want16=True)
    torch.autograd.backward([x3, xb3], [P["g_x3"].to(dev) + P["g_x3h"].to(dev), P["g_xb3"].to(dev)])
    res = {"x3": x3.detach(), "xb3": xb3.detach(), "d_x0": x0.grad, "d_xb0": xb0.grad, "d_k_c": k_c.grad, "d_v_c": v_c.grad}
    res.update({"d_" + n: t.grad for n, t in prm.items()})
    return res


@gpu
@pytest.mark.parametrize("case", CASES, ids=_tag)
def test_fused_layer_equals_the_op_by_op_composition(case):
    """Same kernels, same rounding points: the forward bit for bit; every gradient tensor of the single layer to relative L2 2e-2
    (the bar tests/test_decoder_layer_gpu.py sets per model: the order of bf16 accumulation differs — the fused backward sums its
    two gradient operands inside the first LayerNorm pass and issues the weight gradients as one grouped launch on transposed copies)."""
    P = _cache.setdefault((case, "problem"), _problem(case))
    got, ops = _shared(case, "native"), _run_by_ops(P, torch.device("cuda:0"))
    assert torch.equal(got["x3"], ops["x3"]) and torch.equal(got["xb3"], ops["xb3"])
    G, bad = _seed_scale(P), []
    for n in ACTS + tuple("d_" + n for n in NAMES):
        a, b = got[n].double(), ops[n].double()
        if max(float(a.abs().max()), float(b.abs().max())) < 2.0 ** -16 * G:       # round-off where the gradient vanishes (see _judge)
            continue
        # (the key bias's gradient is zero, both sides hold rounding residue: measured on the scale of its sibling, see _judge)
        rel = float((a - b).norm() / (ops["d_sa_bq"].double().norm() if n == "d_sa_bk" else b.norm()))
        print(f"[layer] {_tag(case)} fused vs ops {n}: {rel:.2e}")
        if not rel < 2e-2:
            bad.append((n, rel))
    assert not bad, bad


# ---- 1d: the gradient operands ---------------------------------------------------------------------------------------------------
def _ulp_bf16(t):
    return torch.exp2(torch.floor(torch.log2(t.abs().double().clamp_min(2.0 ** -126))) - 7)


@gpu
def test_gradient_operand_variants_are_linear_in_the_seed():
    """g_x3, g_xb3 and g_x3h (the gradient of the output's second alias) alone and together on one forward: the backward is linear
    in its seed, so the third operand must act exactly like a term of g_x3, and the three single runs must add up to the joint one."""
    from mp_former_amd import _lib
    from mp_former_amd.decoder_layer import DecoderLayerFn
    dev = torch.device("cuda:0")
    case = VARIANT_CASE
    P = _cache.setdefault((case, "problem"), _problem(case))
    T = _forward_native(P, dev)
    inputs = [T["x0"], T["xb0"], T["Kp"], T["Vp"]] + T["params"]
    names = ACTS + tuple("d_" + n for n in NAMES)
    a, bf, b = (P[s].to(dev) for s in SEEDS)

    def grads(**seeds):
        outs = dict(zip(SEEDS, T["outs"]))
        gs = torch.autograd.grad([outs[k] for k in seeds], inputs, list(seeds.values()), retain_graph=True)
        assert all(torch.isfinite(g.float()).all() for g in gs)
        return dict(zip(names, gs))

    def same_up_to_roundoff(x, y, what):
        """fp32 results to fp32 round-off; bf16 results: one bf16 ulp at most, on fewer than 1 % of the elements"""
        for n in names:
            d = (x[n].double() - y[n].double()).abs()
            if x[n].dtype == torch.float32:
                assert float(d.max()) <= 1e-5 * float(y[n].abs().max()), (what, n, float(d.max()))
            else:
                assert bool((d <= _ulp_bf16(torch.maximum(x[n].abs(), y[n].abs()))).all()), (what, n, float(d.max()))
                assert float((d > 0).double().mean()) < 0.01, (what, n, float((d > 0).double().mean()))

    g_a, g_bf, g_b = grads(g_x3=a), grads(g_xb3=bf), grads(g_x3h=b)
    same_up_to_roundoff(grads(g_x3h=a), g_a, "g_x3h alone acts as g_x3")
    same_up_to_roundoff(grads(g_x3=a, g_x3h=b), grads(g_x3=a + b), "g_x3 + g_x3h")
    # the three single runs add up to the joint run, within the bar of the parity test (2 x torch's bf16 distance from fp64 + 2^-9);
    # measured: row medians 0.001-0.003, i.e. the bf16 rounding of each run's stored gradients
    joint = grads(g_x3=a, g_xb3=bf, g_x3h=b)
    ref, yard = _shared(case, "ref"), _shared(case, "yard")
    G, bad = _seed_scale(P), []
    total = {n: g_a[n].double() + g_bf[n].double() + g_b[n].double() for n in names}
    for n in names:
        bad += _judge("sum of single seeds", n, joint, total, yard, ref, G)
    assert not bad, "\n".join(bad)
    # no gradient at all: nothing to do, nothing launched (no context is touched)
    _lib.profile_enable(True)
    try:
        n0 = _lib.profile_get("")[0]
        none = DecoderLayerFn.backward(None, None, None, None)
        assert _lib.profile_get("")[0] == n0
    finally:
        _lib.profile_enable(False)
    assert len(none) == 9 + len(NAMES) and all(g is None for g in none)


# ---- 1e: packed K / V through split_cols -------------------------------------------------------------------------------------------
@gpu
def test_packed_kv_gradients_land_in_their_column_blocks():
    """Kp / Vp [S, N, 3 * 256] feed two layers (different parameters) through split_cols, the third block feeds nobody: each layer
    writes its dK / dV block of the ONE packed gradient in place, bit-equal to the same layer on a dense copy of its block; the
    unused block is zero; the forward does not depend on the layout."""
    from mp_former_amd.decoder_layer import decoder_layer, split_cols
    dev = torch.device("cuda:0")
    Qt, N, S, F_ = 33, 2, 200, 96
    users = {0: _problem((Qt, N, S, F_, True, (0, True)), seed=2), 2: _problem((Qt, N, S, F_, False, (2, True)), seed=3)}
    Kp, Vp = (users[0][n].to(dev).requires_grad_(True) for n in ("Kp", "Vp"))

    def run(P, k_c, v_c, pack):
        x0, xb0 = P["x0"].to(dev), P["xb0"].to(dev)
        mask_s = P["mask_s"].to(dev) if P["mask_s"] is not None else None
        return decoder_layer(x0, xb0, k_c, v_c, P["mask_c"].to(dev), mask_s, H, EPS, _param_leaves(P["params"], dev), pack)

    ks, vs = split_cols(Kp, 3), split_cols(Vp, 3)
    outs, seeds = {}, []
    for j, P in users.items():
        outs[j] = run(P, ks[j][0], vs[j][0], (ks[j][1], vs[j][1]))
        seeds += [P[s].to(dev) for s in SEEDS]
    torch.autograd.backward([o for j in users for o in outs[j]], seeds)
    assert Kp.grad.shape == Kp.shape and Vp.grad.shape == Vp.shape
    for j, P in users.items():
        kd, vd = (t.detach()[..., j * E:(j + 1) * E].contiguous().requires_grad_(True) for t in (Kp, Vp))
        dense = run(P, kd, vd, None)
        torch.autograd.backward(list(dense), [P[s].to(dev) for s in SEEDS])
        assert torch.equal(dense[0], outs[j][0]) and torch.equal(dense[1], outs[j][1])
        assert torch.equal(Kp.grad[..., j * E:(j + 1) * E], kd.grad), j
        assert torch.equal(Vp.grad[..., j * E:(j + 1) * E], vd.grad), j
        assert float(kd.grad.float().abs().max()) > 0 and float(vd.grad.float().abs().max()) > 0
    assert bool((Kp.grad[..., E:2 * E] == 0).all()) and bool((Vp.grad[..., E:2 * E] == 0).all())


# ---- 1f: mask isolation ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Qt,S", [(7, 77), (40, 2040)])
def test_blocked_cross_attention_keys_have_no_influence(Qt, S):
    """Keys that mask_c blocks for every query of image 1 (of N = 3): whatever k_c / v_c hold there, x3 / xb3 are bit-identical and
    their dK / dV rows are exactly zero.  A wrong image or query stride of the mask, or a padded query row (Qt is no multiple of
    16) reaching a key, shows here."""
    dev = torch.device("cuda:0")
    n = 1
    P = _problem((Qt, 3, S, 96, False, None), seed=4)
    keys = torch.tensor([0, 6, 7] + list(range(16, 48)) + [S // 2, S - 2, S - 1])        # (key 5 is row 0's only open key)
    P["mask_c"][n][:, keys] = True
    assert not P["mask_c"].all(-1).any()
    base = _run_native(P, dev)
    Q = dict(P)
    g = torch.Generator().manual_seed(9)
    for name in ("Kp", "Vp"):
        t = P[name].clone()
        t[keys[:20], n] = (torch.randn(20, E, generator=g) * 3).bfloat16()
        t[keys[20:], n] = t[keys[20:], n] * 100
        Q[name] = t
    other = _run_native(Q, dev)
    for r in (base, other):
        assert bool((r["d_k_c"][keys, n] == 0).all()) and bool((r["d_v_c"][keys, n] == 0).all())
        assert all(torch.isfinite(v.float()).all() for k, v in r.items() if k != "alias")
    assert torch.equal(base["x3"], other["x3"]) and torch.equal(base["xb3"], other["xb3"])
    # (the perturbation is real: an open key of the same image moves the output)
    open_key = int((~P["mask_c"][n]).any(0).nonzero()[0])
    Q2 = dict(P)
    Q2["Vp"] = P["Vp"].clone()
    Q2["Vp"][open_key, n] *= 100
    assert not torch.equal(_forward_native(Q2, dev)["outs"][0].detach(), base["x3"])


@gpu
def test_mp_isolation_rows_do_not_reach_the_matching_part():
    """mask_s[pad:, :pad] = True: the rows pad: neither read the rows :pad (outputs bit-identical when those change) nor send them a
    gradient (d_x0[:pad] = d_xb0[:pad] = 0 exactly when only rows pad: carry a seed)."""
    dev = torch.device("cuda:0")
    Qt = 40
    pad = Qt // 3
    P = _problem((Qt, 2, 200, 96, True, None), seed=5)
    for s in SEEDS:
        P[s][:pad] = 0
    base = _run_native(P, dev)
    Q = dict(P)
    g = torch.Generator().manual_seed(10)
    Q["x0"], Q["xb0"] = P["x0"].clone(), P["xb0"].clone()
    Q["x0"][:pad] = torch.randn(pad, 2, E, generator=g) * 3
    Q["xb0"][:pad] = (torch.randn(pad, 2, E, generator=g) * 3).bfloat16()
    other = _run_native(Q, dev)
    assert torch.equal(base["x3"][pad:], other["x3"][pad:]) and torch.equal(base["xb3"][pad:], other["xb3"][pad:])
    assert not torch.equal(base["x3"][:pad], other["x3"][:pad])
    for r in (base, other):
        assert bool((r["d_x0"][:pad] == 0).all()) and bool((r["d_xb0"][:pad] == 0).all())
        assert float(r["d_x0"][pad:].abs().max()) > 0 and float(r["d_xb0"][pad:].float().abs().max()) > 0


@gpu
def test_images_are_independent():
    """everything of image 0 changed (x0, xb0, k_c, v_c, mask_c): image 1's rows of x3 / xb3 are bit-identical"""
    dev = torch.device("cuda:0")
    P = _problem((33, 2, 200, 96, True, None), seed=6)
    Q = _problem((33, 2, 200, 96, True, None), seed=7)
    M = dict(P)
    for name in ("x0", "xb0", "Kp", "Vp", "mask_c"):
        M[name] = P[name].clone()
        if name == "mask_c":
            M[name][0] = Q[name][0]
        else:
            M[name][:, 0] = Q[name][:, 0]
    a, b = _forward_native(P, dev)["outs"], _forward_native(M, dev)["outs"]
    assert torch.equal(a[0][:, 1], b[0][:, 1]) and torch.equal(a[1][:, 1], b[1][:, 1])
    assert not torch.equal(a[0][:, 0], b[0][:, 0])
