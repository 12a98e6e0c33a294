"""What the tests of the decoder layer with query positions share: the fp64 reference layer, torch's bf16 composition of it (the
yardstick of ``_judge``), the problems and the runners.  Built on the helpers of tests/test_decoder_layer_direct_gpu.py (the
layer without positions), which stay as they are."""
import math

import torch
import torch.nn.functional as F

from test_decoder_layer_direct_gpu import E, EPS, H, HD, NAMES, _block, _mha, _param_leaves, _problem

# (Qt, N, S, ffn_dim, mask_s, K/V layout: None = dense | (column block j of [S, N, 3 * 256], through split_cols))
CASES = [(1, 1, 8, 32, False, None),
         (7, 3, 77, 96, False, None),                  # run with the in-projection weights unpacked: the three-GEMM form
         (33, 2, 200, 2048, True, (1, True)),
         (230, 1, 64, 256, False, None),
         (100, 2, 480, 2048, False, (0, True))]
UNPACKED = CASES[1]
SEEDS = ("g_x3", "g_xb3", "g_x3h")
ACTS = ("d_x0", "d_qpos", "d_k_c", "d_v_c")
FAULTS = ("no_key_pos", "value_pos", "pos_row_mod_q", "d_qpos_self_only")


def tag(case):
    Qt, N, S, F_, mp, kv = case
    return f"Qt {Qt} N {N} S {S} F {F_}"


def problem(case, seed=0):
    """``_problem`` of the direct test plus qpos ~ N(0, 1) fp32 [Qt, 256]: a dropped or doubled position is an O(1) error"""
    P = _problem(case, seed)
    g = torch.Generator().manual_seed(777 + 100000 * seed + 1000 * case[0] + 10 * case[2] + case[1])
    P["qpos"] = torch.randn(case[0], E, generator=g)
    return P


def pos_rows(qpos, N, fault=None):
    """[Qt, N, 256]: the position of row r = q * N + n is qpos[r // N]; the fault indexes it by r % Qt"""
    Qt = qpos.shape[0]
    if fault == "pos_row_mod_q":
        r = torch.arange(Qt * N, device=qpos.device)
        return qpos[r % Qt].view(Qt, N, E)
    return qpos[:, None].expand(Qt, N, E)


def ref_layer_pos(x0, p_c, p_s, k_c, v_c, mask_c, mask_s, params, eps, fault=None):
    """One post-norm decoder layer with query positions in fp64, no intermediate rounding: ``ref_layer`` of the direct test with
    q_c from x0 + p, q_s and k_s from y1 + p, v_s from y1 (video_mask2former_transformer_decoder.py:415, :421).  p_c / p_s: the
    positions as the cross- / self-attention see them, [Qt, N, 256] (two arguments so that their gradients can be told apart).
    ``fault``: one of the single faults the tests must notice.  -> x3"""
    p = params
    t = _mha((x0 + p_c) @ p["ca_wq"].T + p["ca_bq"], k_c, v_c, mask_c) @ p["ca_wo"].T + p["ca_bo"]
    y1 = F.layer_norm(x0 + t, (E,), p["ca_gamma"], p["ca_beta"], eps)
    yq = y1 + p_s
    yk = y1 if fault == "no_key_pos" else yq
    yv = yq if fault == "value_pos" else y1
    t = _mha(yq @ p["sa_wq"].T + p["sa_bq"], yk @ p["sa_wk"].T + p["sa_bk"], yv @ p["sa_wv"].T + p["sa_bv"], mask_s)
    y2 = F.layer_norm(y1 + t @ p["sa_wo"].T + p["sa_bo"], (E,), p["sa_gamma"], p["sa_beta"], eps)
    t = torch.relu(y2 @ p["ff_w1"].T + p["ff_b1"]) @ p["ff_w2"].T + p["ff_b2"]
    return F.layer_norm(y2 + t, (E,), p["ff_gamma"], p["ff_beta"], eps)


def yard_layer_pos(x0, p_c, p_s, k_c, v_c, mask_c, mask_s, params, eps):
    """The yardstick: torch's own bf16 composition of the same layer (``yard_layer`` of the direct test with the positions added
    in fp32 before the operand is rounded, the reference's rounding point under autocast).  -> (x3 fp32, xb3 bf16)"""
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

    t = F.linear(mha(F.linear((x0 + p_c).bfloat16(), p["ca_wq"], p["ca_bq"]), k_c, v_c, mask_c), p["ca_wo"], p["ca_bo"])
    y1 = F.layer_norm(x0 + t.float(), (E,), p["ca_gamma"], p["ca_beta"], eps)
    b1, bq = y1.bfloat16(), (y1 + p_s).bfloat16()
    t = mha(F.linear(bq, p["sa_wq"], p["sa_bq"]), F.linear(bq, p["sa_wk"], p["sa_bk"]), F.linear(b1, p["sa_wv"], p["sa_bv"]), mask_s)
    y2 = F.layer_norm(y1 + F.linear(t, p["sa_wo"], p["sa_bo"]).float(), (E,), p["sa_gamma"], p["sa_beta"], eps)
    t = F.linear(torch.relu(F.linear(y2.bfloat16(), p["ff_w1"], p["ff_b1"])), p["ff_w2"], p["ff_b2"])
    x3 = F.layer_norm(y2 + t.float(), (E,), p["ff_gamma"], p["ff_beta"], eps)
    return x3, x3.bfloat16()


def run_torch(P, dev, wide, fault=None):
    """ref_layer_pos (wide: fp64, optionally with a single fault) or yard_layer_pos on a problem with all three gradient seeds
    -> {name: tensor}"""
    def leaf(t):
        t = t.to(dev)
        return (t.double() if wide else t).detach().clone().requires_grad_(True)

    def mask(t):
        return t.to(dev) if t is not None else None

    N = P["case"][1]
    x0 = leaf(P["x0"])
    q_c, q_s = leaf(P["qpos"]), leaf(P["qpos"])                      # one leaf per use: d_qpos = their sum
    k_c, v_c = leaf(_block(P, P["Kp"]).contiguous()), leaf(_block(P, P["Vp"]).contiguous())
    prm = {n: leaf(t) for n, t in P["params"].items()}
    g32, g16 = P["g_x3"].to(dev), P["g_xb3"].to(dev)
    args = (x0, pos_rows(q_c, N, fault), pos_rows(q_s, N, fault), k_c, v_c, mask(P["mask_c"]), mask(P["mask_s"]), prm, EPS)
    if wide:
        x3 = xb3 = ref_layer_pos(*args, fault=fault)
        x3.backward(g32.double() + P["g_x3h"].to(dev).double() + g16.double())
    else:
        x3, xb3 = yard_layer_pos(*args)
        torch.autograd.backward([x3, xb3], [g32 + P["g_x3h"].to(dev), g16])
    d_qpos = q_s.grad if fault == "d_qpos_self_only" else q_c.grad + q_s.grad
    res = {"x3": x3.detach(), "xb3": xb3.detach(), "d_x0": x0.grad, "d_qpos": d_qpos, "d_k_c": k_c.grad, "d_v_c": v_c.grad}
    res.update({"d_" + n: t.grad for n, t in prm.items()})
    return res


def forward_native(P, dev, packed=True):
    from mp_former_amd.decoder_layer import PARAM_NAMES, decoder_layer_pos, split_cols
    assert PARAM_NAMES == NAMES
    kv = P["case"][5]
    T = {"x0": P["x0"].to(dev).requires_grad_(True), "qpos": P["qpos"].to(dev).requires_grad_(True),
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
    T["outs"] = decoder_layer_pos(T["x0"], T["qpos"], k_c, v_c, P["mask_c"].to(dev), mask_s, H, EPS, T["params"], pack)
    return T


def run_native(P, dev, packed=True):
    """the native layer with positions on a problem, backward with the three gradient operands -> {name: tensor}"""
    T = forward_native(P, dev, packed)
    x3, xb3, x3h = T["outs"]
    torch.autograd.backward([x3, xb3, x3h], [P[s].to(dev) for s in SEEDS])
    res = {"x3": x3.detach(), "xb3": xb3.detach(), "alias": x3h.data_ptr() == x3.data_ptr(), "d_x0": T["x0"].grad,
           "d_qpos": T["qpos"].grad, "d_Kp": T["Kp"].grad, "d_Vp": T["Vp"].grad, "d_k_c": _block(P, T["Kp"].grad),
           "d_v_c": _block(P, T["Vp"].grad)}
    res.update({"d_" + n: t.grad for n, t in zip(NAMES, T["params"])})
    return res


def run_by_ops(P, dev):
    """The layer as video_decoder._layer_by_ops composes it (linear, attention_core, res_ln, one autograd node per op) under
    autocast, on projected cross-attention keys / values."""
    from types import SimpleNamespace
    from mp_former_amd.attention import attention_core
    from mp_former_amd.resln import res_ln
    from mp_former_amd.transformer_decoder import linear
    x0, qpos = P["x0"].to(dev).requires_grad_(True), P["qpos"].to(dev).requires_grad_(True)
    k_c, v_c = (_block(P, P[n]).contiguous().to(dev).requires_grad_(True) for n in ("Kp", "Vp"))
    prm = dict(zip(NAMES, _param_leaves(P["params"], dev)))
    mask_c = P["mask_c"].to(dev)
    mask_s = P["mask_s"].to(dev) if P["mask_s"] is not None else None
    qp = qpos.unsqueeze(1)

    def norm(blk):
        return SimpleNamespace(weight=prm[blk + "_gamma"], bias=prm[blk + "_beta"], eps=EPS, elementwise_affine=True)

    def cast(v):
        return v.to(torch.bfloat16)

    with torch.autocast("cuda", dtype=torch.bfloat16):
        q = linear(cast(x0 + qp), prm["ca_wq"], prm["ca_bq"])
        t2 = linear(attention_core(q, k_c, v_c, mask_c, H), prm["ca_wo"], prm["ca_bo"])
        out, xb = res_ln(norm("ca"), x0, t2, want32=True, want16=True)
        xq = cast(out + qp)
        o = attention_core(linear(xq, prm["sa_wq"], prm["sa_bq"]), linear(xq, prm["sa_wk"], prm["sa_bk"]),
                           linear(xb, prm["sa_wv"], prm["sa_bv"]), mask_s, H)
        t2 = linear(o, prm["sa_wo"], prm["sa_bo"])
        out, xb = res_ln(norm("sa"), out, t2, want32=True, want16=True)
        t2 = linear(linear(xb, prm["ff_w1"], prm["ff_b1"], relu=True), prm["ff_w2"], prm["ff_b2"])
        x3, xb3 = res_ln(norm("ff"), out, t2, want32=True, want16=True)
    torch.autograd.backward([x3, xb3], [P["g_x3"].to(dev) + P["g_x3h"].to(dev), P["g_xb3"].to(dev)])
    res = {"x3": x3.detach(), "xb3": xb3.detach(), "d_x0": x0.grad, "d_qpos": qpos.grad, "d_k_c": k_c.grad, "d_v_c": v_c.grad}
    res.update({"d_" + n: t.grad for n, t in prm.items()})
    return res
