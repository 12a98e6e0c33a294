"""Shifted-window attention problems for csrc/win_attn.hip (modelled on tests/_attn_cases.py).

  CASES            (B, Hp, Wp, heads, ws, shift): every token tail (9, 49, 64, 144 tokens), one-window maps, all nine mask regions
  build(case)      bf16-representable qkv, dout and an fp32 table, wide enough that the bias and the mask visibly move the softmax
  reference(prob)  fp64 restatement in the reference's own formulation (roll, window partition, index buffer, mask from slices)
                   with the per-element bounds of the kernels' first-order rounding model — the constants of _attn_cases.reference
                   — and a bound for the table gradient
  emulate(prob, fault=None)   the kernel's arithmetic in plain float32 torch, in the kernel's formulation (token positions and
                   region codes from index arithmetic), with single faults switched in
  evaluate(prob, res)         every assertion, on all elements; used unchanged on the emulation (CPU) and on the device results
"""
import math
from collections import namedtuple

import numpy as np
import torch

HD = 32
SCALE = HD ** -0.5
FLUSH = 2.0 ** -126         # the smallest normal float32
FAULTS = ("roll", "region_edge", "bias_transposed", "bias_next_head", "mask_zero", "drop_last_token")

Case = namedtuple("Case", "B Hp Wp heads ws shift")
CASES = [
    Case(2, 14, 21, 3, 7, 0),       # 49 = 3 * 16 + 1 token tail, 2 x 3 window grid, odd head count
    Case(2, 14, 21, 3, 7, 3),       # all nine mask regions occur
    Case(1, 7, 7, 1, 7, 3),         # one window: Hp - ws = 0, the roll wraps the whole map
    Case(2, 24, 36, 4, 12, 0),      # 144 tokens = nine full tiles
    Case(2, 24, 36, 4, 12, 6),      # 144 tokens, shifted
    Case(1, 12, 12, 2, 12, 6),      # 144 tokens, one window
    Case(1, 16, 8, 1, 8, 4),        # 64 tokens, no tail
    Case(1, 6, 9, 2, 3, 1),         # 9 tokens, less than one tile
]
CASE_IDS = ["B%d_%dx%d_h%d_ws%d_s%d" % c for c in CASES]


def _grid(rng, shape, lim, step=0.125):
    n = int(round(lim / step))
    return torch.from_numpy(rng.randint(-n, n + 1, size=shape).astype(np.float32) * step)


def build(case):
    """-> dict: qkv [B, Hp, Wp, 3 C], dout [B, Hp, Wp, C] (float32 holding bf16-representable values), table [(2 ws - 1)^2, heads]
    (float32): q, k ~ U(-2, 2), v, dout ~ U(-1, 1), table ~ U(-2, 2), on a grid of 1 / 8"""
    rng = np.random.RandomState(2000 + CASES.index(case))
    B, Hp, Wp, heads, ws, shift = case
    C = heads * HD
    qkv = torch.cat([_grid(rng, (B, Hp, Wp, 2 * C), 2.0), _grid(rng, (B, Hp, Wp, C), 1.0)], -1)
    dout = _grid(rng, (B, Hp, Wp, C), 1.0)
    table = _grid(rng, ((2 * ws - 1) ** 2, heads), 2.0)
    for t in (qkv, dout, table):
        assert torch.equal(t, t.bfloat16().float())
    return dict(case=case, qkv=qkv, dout=dout, table=table)


# ---- the reference's formulation (fp64) ---------------------------------------------------------------------------------------------
def _to_windows(x, ws, shift):
    """[B, Hp, Wp, ch] un-rolled -> [B, nW, ws^2, ch] rolled and partitioned"""
    B, Hp, Wp, ch = x.shape
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    return x.view(B, Hp // ws, ws, Wp // ws, ws, ch).permute(0, 1, 3, 2, 4, 5).reshape(B, -1, ws * ws, ch)


def _from_windows(x, ws, shift, Hp, Wp):
    B, _, _, ch = x.shape
    x = x.view(B, Hp // ws, Wp // ws, ws, ws, ch).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, ch)
    return torch.roll(x, shifts=(shift, shift), dims=(1, 2)) if shift else x


def _heads(x, heads):
    """[B, nW, N, heads * 32] -> [B, nW, heads, N, 32]"""
    B, nW, N, _ = x.shape
    return x.view(B, nW, N, heads, HD).permute(0, 1, 3, 2, 4)


def _unheads(x):
    B, nW, heads, N, _ = x.shape
    return x.permute(0, 1, 3, 2, 4).reshape(B, nW, N, heads * HD)


def index_buffer(ws):
    """the relative_position_index buffer, built as the reference builds it (differences of a coordinate grid)"""
    coords = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = (coords[:, :, None] - coords[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def slice_mask(Hp, Wp, ws, shift):
    """[nW, N, N] additive mask built as the reference builds it (region numbers painted through slices)"""
    img = torch.zeros(1, Hp, Wp, 1, dtype=torch.float64)
    cnt = 0
    for h in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
        for w in (slice(0, -ws), slice(-ws, -shift), slice(-shift, None)):
            img[:, h, w, :] = cnt
            cnt += 1
    mw = _to_windows(img, ws, 0)[0, :, :, 0]
    d = mw[:, None, :] - mw[:, :, None]
    return torch.where(d != 0, torch.full_like(d, -100.0), torch.zeros_like(d))


def reference(prob):
    """fp64 results in un-rolled coordinates (out [B, Hp, Wp, C], dqkv [B, Hp, Wp, 3 C], dtable) and `bound`, per element: the
    first-order rounding model of _attn_cases.reference (P and dS rounded to bf16 once, delta formed from the bf16-rounded output,
    results rounded to bf16).  One term that model does not need: a pair 100 below its row's maximum has a probability under the
    smallest normal fp32 number, which float32 may flush to zero, so every probability carries an absolute error of FLUSH = 2^-126
    (it matters only where a token is alone in its region and the exact result is itself ~e^-100).  Table gradient: every
    contributing (window, i, j) adds that model's dS error (without the scale factor, which the bias does not carry), and an fp32
    sum of n terms adds at most n 2^-24 sum |dS|."""
    B, Hp, Wp, heads, ws, shift = prob["case"]
    C = heads * HD
    qkv, dout, table = prob["qkv"].double(), prob["dout"].double(), prob["table"].double()
    q, k, v = (_heads(_to_windows(qkv[..., i * C:(i + 1) * C], ws, shift), heads) for i in range(3))
    dO = _heads(_to_windows(dout, ws, shift), heads)
    N = ws * ws
    idx = index_buffer(ws)
    bias = table[idx.view(-1)].view(N, N, heads).permute(2, 0, 1)
    s = SCALE * (q @ k.transpose(-1, -2)) + bias
    if shift:
        s = s + slice_mask(Hp, Wp, ws, shift)[None, :, None]
    p = torch.softmax(s, -1)
    out = p @ v
    dP = dO @ v.transpose(-1, -2)
    delta = (dO * out).sum(-1, keepdim=True)
    dS_raw = p * (dP - delta)
    dS = SCALE * dS_raw
    dq, dk, dv = dS @ k, dS.transpose(-1, -2) @ q, p.transpose(-1, -2) @ dO
    derr = p * (2.0 ** -9 * (dO.abs() * out.abs()).sum(-1, keepdim=True))
    derr = derr + FLUSH * (dP - delta).abs()
    err = 2.0 ** -9 * dS.abs() + SCALE * derr
    err_raw = 2.0 ** -9 * dS_raw.abs() + derr
    per_pair = dS_raw.sum((0, 1)).permute(1, 2, 0).reshape(N * N, heads)                # [N * N, heads]
    dtable = torch.zeros_like(table).index_add_(0, idx.view(-1), per_pair)
    n_terms = B * (Hp // ws) * (Wp // ws) * N
    tb_pair = (err_raw + n_terms * 2.0 ** -24 * dS_raw.abs()).sum((0, 1)).permute(1, 2, 0).reshape(N * N, heads)
    b_table = torch.zeros_like(table).index_add_(0, idx.view(-1), tb_pair)

    def back(x):
        return _from_windows(_unheads(x), ws, shift, Hp, Wp)
    ref = dict(out=back(out), dqkv=torch.cat([back(dq), back(dk), back(dv)], -1), dtable=dtable)
    ref["bound"] = dict(
        out=back(2.0 ** -8 * (p @ v.abs() + out.abs()) + FLUSH * v.abs().sum(-2, keepdim=True)),
        dqkv=torch.cat([back(2.0 * (err @ k.abs() + 2.0 ** -9 * dq.abs())),
                        back(2.0 * (err.transpose(-1, -2) @ q.abs() + 2.0 ** -9 * dk.abs())),
                        back(2.0 ** -8 * (p.transpose(-1, -2) @ dO.abs() + dv.abs()) + FLUSH * dO.abs().sum(-2, keepdim=True))], -1),
        dtable=b_table)
    return ref


# ---- the kernel's formulation (float32) -----------------------------------------------------------------------------------------------
def token_geometry(case, roll=None, region_edge=0):
    """-> pos [nW, N] (flat position in the un-rolled Hp x Wp map), code [N] (in-window row (2 ws - 1) + col), region [nW, N]:
    the closed forms the kernel indexes with.  roll: the shift the loads use; region_edge: added to Hp - ws / Wp - ws"""
    B, Hp, Wp, heads, ws, shift = case
    roll = shift if roll is None else roll
    w = torch.arange((Hp // ws) * (Wp // ws))
    i = torch.arange(ws * ws)
    r = (w // (Wp // ws))[:, None] * ws + (i // ws)[None, :]
    c = (w % (Wp // ws))[:, None] * ws + (i % ws)[None, :]
    pos = ((r + roll) % Hp) * Wp + (c + roll) % Wp
    code = (i // ws) * (2 * ws - 1) + i % ws
    if shift:
        rh = (r >= Hp - ws + region_edge).long() + (r >= Hp - shift).long()
        rc = (c >= Wp - ws + region_edge).long() + (c >= Wp - shift).long()
        region = 3 * rh + rc
    else:
        region = torch.zeros_like(r)
    return pos, code, region


def fault_applies(prob, fault):
    """whether a single fault can change a result of this problem at all, from the case data"""
    B, Hp, Wp, heads, ws, shift = prob["case"]
    if fault in ("roll", "region_edge", "mask_zero"):
        return shift > 0                    # an unshifted block rolls by 0 and has no mask
    if fault == "bias_next_head":
        return heads > 1                    # one head has no next column
    if fault in ("bias_transposed", "drop_last_token"):
        return ws * ws > 1
    raise ValueError(fault)


def _bf(x):
    return x.bfloat16().float()


def emulate(prob, fault=None):
    """-> dict out [B, Hp, Wp, C], dqkv [B, Hp, Wp, 3 C] (bf16), dtable (float32): the forward and backward kernels of
    csrc/win_attn.hip in float32 torch.  fault: one of FAULTS — a single wrong index or constant of the kind the kernel can have."""
    case = prob["case"]
    B, Hp, Wp, heads, ws, shift = case
    C, N = heads * HD, ws * ws
    pos, code, region = token_geometry(case, roll=shift - 1 if fault == "roll" and shift else None,
                                       region_edge=1 if fault == "region_edge" else 0)
    nW = pos.shape[0]
    flat = prob["qkv"].view(B, Hp * Wp, 3 * C)
    win = flat[:, pos.view(-1)].view(B, nW, N, 3, heads, HD).permute(3, 0, 1, 4, 2, 5)              # [3, B, nW, heads, N, 32]
    q, k, v = win[0], win[1], win[2]
    dO = prob["dout"].view(B, Hp * Wp, C)[:, pos.view(-1)].view(B, nW, N, heads, HD).permute(0, 1, 3, 2, 4)
    off = (ws - 1) * 2 * ws
    idx = code[:, None] - code[None, :] + off                                                       # [query, key]
    if fault == "bias_transposed":
        idx = idx.t()
    table = prob["table"]
    if fault == "bias_next_head":
        table = table[:, (torch.arange(heads) + 1) % heads]
    bias = table[idx.reshape(-1)].view(N, N, heads).permute(2, 0, 1)
    scale = torch.tensor(SCALE, dtype=torch.float32)
    S = (q @ k.transpose(-1, -2)) * scale + bias
    differ = region[:, :, None] != region[:, None, :]                                               # [nW, N, N]
    S = S + (differ.float() * (0.0 if fault == "mask_zero" else -100.0))[None, :, None]
    if fault == "drop_last_token":
        S[..., N - 1] = -math.inf
    mx = S.amax(-1, keepdim=True)
    e = torch.exp(S - mx)
    l = e.sum(-1, keepdim=True)
    out = _bf((_bf(e) @ v) / l)
    lse = mx + torch.log(l)
    p = torch.exp(S - lse)
    delta = (dO * out).sum(-1, keepdim=True)
    ds = p * ((dO @ v.transpose(-1, -2)) - delta)
    dsb = _bf(ds * scale)
    dq, dk, dv = _bf(dsb @ k), _bf(dsb.transpose(-1, -2) @ q), _bf(_bf(p).transpose(-1, -2) @ dO)
    dtable = torch.zeros_like(prob["table"]).index_add_(0, idx.reshape(-1), ds.sum((0, 1)).permute(1, 2, 0).reshape(N * N, heads))
    if fault == "bias_next_head":
        dtable = dtable[:, (torch.arange(heads) - 1) % heads]

    def scatter(x, ch):                                                                             # [B, nW, heads, N, 32] -> map
        o = torch.zeros(B, Hp * Wp, ch)
        o[:, pos.view(-1)] = x.permute(0, 1, 3, 2, 4).reshape(B, nW * N, ch)
        return o.view(B, Hp, Wp, ch)
    return dict(out=scatter(out, C).bfloat16(), dqkv=torch.cat([scatter(t, C) for t in (dq, dk, dv)], -1).bfloat16(), dtable=dtable)


# ---- the assertions -------------------------------------------------------------------------------------------------------------------
def evaluate(prob, res, ref=None):
    """Every element of out, of the three thirds of dqkv and of dtable against `reference` -> {tensor: worst err / bound};
    raises AssertionError naming the first tensor that leaves its bound."""
    case = prob["case"]
    C = case.heads * HD
    ref = ref or reference(prob)
    assert res["out"].dtype == torch.bfloat16 and res["dqkv"].dtype == torch.bfloat16 and res["dtable"].dtype == torch.float32
    ratios = {}
    parts = [("out", res["out"], ref["out"], ref["bound"]["out"])]
    for i, name in enumerate(("dq", "dk", "dv")):
        sl = slice(i * C, (i + 1) * C)
        parts.append((name, res["dqkv"][..., sl], ref["dqkv"][..., sl], ref["bound"]["dqkv"][..., sl]))
    parts.append(("dtable", res["dtable"], ref["dtable"], ref["bound"]["dtable"]))
    for name, got, want, bound in parts:
        assert got.shape == want.shape, f"{case}: {name} has shape {tuple(got.shape)}"
        assert torch.isfinite(got.float()).all(), f"{case}: {name} not finite"
        err = (got.double() - want).abs()
        bad = err > bound
        ratios[name] = float((err / bound.clamp_min(1e-300)).max())
        assert not bad.any(), f"{case}: {name} leaves its bound at {int(bad.sum())} of {bad.numel()} elements " \
                              f"(worst err / bound {ratios[name]:.3g})"
    return ratios
