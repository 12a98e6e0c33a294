"""Key-exact attention problems for csrc/attn.hip: sparse masks in which every open key carries O(1) weight, so that a key dropped
at a tail, counted twice at a split boundary or masked one byte off REPLACES a result instead of nudging it by 1 / (open keys).

  CASES            the case table (explicit rows); `split_of` gives the wave / workgroup geometry the kernels index with
  build(case)      bf16-representable q, k, v, dO and a boolean mask: boundary keys of the case's split opened by the covering rows,
                   masked decoys (score >= 20 above every open key, |v| ~ 2^20) around them and at the clamped-load positions
  reference(prob)  fp64 softmax attention and its gradients on the same inputs, with the per-element bounds of the kernels'
                   first-order rounding model
  emulate(prob, fault=...)   plain torch emulation of the kernels' arithmetic (32-key steps, running max, bf16 P in the numerator,
                   LDS merge, combine), with single faults switched in: tests/test_attn_keys_cpu.py proves the assertions sharp
  evaluate(prob, res)        every assertion of the two families; used unchanged on the emulation (CPU) and on the device results
"""
import math
from collections import namedtuple

import numpy as np
import torch

H, HD, E = 8, 32, 256
SCALE = HD ** -0.5
RES = HD - 1               # the reserved dim of every head: constant in q, nonzero in decoy keys only
Q_RES = 4.0
GAP = 20.0                 # decoy score - open score, at least
COVER_ROWS = (0, 15, 16, 31, 32)          # and Lq - 1
OFFSETS = (1, 4, 8, 16, 32)               # and kpw
FAULTS = ("drop_last", "admit_after", "mask_shift", "double", "skip_last_wg", "admit_decoy_kv")

# family: selector (one open key per row, each key opened once) | few (2-4 open keys per row) | few_scaled (q x 4: open scores up
# to ~30 apart) | nomask | fullmask (few, rows 0, 16 and Lq - 1 fully masked).  mask: image [N, Lq, Lk] | shared [Lq, Lk] | none.
# kpw / nw: the attn_kpw / attn_nw options (0 / 8 = the library's policy); kpw_eff: the keys per wave the policy is documented to
# choose for a default row (csrc/attn.hip: 64 up to 256 keys, 128 beyond, at these query counts) — the GPU test checks `wg`, the
# workgroup splits this implies, against the library's own workspace size.  odd: the mask is a view at an odd byte offset.
Case = namedtuple("Case", "name family Lq Lk N mask kpw nw kpw_eff wg odd")
CASES = [
    # forced splits
    Case("one_wave_63", "few", 33, 63, 1, "image", 64, 1, 64, 1, False),                # one wave, unaligned
    Case("one_wave_lq1", "few", 1, 64, 2, "image", 64, 8, 64, 1, False),                # Lq = 1, one aligned wave
    Case("two_waves_65", "few_scaled", 64, 65, 2, "shared", 64, 8, 64, 1, False),       # the second wave holds one key
    Case("five_waves_sel", "selector", 64, 257, 2, "image", 64, 8, 64, 1, False),       # several waves in one workgroup
    Case("wg3_empty_sel", "selector", 81, 453, 2, "image", 64, 3, 64, 3, False),        # 8 waves in 3 workgroups: one empty slot
    Case("wg3_empty_few", "few_scaled", 81, 453, 1, "shared", 64, 3, 64, 3, False),
    Case("wg10_sel", "selector", 33, 600, 1, "image", 64, 1, 64, 10, False),            # > 8 workgroups: combine loop, sum loop
    Case("wg10_few", "few_scaled", 81, 600, 2, "shared", 64, 1, 64, 10, False),
    Case("wg4_odd_mask", "selector", 81, 600, 2, "image", 64, 3, 64, 4, True),          # Lk % 8 == 0, mask at an odd address
    Case("kpw512_few", "few", 64, 1032, 2, "image", 512, 8, 512, 1, False),             # kpw 512: three waves, 8-key last wave
    Case("kpw512_wg2_sel", "selector", 81, 1100, 1, "shared", 512, 2, 512, 2, False),   # ... two workgroups, one empty slot
    # the library's own policy
    Case("dflt_1100_sel", "selector", 81, 1100, 2, "image", 0, 8, 128, 2, False),       # 9 waves: seven empty in workgroup 1
    Case("dflt_1100_few", "few_scaled", 33, 1100, 1, "shared", 0, 8, 128, 2, False),
    Case("dflt_257_sel", "selector", 64, 257, 1, "shared", 0, 8, 128, 1, False),        # the last wave holds one key, unaligned
    Case("dflt_1032_few", "few", 33, 1032, 2, "image", 0, 8, 128, 2, False),            # aligned 8-key tail in workgroup 1
    Case("dflt_8_sel", "selector", 1, 8, 2, "image", 0, 8, 64, 1, False),
    # no mask
    Case("nomask_1", "nomask", 1, 1, 1, "none", 0, 8, 64, 1, False),
    Case("nomask_3", "nomask", 33, 3, 2, "none", 0, 8, 64, 1, False),
    Case("nomask_8", "nomask", 64, 8, 1, "none", 0, 8, 64, 1, False),
    Case("nomask_9", "nomask", 81, 9, 2, "none", 0, 8, 64, 1, False),
    # fully masked rows
    Case("full_one_wg", "fullmask", 33, 257, 2, "image", 0, 8, 128, 1, False),
    Case("full_wg10", "fullmask", 81, 600, 1, "shared", 64, 1, 64, 10, False),
]
CASE_IDS = [c.name for c in CASES]


def split_of(case):
    """(kpw, nw, wg, [(kb0, kb1)] per wave slot) as the kernels index them: slot w of workgroup g starts at (g nw + w) kpw"""
    kpw = case.kpw_eff
    waves = -(-case.Lk // kpw)
    nw = min(waves, case.nw)
    wg = -(-waves // nw)
    ranges = []
    for s in range(wg * nw):
        kb0 = min(case.Lk, s * kpw)
        ranges.append((kb0, min(case.Lk, kb0 + kpw)))
    return kpw, nw, wg, ranges


def boundary_keys(case):
    """the keys at which a split, tail or block edge of this case can go wrong (ISSUE: boundary set)"""
    kpw, nw, _, _ = split_of(case)
    Lk = case.Lk
    waves = -(-Lk // kpw)
    b = (Lk - 1) // 32
    ks = [Lk - 1, 0, kpw - 1, kpw, nw * kpw - 1, nw * kpw, (waves - 1) * kpw, Lk - 8, Lk - 9, Lk - 2,
          7, 8, 31, 32, 63, 64, 32 * b - 1, 32 * b]
    out = []                            # (in the order in which a problem with too few rows for all of them takes them)
    for k in ks:
        if 0 <= k < Lk and k not in out:
            out.append(k)
    return out


def clamp_keys(case):
    """where a clamped load past a range's end falls back to"""
    _, _, _, ranges = split_of(case)
    ks = {kb1 - 1 for kb0, kb1 in ranges if kb1 > kb0} | {case.Lk - 1, case.Lk - 8}
    return sorted(k for k in ks if 0 <= k < case.Lk)


def full_rows(case):
    return sorted({0, 16, case.Lq - 1}) if case.family == "fullmask" else []


def cover_rows(case):
    rows = [r for r in COVER_ROWS if r < case.Lq] + [case.Lq - 1]
    out = []
    for r in rows:
        if r not in out and r not in full_rows(case):
            out.append(r)
    return out


def _bf16_grid(rng, shape, step=0.125, lim=2.0):
    n = int(round(lim / step))
    return torch.from_numpy(rng.randint(-n, n + 1, size=shape).astype(np.float32) * step)


def build(case):
    """-> dict: q, k, v, dO (float32 holding bf16-representable values, [L, N, 256]), mask (bool, or None), open (list per image of
    list per row of open keys), decoys, boundary; everything on the CPU"""
    rng = np.random.RandomState(1000 + CASES.index(case))
    Lq, Lk, N = case.Lq, case.Lk, case.N
    kpw, nw, wg, ranges = split_of(case)
    q = _bf16_grid(rng, (Lq, N, E))
    k = _bf16_grid(rng, (Lk, N, E))
    v = _bf16_grid(rng, (Lk, N, E))
    dO = _bf16_grid(rng, (Lq, N, E))
    prob = dict(case=case, boundary=boundary_keys(case), decoys=[], open=None, mask=None)
    if case.family == "few_scaled":
        q = q * 4.0
    if case.mask != "none":
        B = prob["boundary"]
        per_row = 1 if case.family == "selector" else 4
        live = [r for r in range(Lq) if r not in full_rows(case)]
        order = cover_rows(case) + [r for r in live if r not in cover_rows(case)]
        imgs = N if case.mask == "image" else 1
        # the boundary keys that get opened: all of them where the rows suffice, else the first ones.  Each row's first key is a
        # boundary key, the covering rows served first (per image another rotation, so that the images differ)
        opened = set(B[:imgs * len(order) * per_row])
        first = []
        for im in range(imgs):
            if len(order) >= len(B):
                rot = B if im % 2 == 0 else B[::-1]
            else:
                sh = (im * len(order)) % len(B)
                rot = B[sh:] + B[:sh]
            if case.family == "selector":
                first.append({r: rot[i] for i, r in enumerate(order[:len(rot)])})
            else:
                first.append({r: rot[i % len(rot)] for i, r in enumerate(order)})
        assert {kk for f in first for kk in f.values()} <= opened
        todo = [b_ for b_ in B if b_ in opened and not any(b_ in f.values() for f in first)]     # ... the rows' further keys take these
        # decoys: around the boundary keys and at the clamp positions, wherever no row opens the key
        dec = set()
        for b_ in B:
            for off in OFFSETS + (kpw,):
                dec |= {b_ - off, b_ + off}
        dec |= set(clamp_keys(case))
        dec = sorted(kk for kk in dec if 0 <= kk < Lk and kk not in opened)
        free = [kk for kk in range(Lk) if kk not in opened and kk not in dec]
        wave_of = lambda kk: kk // kpw
        open_ = []
        for im in range(imgs):
            rows = [[] for _ in range(Lq)]
            if case.family == "selector":
                pool = [kk for kk in free]
                rng.shuffle(pool)
                assert len(pool) >= len(order) - len(first[im]), "not enough free keys for a selector problem"
                for r in order:
                    rows[r] = [first[im][r]] if r in first[im] else [pool.pop()]
            else:
                pool = sorted(opened | set(free))
                for i, r in enumerate(order):
                    ks = [first[im][r]]
                    want = 2 + (i % 3)                                      # 2, 3 or 4 open keys
                    same = (i % 3 == 1)                                     # a row whose keys all lie in one wave's range
                    while len(ks) < want:
                        cand = [kk for kk in pool if kk not in ks and ((wave_of(kk) == wave_of(ks[0])) if same
                                                                     else all(wave_of(kk) != wave_of(x) for x in ks))]
                        if not cand:
                            cand = [kk for kk in pool if kk not in ks]
                        if not cand:
                            break
                        pref = [kk for kk in cand if kk in todo]
                        pick = pref[0] if pref else cand[rng.randint(len(cand))]
                        if pick in todo:
                            todo.remove(pick)
                        ks.append(pick)
                    rows[r] = sorted(ks)
            open_.append(rows)
        if case.family != "selector":
            for b_ in list(todo):               # boundary keys that the wave rules above left over: any row with room
                row = next(rows[r] for rows in open_ for r in order if len(rows[r]) < 4 and b_ not in rows[r])
                row.append(b_)
                row.sort()
                todo.remove(b_)
        mask = torch.ones(imgs, Lq, Lk, dtype=torch.bool)
        for im in range(imgs):
            for r in range(Lq):
                mask[im, r, open_[im][r]] = False
        prob["mask"] = mask if case.mask == "image" else mask[0]
        prob["open"] = open_ if case.mask == "image" else open_ * N
        prob["decoys"] = dec
        # the reserved dim: constant in q, zero in every key but the decoys, where it lifts the score GAP above every open score
        for h in range(H):
            q[:, :, h * HD + RES] = Q_RES
            k[:, :, h * HD + RES] = 0.0
        if dec:
            s = scores64(q, k)                                             # [N, H, Lq, Lk], decoys without their lift yet
            m3 = mask if case.mask == "image" else mask[0].expand(N, Lq, Lk)
            top_open = s.masked_fill(m3[:, None], -math.inf).amax()
            low_dec = s[..., dec].amin()
            need = (GAP + float(top_open) - float(low_dec)) / (SCALE * Q_RES)
            lift = 2.0 ** math.ceil(math.log2(max(need, 1.0)))
            sign = torch.from_numpy(rng.choice([-1.0, 1.0], size=(len(dec), N, E)).astype(np.float32))
            v[dec] = sign * 2.0 ** 20 * (1.0 + _bf16_grid(rng, (len(dec), N, E)).abs() / 4.0)
            for h in range(H):
                k[dec, :, h * HD + RES] = lift
    for t in (q, k, v, dO):
        assert torch.equal(t, t.bfloat16().float()) and torch.isfinite(t).all()
    prob.update(q=q, k=k, v=v, dO=dO)
    return prob


def heads(t):
    """[L, N, 256] -> [N, H, L, 32]"""
    L, N, _ = t.shape
    return t.reshape(L, N, H, HD).permute(1, 2, 0, 3)


def unheads(t):
    """[N, H, L, 32] -> [L, N, 256]"""
    N, _, L, _ = t.shape
    return t.permute(2, 0, 1, 3).reshape(L, N, E)


def scores64(q, k):
    return SCALE * torch.matmul(heads(q.double()), heads(k.double()).transpose(-1, -2))


def mask4(prob):
    """the mask as [N or 1, 1, Lq, Lk], or None"""
    m = prob["mask"]
    if m is None:
        return None
    return m[:, None] if m.dim() == 3 else m[None, None]


def reference(prob):
    """fp64 results and the per-element bounds of the first-order rounding model (P and dS rounded to bf16 once, delta formed from
    the bf16-rounded output, results rounded to bf16).  Fully masked rows: zeros, lse = -inf."""
    q, k, v, dO = (heads(prob[n].double()) for n in ("q", "k", "v", "dO"))
    s = SCALE * torch.matmul(q, k.transpose(-1, -2))
    m = mask4(prob)
    if m is not None:
        s = s.masked_fill(m, -math.inf)
    full = torch.isinf(s).all(-1)                                         # [N, H, Lq]
    lse = torch.logsumexp(s.masked_fill(full[..., None], 0.0), -1).masked_fill(full, -math.inf)
    p = torch.exp(s - lse.masked_fill(full, 0.0)[..., None]).masked_fill(full[..., None], 0.0)
    out = p @ v
    dP = dO @ v.transpose(-1, -2)
    delta = (dO * out).sum(-1, keepdim=True)
    dS = SCALE * p * (dP - delta)
    dq, dk, dv = dS @ k, dS.transpose(-1, -2) @ q, p.transpose(-1, -2) @ dO
    err = 2.0 ** -9 * dS.abs() + p * (2.0 ** -9 * SCALE * (dO.abs() * out.abs()).sum(-1, keepdim=True))
    ref = dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, p=p, full=full)
    ref["bound"] = dict(
        out=2.0 ** -8 * (p @ v.abs() + out.abs()),
        dv=2.0 ** -8 * (p.transpose(-1, -2) @ dO.abs() + dv.abs()),
        dq=2.0 * (err @ k.abs() + 2.0 ** -9 * dq.abs()),
        dk=2.0 * (err.transpose(-1, -2) @ q.abs() + 2.0 ** -9 * dk.abs()))
    return ref


# ---- the kernels' arithmetic in plain torch ---------------------------------------------------------------------------------------
def _bf(x):
    return x.bfloat16().float()


def fault_applies(prob, fault):
    """whether a single fault can change a result of this problem at all, from the builder's own data"""
    case = prob["case"]
    _, _, wg, ranges = split_of(case)
    live = [(a, b) for a, b in ranges if b > a]
    if case.mask == "none":
        opened = set(range(case.Lk))
    else:
        opened = {kk for rows in prob["open"] for ks in rows for kk in ks}
    if fault == "drop_last":
        return any(b - 1 in opened for _, b in live)
    if fault == "admit_after":
        return any(min(b, case.Lk - 1) in opened for _, b in live)
    if fault == "mask_shift":
        return case.mask != "none"
    if fault == "double":
        return min(split_of(case)[0], case.Lk - 1) in opened
    if fault == "skip_last_wg":
        return wg > 1
    if fault == "admit_decoy_kv":
        return bool(prob["decoys"])
    raise ValueError(fault)


def emulate(prob, fault=None):
    """-> dict out, dq [Lq, N, 256], dk, dv [Lk, N, 256] (bf16), lse [N, H, Lq] (float32): the forward, dQ and dK / dV kernels of
    csrc/attn.hip for the case's split in float32 torch.  fault: one of FAULTS — a single wrong index of the kind the split code
    can have (forward and dQ kernels: the first five; dK / dV kernel: the last)."""
    case = prob["case"]
    Lq, Lk, N = case.Lq, case.Lk, case.N
    kpw, nw, wg, ranges = split_of(case)
    q, k, v, dO = (heads(prob[n]) for n in ("q", "k", "v", "dO"))
    scale = torch.tensor(SCALE, dtype=torch.float32)
    S = torch.matmul(q, k.transpose(-1, -2)) * scale                       # [N, H, Lq, Lk]
    m = mask4(prob)
    mult = torch.ones(Lk)                                                   # how often the forward / dQ kernels count a key
    if fault == "mask_shift" and m is not None:
        m = m[..., torch.arange(1, Lk + 1).clamp(max=Lk - 1)]
    if fault == "drop_last":
        for a, b in ranges:
            if b > a:
                mult[b - 1] = 0.0
    if fault == "admit_after":
        for a, b in ranges:
            if b > a:
                mult[min(b, Lk - 1)] += 1.0
    if fault == "double":
        mult[min(kpw, Lk - 1)] = 2.0
    Sm = S if m is None else S.masked_fill(m, -math.inf)
    ninf = torch.tensor(-math.inf)

    def merge(parts):
        M = torch.stack([p_[0] for p_ in parts]).amax(0)
        L, O = torch.zeros_like(M), torch.zeros(N, H, Lq, HD)
        for ms, ls, os_ in parts:
            w = torch.where(ms == ninf, torch.zeros_like(ms), torch.exp(ms - torch.where(M == ninf, torch.zeros_like(M), M)))
            L, O = L + w * ls, O + w[..., None] * os_
        return M, L, O

    partials = []
    for g in range(wg):
        parts = []
        for w in range(nw):
            kb0, kb1 = ranges[g * nw + w]
            mx = torch.full((N, H, Lq), -math.inf)
            l, o = torch.zeros(N, H, Lq), torch.zeros(N, H, Lq, HD)
            for kk in range(kb0, kb1, 32):
                ke = min(kk + 32, kb1)
                s = Sm[..., kk:ke]
                mn = torch.maximum(mx, s.amax(-1))
                dead = mn == ninf
                base = torch.where(dead, torch.zeros_like(mn), mn)
                alpha = torch.where(dead, torch.ones_like(mn), torch.exp(mx - base))
                e = torch.where(dead[..., None], torch.zeros_like(s), torch.exp(s - base[..., None])) * mult[kk:ke]
                l = l * alpha + e.sum(-1)
                o = o * alpha[..., None] + _bf(e) @ v[:, :, kk:ke]
                mx = mn
            parts.append((mx, l, o))
        partials.append(merge(parts))
    if fault == "skip_last_wg" and wg > 1:
        partials = partials[:-1]
    M, L, O = merge(partials)
    pos = L > 0
    out = _bf(torch.where(pos[..., None], O / torch.where(pos, L, torch.ones_like(L))[..., None], torch.zeros_like(O)))
    lse = torch.where(pos, M + torch.log(torch.where(pos, L, torch.ones_like(L))), ninf)

    # backward: P recomputed from the saved lse; delta from the bf16 output
    delta = (dO * out).sum(-1, keepdim=True)
    dP = dO @ v.transpose(-1, -2)
    lse_ = torch.where(lse == ninf, torch.zeros_like(lse), lse)[..., None]

    def probs(Smask):
        return torch.where((lse == ninf)[..., None] | torch.isinf(Smask), torch.zeros_like(S), torch.exp(Smask - lse_))
    pr = probs(Sm)
    mq = mult.clone()
    if fault == "skip_last_wg" and wg > 1:
        mq[ranges[(wg - 1) * nw][0]:] = 0.0
    dq = (_bf(pr * (dP - delta) * scale) * mq) @ k
    mkv = m
    if fault == "admit_decoy_kv" and prob["decoys"]:
        mkv = m.clone()
        mkv[..., prob["decoys"][len(prob["decoys"]) // 2]] = False
    prk = probs(S if mkv is None else S.masked_fill(mkv, -math.inf))
    dv = _bf(prk).transpose(-1, -2) @ dO
    dk = _bf(prk * (dP - delta) * scale).transpose(-1, -2) @ q
    return dict(out=unheads(out).bfloat16(), lse=lse, dq=unheads(dq).bfloat16(), dk=unheads(dk).bfloat16(),
                dv=unheads(dv).bfloat16())


# ---- the assertions ---------------------------------------------------------------------------------------------------------------
def _ratio(err, bound):
    r = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, math.inf))
    return float(torch.where(err == 0, torch.zeros_like(r), r).max())


def _bits(t):
    return t.contiguous().view(torch.int16)


def evaluate(prob, res, ref=None):
    """Every assertion of the case's family on results `res` (out, lse, dq, dk, dv as the kernels write them, on the CPU).
    -> {tensor: worst err / bound}; raises AssertionError naming the first line that does not hold."""
    case = prob["case"]
    Lq, Lk, N = case.Lq, case.Lk, case.N
    ref = ref or reference(prob)
    full = ref["full"]
    for name in ("out", "dq", "dk", "dv"):
        assert res[name].dtype == torch.bfloat16 and torch.isfinite(res[name].float()).all(), f"{case.name}: {name} not finite"
    assert torch.isfinite(res["lse"][~full]).all(), f"{case.name}: lse not finite"
    ratios = {}
    if case.family == "selector":
        q, k, v, dO = (prob[n] for n in ("q", "k", "v", "dO"))
        key = torch.tensor([[prob["open"][n][i][0] for n in range(N)] for i in range(Lq)])           # [Lq, N]
        img = torch.arange(N)[None].expand(Lq, N)
        assert torch.equal(_bits(res["out"]), _bits(v[key, img].bfloat16())), f"{case.name}: out != v[key] bit for bit"
        s64 = scores64(q, k)                                                                         # [N, H, Lq, Lk]
        kk = key.t()[:, None, :, None].expand(N, H, Lq, 1)
        want = s64.gather(-1, kk)[..., 0]
        sabs = SCALE * torch.matmul(heads(q.double()).abs(), heads(k.double()).abs().transpose(-1, -2)).gather(-1, kk)[..., 0]
        err = (res["lse"].double() - want).abs()
        assert (err <= 2.0 ** -19 * sabs).all(), f"{case.name}: lse off by {float(err.max())} (a key counted twice moves it by log 2)"
        ratios["lse"] = _ratio(err, 2.0 ** -19 * sabs)
        assert torch.equal(_bits(res["dv"][key, img]), _bits(dO.bfloat16())), f"{case.name}: dv[key] != dO bit for bit"
        unopened = torch.ones(Lk, N, dtype=torch.bool)
        unopened[key, img] = False
        for name in ("dv", "dk"):
            assert (res[name][unopened].float() == 0).all(), f"{case.name}: {name} of a key no row opens is not zero"
        dot = SCALE * (heads(dO.double()).abs() * heads(v[key, img].double()).abs()).sum(-1, keepdim=True)   # [N, H, Lq, 1]
        bq = unheads(2.0 ** -18 * dot * heads(k[key, img].double()).abs().amax(-1, keepdim=True).expand(N, H, Lq, HD))
        bk = unheads(2.0 ** -18 * dot * heads(q.double()).abs().amax(-1, keepdim=True).expand(N, H, Lq, HD))
        for name, got, bound in (("dq", res["dq"], bq), ("dk", res["dk"][key, img], bk)):
            bound = bound * (1 + 2.0 ** -8)                                                          # then bf16 rounding
            assert (got.double().abs() <= bound).all(), f"{case.name}: {name} of a one-key row exceeds round-off"
            ratios[name] = _ratio(got.double().abs(), bound)
        return ratios
    if full.any():
        rows = full[:, 0]                                                                            # [N, Lq] (one mask for all heads)
        assert (res["out"].float().transpose(0, 1)[rows] == 0).all(), f"{case.name}: out of a fully masked row is not zero"
        assert (res["dq"].float().transpose(0, 1)[rows] == 0).all(), f"{case.name}: dq of a fully masked row is not zero"
        assert (res["lse"][full] == -math.inf).all(), f"{case.name}: lse of a fully masked row is not -inf"
    for name in ("out", "dq", "dk", "dv"):
        err = (heads(res[name].double()) - ref[name]).abs()
        bound = ref["bound"][name]
        ratios[name] = _ratio(err, bound)
        assert (err <= bound).all(), f"{case.name}: {name} err / bound = inf at {int((err > bound).sum())} elements " \
                                     f"(worst excess {float((err - bound).max())})"
    # lse (not in the few-keys table of bounds, which has no bf16 step on its path): the row maximum carries the selector family's
    # score bound, 2^-19 scale sum_d |q_d k_d| of the row's largest such key; L sums at most a few fp32 exponentials whose
    # arguments (<= ~64 in size) are off by <= 2^-24 * 64 * log2(e) relative, and the fast log adds a few ulp of a value <= ~64:
    # together <= 1.2e-5, held to 2^-15.  A key counted twice or dropped moves lse by log(1 + p_j).
    sabs = SCALE * torch.matmul(heads(prob["q"].double()).abs(), heads(prob["k"].double()).abs().transpose(-1, -2))
    m = mask4(prob)
    sabs = (sabs if m is None else sabs.masked_fill(m, 0.0)).amax(-1)
    lerr = (res["lse"].double() - ref["lse"])[~full].abs()
    lb = (2.0 ** -19 * sabs + 2.0 ** -15)[~full]
    ratios["lse"] = _ratio(lerr, lb)
    assert (lerr <= lb).all(), f"{case.name}: lse off by {float(lerr.max())}"
    return ratios
