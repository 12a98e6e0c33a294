"""The problems, fp64 reference, geometry mirrors and single-fault emulation of the clip matching cost from the factors
(csrc/mask_fused.hip: mpf_match_cost_fused_clip).  No GPU and no library is needed to import this file.
tests/test_mask_fused_clip_cases_cpu.py holds the case table to the branches it names, the mirrors to the built library and every
fault of the emulation to a failing check; tests/test_mask_fused_clip_gpu.py runs the same problems through the C ABI and the same
check function.

A group is (decoder output l, clip b).  Its map is F frames, each a channel-last [h * w, 256] plane, sampled at ONE point set; a
target row of ``tsamp`` is the tube's F * P samples, frame-major (mask2former_video/modeling/matcher.py:113-148).  Buffers carry
poison: the 64 elements behind every frame, the target rows before, between and behind the groups' ranges and every embedding row
that no group addresses are NaN, so a read outside the addressed set shows in the result.

Every entry t < t_count[g]: |got - ref| <= 2e-4 + 2e-4 |ref| with w_mask = w_dice = 5 (the bound of mpf_match_cost_fused and
mpf_match_cost_clip: the per-sample arithmetic is the image kernel's and both sums are means)."""
from types import SimpleNamespace

import numpy as np
import torch

import _loss_restate as LR
import _mask_fused_cases as MC

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
C, NAN, SENT = MC.C, MC.NAN, MC.SENT_GRAD
W_MASK, W_DICE = MC.W_MASK, MC.W_DICE
HW = (8, 12)
FRAME_GAP = 64


# ---- geometry mirrors (mc_geom with F frames and the workspace formula of csrc/mask_fused.hip) --------------------------------------
def mc_geom_clip(G, Q, P, F):
    """the F * ceil(P / 32) tiles of all frames, frame-major, dealt to the workgroups in runs of tiles_per_wg"""
    per_frame = (P + 31) // 32
    ntiles = F * per_frame
    qgroups = (Q + 127) // 128
    want = max(1, 512 // max(1, G * qgroups))
    tiles_per_wg = (ntiles + want - 1) // want
    nwg = (ntiles + tiles_per_wg - 1) // tiles_per_wg
    crossing = sum(1 for k in range(nwg) if (k * tiles_per_wg) // per_frame != (min((k + 1) * tiles_per_wg, ntiles) - 1) // per_frame)
    return SimpleNamespace(per_frame=per_frame, ntiles=ntiles, qgroups=qgroups, tiles_per_wg=tiles_per_wg, nwg=nwg, crossing=crossing)


def clip_workspace_bytes(G, Q, Tmax, P, F, tsamp_rows):
    if G <= 0 or Q <= 0 or Tmax <= 0 or P <= 0 or F <= 0 or tsamp_rows < 0 or F * P >= 2 ** 31:
        return 0
    m = mc_geom_clip(G, Q, P, F)
    return MC.align256(m.nwg * G * Q * Tmax * 2 * 4) + MC.align256(m.nwg * G * Q * 2 * 4) + MC.align256(tsamp_rows * 4)


# name -> F, L, N clips, Q, tubes per clip, P, and (TCH, qgroups, tiles per frame, tiles_per_wg, nwg, workgroups whose run of tiles
# crosses a frame boundary)
CLIP_CASES = {
    "K1": dict(F=1, L=2, N=3, Q=127, counts=(8, 0, 3), P=31, outside_group=3, geom=(4, 1, 1, 1, 1, 0)),           # the shape of C2
    "K2": dict(F=1, L=1, N=3, Q=129, counts=(17, 24, 1), P=33, geom=(12, 2, 2, 1, 2, 0)),                          # the shape of C4
    "K3": dict(F=2, L=2, N=3, Q=127, counts=(8, 0, 3), P=31, outside_group=3, geom=(4, 1, 1, 1, 2, 0)),
    "K4": dict(F=3, L=1, N=3, Q=129, counts=(17, 24, 1), P=33, geom=(12, 2, 2, 1, 6, 0)),
    "K5": dict(F=2, L=1, N=1, Q=1, counts=(1,), P=1, geom=(4, 1, 1, 1, 2, 0)),
    "K6": dict(F=2, L=2, N=2, Q=200, counts=(6, 2), P=4128, geom=(4, 2, 129, 5, 52, 1)),
    "K7": dict(F=5, L=1, N=4, Q=10, counts=(65, 128, 0, 127), P=100, geom=(64, 1, 4, 1, 20, 0)),
}


def planted_points(h, w):
    """y = 0, y = 1, just inside the last row (a footprint whose lower corners are row h: outside), the first row, and outside"""
    return torch.tensor([[0.3, 0.0], [0.6, 1.0], [0.4, (h - 0.25) / h], [0.7, 0.25 / h], [2.0, -1.0], [-1.0, 2.0],
                         [0.0, (h - 0.125) / h], [1.0, (h - 0.375) / h]])


def clip_problem(F, L, N, Q, counts, P, seed, hw=HW, outside_group=None, **_):
    """group g = l * N + b; its queries are rows l * Qt + 3 + q of clip b in the [L * Qt, N, 256] parent (Qt = Q + 3); its targets
    the tsamp rows t_first[g] .. + counts[b] of F * P floats"""
    h, w = hw
    g = torch.Generator().manual_seed(seed)
    G, Qt = L * N, Q + 3
    counts = np.asarray(counts, dtype=np.int64)
    Tmax = int(counts.max())
    group_clip = np.tile(np.arange(N), L).astype(np.int32)
    t_count = counts[group_clip].astype(np.int32)
    embed = torch.full((L * Qt, N, C), NAN, dtype=BF16)
    embed_first = np.zeros(G, dtype=np.int64)
    for gi in range(G):
        l, b = divmod(gi, N)
        embed_first[gi] = (l * Qt + 3) * N * C + b * C
        if t_count[gi] > 0:
            embed[l * Qt + 3:(l + 1) * Qt, b] = (torch.randn(Q, C, generator=g) * MC.EMBED_SCALE_COST).to(BF16)
    frame_stride = h * w * C + FRAME_GAP
    clip_stride = F * frame_stride
    feat = torch.full((N * clip_stride,), NAN, dtype=BF16)
    for b in range(N):
        if counts[b] > 0:
            for f in range(F):
                o = b * clip_stride + f * frame_stride
                feat[o:o + h * w * C] = torch.randn(h * w * C, generator=g).to(BF16)
    coords = torch.rand(G, P, 2, generator=g) * 1.2 - 0.1
    pl = planted_points(h, w)
    coords[:, :min(P, len(pl))] = pl[:min(P, len(pl))]
    if outside_group is not None:                                  # every footprint wholly outside the plane: logits exactly 0
        coords[outside_group, :, 0] = 1.3 + 0.2 * torch.rand(P, generator=g)
    masks = [torch.rand(int(c), F, *MC.GT_HW, generator=g) < 0.4 for c in counts]          # tubes [T, F, H, W]
    t_first = np.zeros(G, dtype=np.int32)
    rows, r = [torch.full((2, F * P), NAN)], 2
    for gi in range(G):
        t_first[gi] = r
        Tn = int(t_count[gi])
        if Tn > 0:
            m = masks[group_clip[gi]]
            rows.append(LR.point_sample(m.reshape(Tn * F, *MC.GT_HW), coords[gi:gi + 1]).reshape(Tn, F * P).to(F32))
        rows.append(torch.full((1, F * P), NAN))
        r += Tn + 1
    tsamp = torch.cat(rows)
    assert tsamp.shape[0] == r
    return SimpleNamespace(F=F, L=L, N=N, Q=Q, Qt=Qt, G=G, P=P, h=h, w=w, counts=counts, Tmax=Tmax, group_clip=group_clip,
                           t_first=t_first, t_count=t_count, embed=embed, embed_first=embed_first, row_stride=N * C, feat=feat,
                           clip_stride=clip_stride, frame_stride=frame_stride, coords=coords, masks=masks, tsamp=tsamp,
                           outside_group=outside_group)


def clip_case(name):
    return clip_problem(seed=4000 + int(name[1:]), **CLIP_CASES[name])


def group_embed(cp, gi):
    return cp.embed.view(-1)[cp.embed_first[gi]:].as_strided((cp.Q, C), (cp.row_stride, 1))


def frame_feat(cp, gi, f):
    o = int(cp.group_clip[gi]) * cp.clip_stride + f * cp.frame_stride
    return cp.feat[o:o + cp.h * cp.w * C].view(cp.h * cp.w, C)


def cost_ref(cp):
    """-> list over the groups of [Q, t_count[g]] fp64 (None for a group without tubes): the logits of every frame at the group's
    points, frame-major, then the cost of the F * P samples"""
    out = []
    for gi in range(cp.G):
        T0, Tn = int(cp.t_first[gi]), int(cp.t_count[gi])
        if not Tn:
            out.append(None)
            continue
        E = group_embed(cp, gi)
        x = torch.cat([MC.logits_ref(E, frame_feat(cp, gi, f), cp.coords[gi], cp.h, cp.w) for f in range(cp.F)], 1)
        out.append(LR.match_cost_samples(x, cp.tsamp[T0:T0 + Tn], W_MASK, W_DICE))
    return out


def check_cost(cp, cost, ref, what=""):
    """cost [G, Q, Tmax] fp32 that started as SENT"""
    cost = cost.cpu()
    for gi in range(cp.G):
        assert bool((cost[gi, :, int(cp.t_count[gi]):] == SENT).all()), f"group {gi}: entries t >= {cp.t_count[gi]} were written"
    live = [gi for gi in range(cp.G) if cp.t_count[gi] > 0]
    got = torch.cat([cost[gi, :, :int(cp.t_count[gi])].reshape(-1) for gi in live])
    want = torch.cat([ref[gi].reshape(-1) for gi in live])
    return MC.hold("match_cost_fused_kernel<clip>", f"cost {what}", got, want, MC.COST_ATOL + MC.COST_RTOL * want.abs())


# ---- emulation in the kernel's arithmetic, one fault at a time ------------------------------------------------------------------------
CLIP_FAULTS = ("prev_frame", "tsamp_frame", "divisor", "tail", "next_frame_corner")


def _emu_frame_logits(cp, gi, f, fault):
    """fp32 coordinates, weights and interpolation, the interpolated features as two bf16 planes, fp32 product -> [Q, P]"""
    h, w, P = cp.h, cp.w, cp.P
    one = torch.ones((), dtype=F32)
    c = cp.coords[gi].to(F32)
    x, y = c[:, 0] * w - 0.5, c[:, 1] * h - 0.5
    xf, yf = torch.floor(x), torch.floor(y)
    lx, ly = x - xf, y - yf
    x0, y0 = xf.long(), yf.long()
    src = f - 1 if fault == "prev_frame" and f > 0 else f
    Fm = frame_feat(cp, gi, src).float()
    rows = h
    if fault == "next_frame_corner" and f + 1 < cp.F:              # the tall image: row h is the first row of frame f + 1
        Fm = torch.cat([Fm, frame_feat(cp, gi, f + 1).float()])
        rows = h + 1
    e = torch.zeros(P, C)
    for dy, wy in ((0, one - ly), (1, ly)):
        for dx, wx in ((0, one - lx), (1, lx)):
            xi, yi = x0 + dx, y0 + dy
            inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < rows)
            wt = torch.where(inside, wy * wx, torch.zeros(()))
            e = e + wt[:, None] * Fm[yi.clamp(0, rows - 1) * w + xi.clamp(0, w - 1)]
    hi = e.to(BF16).float()
    lo = (e - hi).to(BF16).float()
    E = group_embed(cp, gi).float()
    return E @ hi.T + E @ lo.T


def emu_cost(cp, fault=None):
    """Faults: ``prev_frame`` frame f reads frame f - 1's features; ``tsamp_frame`` the frame offset into the target rows is
    dropped (every frame reads the samples of frame 0); ``divisor`` P instead of F * P; ``tail`` a frame's last tile is not cut
    at P (clamped copies of point P - 1 against the first samples of the next frame; of the last frame: against its own last
    sample); ``next_frame_corner`` a corner in row h is taken from the first row of the next frame"""
    assert fault is None or fault in CLIP_FAULTS
    cost = torch.full((cp.G, cp.Q, cp.Tmax), SENT, dtype=F32)
    F, P = cp.F, cp.P
    one = torch.ones((), dtype=F32)
    tsum = cp.tsamp.sum(1)
    pad = (P + 31) // 32 * 32 - P
    for gi in range(cp.G):
        T0, Tn = int(cp.t_first[gi]), int(cp.t_count[gi])
        if Tn <= 0:
            continue
        trow = cp.tsamp[T0:T0 + Tn]
        sx, sst = torch.zeros(cp.Q, Tn), torch.zeros(cp.Q, Tn)
        sp, ss = torch.zeros(cp.Q), torch.zeros(cp.Q)
        for f in range(F):
            X = _emu_frame_logits(cp, gi, f, fault)
            o = 0 if fault == "tsamp_frame" else f * P
            t = trow[:, o:o + P]
            if fault == "tail" and pad:
                extra = trow[:, o + P:o + P + pad] if f + 1 < F else trow[:, -1:].expand(-1, pad)
                X, t = torch.cat([X, X[:, -1:].expand(-1, pad)], 1), torch.cat([t, extra], 1)
            ex = torch.exp(-X.abs())
            s = torch.where(X >= 0, one, ex) / (1 + ex)
            sp, ss = sp + (X.clamp(min=0) + torch.log(1 + ex)).sum(1), ss + s.sum(1)
            sx, sst = sx + X @ t.T, sst + s @ t.T
        div = P if fault == "divisor" else F * P
        cost[gi, :, :Tn] = W_MASK * (sp[:, None] - sx) / div + W_DICE * (1 - (2 * sst + 1) / (ss[:, None] + tsum[None, T0:T0 + Tn] + 1))
    return cost


# the case every fault is held to
CLIP_FAULT_CASE = {"prev_frame": "K3", "tsamp_frame": "K4", "divisor": "K7", "tail": "K4", "next_frame_corner": "K6"}
