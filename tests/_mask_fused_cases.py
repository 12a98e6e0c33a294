"""The problems, fp64 references, bounds, geometry mirrors and single-fault emulations of the fused mask product kernels
(csrc/mask_fused.hip: mpf_pair_planes_forward, mpf_pair_planes_backward, mpf_match_cost_fused).  No GPU and no library is needed
to import this file.  tests/test_mask_fused_cases_cpu.py holds the references to einsum / autograd / the oracle, the case tables to
the branches they name, the mirrors to the built library and every fault of the emulation to a failing check;
tests/test_mask_fused_routes_gpu.py runs the same problems through the C ABI and the same check functions.

Buffers carry poison: every embedding row, feature gap, gradient-plane row and target-sample row that no pair or group addresses
is NaN, so a read outside the addressed set shows in the result (the kernels' clamped loads stay inside the addressed set, and the
zero weights of points outside a plane are applied by selection; the one product with a zero operand, d F's zero-padded Et, reads
the finite row count - 1).  Result buffers start as a sentinel that is exact in bf16.

Pair planes, every element, fp64 reference on the bf16 values (derivation: tests/test_small_gemm_forms_gpu.py):
    |got - ref| <= 2^-8 |ref| [output is bf16] + (K + 8) 2^-22 S + 1e-30
with K the contraction length as the kernel pads it and S the sum of the absolute products.  Contractions of more than 1024
pixels (d E at the long-chunk cases) use gradient planes that are non-zero only on the boundaries of the pixel split, so that S has
a handful of terms and one lost pixel is many bounds; the other slots of the image stay dense.
Matching cost, every entry t < t_count[g]: |got - ref| <= 2e-4 + 2e-4 |ref| with w_mask = w_dice = 5."""
from types import SimpleNamespace

import numpy as np
import torch

import _loss_restate as LR

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
C = 256
SENT_OUT, SENT_GRAD = 3.0, -7.0            # exact in bf16
NAN = float("nan")
W_MASK = W_DICE = 5.0
COST_RTOL = COST_ATOL = 2e-4
EMBED_SCALE_COST = 0.5


# ---- geometry mirrors (pb_geom, mc_geom, the TCH choice and the two workspace formulas of csrc/mask_fused.hip) ----------------------
def align256(x):
    return (x + 255) & ~255


def pb_geom(N, HW, max_count):
    KP = max(64, (max_count + 63) // 64 * 64)
    mgroups = max(1, (max_count + 127) // 128)
    ks = max(1, min(64, 512 // max(1, N * mgroups)))
    while ks > 1 and HW % (ks * 64):
        ks -= 1
    return SimpleNamespace(KP=KP, mgroups=mgroups, KS=ks, px_per_chunk=HW // ks)


def pb_workspace_bytes(N, HW, total_slots, max_count):
    if N <= 0 or HW <= 0 or total_slots <= 0 or max_count <= 0:
        return 0
    p = pb_geom(N, HW, max_count)
    return align256(N * C * p.KP * 2) + align256(p.KS * total_slots * C * 4) + align256(total_slots * 4)


def mc_geom(G, Q, P):
    ntiles = (P + 31) // 32
    qgroups = (Q + 127) // 128
    want = max(1, 512 // max(1, G * qgroups))
    tiles_per_wg = (ntiles + want - 1) // want
    nwg = (ntiles + tiles_per_wg - 1) // tiles_per_wg
    return SimpleNamespace(ntiles=ntiles, qgroups=qgroups, tiles_per_wg=tiles_per_wg, nwg=nwg, last_tiles=ntiles - (nwg - 1) * tiles_per_wg)


def tch_of(Tmax):
    need = (Tmax + 1) // 2
    return next(t for t in (4, 8, 12, 16, 24, 32, 64) if need <= t)


def mc_workspace_bytes(G, Q, Tmax, P, tsamp_rows):
    if G <= 0 or Q <= 0 or Tmax <= 0 or P <= 0 or tsamp_rows < 0:
        return 0
    m = mc_geom(G, Q, P)
    return align256(m.nwg * G * Q * Tmax * 2 * 4) + align256(m.nwg * G * Q * 2 * 4) + align256(tsamp_rows * 4)


# ---- case tables ----------------------------------------------------------------------------------------------------------------------
FWD_HW = [(2, 2), (10, 10), (11, 12), (8, 16), (13, 20)]
FWD_COUNTS = [(1,), (15, 16), (17, 31), (32, 33), (48, 49, 0)]
# name -> N, (h, w), counts, slot_first / total_slots (None: packed), sparse planes, and the geometry the case is there for:
# (KP, mgroups, KS, 64-pixel steps per chunk)
P9_COUNTS = tuple(0 if b == 7 else 1 for b in range(300))
PAIR_CASES = {
    "P1": dict(N=1, hw=(8, 16), counts=(1,), sparse=False, geom=(64, 1, 2, 1)),
    "P2": dict(N=3, hw=(8, 48), counts=(63, 0, 64), sparse=False, geom=(64, 1, 6, 1)),
    "P3": dict(N=2, hw=(20, 32), counts=(65, 1), sparse=False, geom=(128, 1, 10, 1)),
    "P4": dict(N=2, hw=(16, 64), counts=(129, 128), sparse=False, geom=(192, 2, 16, 1)),
    "P5": dict(N=1, hw=(32, 32), counts=(257,), sparse=False, geom=(320, 3, 16, 1)),
    "P6": dict(N=1, hw=(67, 128), counts=(5,), sparse=True, geom=(64, 1, 2, 67)),
    "P7": dict(N=2, hw=(96, 128), counts=(3, 130), sparse=True, geom=(192, 2, 64, 3)),
    "P8": dict(N=3, hw=(16, 16), counts=(5, 0, 37), slot_first=(3, 50, 60), total_slots=100, sparse=False, geom=(64, 1, 4, 1)),
    "P9": dict(N=300, hw=(8, 16), counts=P9_COUNTS, sparse=False, geom=(64, 1, 1, 2)),
}
# name -> L, N, Q, counts per image, P, maps, and (TCH, qgroups, tiles_per_wg, nwg, tiles of the last workgroup)
COST_CASES = {
    "C1": dict(L=1, N=1, Q=1, counts=(1,), P=1, hw=(4, 4), geom=(4, 1, 1, 1, 1)),
    "C2": dict(L=2, N=3, Q=127, counts=(8, 0, 3), P=31, hw=(8, 12), geom=(4, 1, 1, 1, 1), outside_group=3),
    "C3": dict(L=2, N=2, Q=128, counts=(9, 16), P=32, hw=(8, 12), geom=(8, 1, 1, 1, 1)),
    "C4": dict(L=1, N=3, Q=129, counts=(17, 24, 1), P=33, hw=(8, 12), geom=(12, 2, 1, 2, 1)),
    "C5": dict(L=2, N=2, Q=10, counts=(25, 32), P=112, hw=(8, 12), geom=(16, 1, 1, 4, 1)),
    "C6": dict(L=1, N=2, Q=10, counts=(33, 48), P=1000, hw=(8, 12), geom=(24, 1, 1, 32, 1)),
    "C7": dict(L=1, N=2, Q=10, counts=(49, 64), P=1001, hw=(8, 12), geom=(32, 1, 1, 32, 1)),
    "C8": dict(L=1, N=4, Q=10, counts=(65, 128, 0, 127), P=100, hw=(8, 12), geom=(64, 1, 1, 4, 1)),
    "C9": dict(L=8, N=8, Q=8, counts=(0, 5, 1, 3, 2, 0, 4, 5), P=330, hw=(8, 12), geom=(4, 1, 2, 6, 1)),
    "C10": dict(L=2, N=2, Q=200, counts=(6, 2), P=4128, hw=(8, 12), geom=(4, 2, 3, 43, 3)),
}


# ---- pair-plane problems --------------------------------------------------------------------------------------------------------------
def boundary_pixels(HW, KS):
    """the pixels on the boundaries of the d E pixel split: 0, 63, 64, the last pixel of every chunk and the first of the next,
    HW - 65, HW - 64, HW - 1"""
    ppc = HW // KS
    px = {0, 63, 64, HW - 65, HW - 64, HW - 1}
    for kc in range(1, KS):
        px |= {kc * ppc - 1, kc * ppc}
    return sorted(p for p in px if 0 <= p < HW)


def pair_problem(N, hw, counts, seed, slot_first=None, total_slots=None, sparse=False, gap=0, backward=True, **_):
    """-> namespace of CPU tensors.  ``gap`` unaddressed slots before, between and after the images' ranges (packed when 0)."""
    h, w = hw
    HW = h * w
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, dtype=np.int64)
    assert len(counts) == N
    if slot_first is None:
        first = gap + np.concatenate([[0], np.cumsum(counts + gap)[:-1]])
        total = int(first[-1] + counts[-1] + gap)
    else:
        first, total = np.asarray(slot_first, dtype=np.int64), int(total_slots)
    max_count = int(counts.max())
    R = max_count + 3                                              # every image keeps at least three rows that no pair addresses
    embed = torch.full((R, N, C), NAN, dtype=BF16)                 # sequence-first parent: row stride N * 256
    slot_img = np.full(total, -1, dtype=np.int64)
    slot_row = np.full(total, -1, dtype=np.int64)
    for b in range(N):
        rows = rng.permutation(R)[:counts[b]]
        slot_img[first[b]:first[b] + counts[b]] = b
        slot_row[first[b]:first[b] + counts[b]] = rows
        embed[rows, b] = torch.randn(len(rows), C, generator=g).to(BF16)
    valid = slot_img >= 0
    vslots = np.nonzero(valid)[0]
    feat_stride = HW * C + 64
    feat = torch.full((N * feat_stride,), NAN, dtype=BF16)          # the 64 elements behind every image stay NaN
    for b in range(N):
        if counts[b] > 0:                                           # (an image without pairs is never read)
            feat[b * feat_stride:b * feat_stride + HW * C] = torch.randn(HW * C, generator=g).to(BF16)
    pb = SimpleNamespace(N=N, h=h, w=w, HW=HW, counts=counts, first=first, total=total, max_count=max_count, R=R, embed=embed,
                         feat=feat, feat_stride=feat_stride, slot_img=slot_img, slot_row=slot_row, valid=torch.from_numpy(valid),
                         vslots=vslots, sparse=sparse, seed=seed, G=None, sparse_slots=np.zeros(0, np.int64), sparse_px=[])
    pb.poison_row = int(np.setdiff1d(np.arange(R), slot_row[slot_img == 0])[0]) * N * C      # a NaN row (of image 0)
    set_pair_order(pb, rng.permutation(len(vslots)))
    if backward:
        geom = pb_geom(N, HW, max_count)
        G = torch.full((total, HW), NAN, dtype=BF16)               # rows outside every image's range stay NaN
        G[vslots] = torch.randn(len(vslots), HW, generator=g).to(BF16)
        if sparse:
            pb.sparse_px = boundary_pixels(HW, geom.KS)
            pb.sparse_slots = np.array([s for s in vslots if (s - first[slot_img[s]]) % 2 == 0], dtype=np.int64)
            v = torch.randn(len(pb.sparse_slots), len(pb.sparse_px), generator=g)
            rows = torch.zeros(len(pb.sparse_slots), HW)
            rows[:, pb.sparse_px] = torch.sign(v) * (0.5 + v.abs())
            G[pb.sparse_slots] = rows.to(BF16)
        pb.G, pb.geom = G, geom
    return pb


def set_pair_order(pb, perm):
    """list the pairs in the order ``perm`` of the valid slots: row_off [pairs + 1] (the last entry a NaN row, what the slots of no
    range point to) and pair_of_slot [total]"""
    n = len(pb.vslots)
    order = pb.vslots[perm]                                         # slot of every pair
    row_off = np.empty(n + 1, dtype=np.int64)
    row_off[:n] = pb.slot_row[order] * pb.N * C + pb.slot_img[order] * C
    row_off[n] = pb.poison_row
    pos = np.full(pb.total, n, dtype=np.int32)
    pos[order] = np.arange(n, dtype=np.int32)
    pb.row_off, pb.pair_of_slot = torch.from_numpy(row_off), torch.from_numpy(pos)


def feat_image(pb, b):
    return pb.feat[b * pb.feat_stride:b * pb.feat_stride + pb.HW * C].view(pb.HW, C)


def slot_rows(pb, slots):
    return pb.embed[pb.slot_row[slots], pb.slot_img[slots]]


def image_slots(pb, b):
    return np.arange(pb.first[b], pb.first[b] + pb.counts[b])


def planes_ref(pb):
    """-> (ref, S) fp64 [valid slots, HW] in slot order"""
    ref, S = [], []
    for b in range(pb.N):
        if pb.counts[b] > 0:
            E, F = slot_rows(pb, image_slots(pb, b)).to(F64), feat_image(pb, b).to(F64)
            ref.append(E @ F.T)
            S.append(E.abs() @ F.abs().T)
    return torch.cat(ref), torch.cat(S)


def grads_ref(pb):
    """-> namespace: dF, S_dF, K_dF [N, HW, C] (image without pairs: zero) and dE, S_dE [valid slots, C] in slot order"""
    dF, SF, KF = (torch.zeros(pb.N, pb.HW, C, dtype=F64) for _ in range(3))
    dE, SE = [], []
    for b in range(pb.N):
        if pb.counts[b] > 0:
            sl = image_slots(pb, b)
            E, F, G = slot_rows(pb, sl).to(F64), feat_image(pb, b).to(F64), pb.G[sl].to(F64)
            dF[b], SF[b] = G.T @ E, G.abs().T @ E.abs()
            KF[b] = max(64, (int(pb.counts[b]) + 63) // 64 * 64)
            dE.append(G @ F)
            SE.append(G.abs() @ F.abs())
    return SimpleNamespace(dF=dF, S_dF=SF, K_dF=KF, dE=torch.cat(dE), S_dE=torch.cat(SE), K_dE=pb.HW + pb.geom.KS)


def pair_bound(ref, S, K, out_bf16):
    return (2.0 ** -8 * ref.abs() if out_bf16 else 0.0) + (K + 8) * 2.0 ** -22 * S + 1e-30


def hold(route, what, got, ref, bound):
    """print the worst error of this comparison, then assert |got - ref| <= bound for every element -> (max abs err, worst err/bound)"""
    got = got.detach().to(F64).cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got - ref).abs()
    frac = err / bound
    bad = int((~(frac <= 1.0)).sum())
    print(f"[mask-fused] {route} | {what} | max abs err {float(err.max()):.3e} | worst err/bound {float(frac.max()):.3e} | "
          f"{bad} of {frac.numel()} outside")
    assert bool(torch.isfinite(got).all()) and bad == 0, (route, what, float(err.max()), float(frac.max()), bad)
    return float(err.max()), float(frac.max())


def check_planes(pb, out, what=""):
    """out [total, HW] bf16 that started as SENT_OUT"""
    ref, S = planes_ref(pb)
    out = out.cpu()
    assert bool((out[~pb.valid] == SENT_OUT).all()), "a slot outside every image's range was written"
    return hold("pair_planes_fwd_kernel", f"planes {what}", out[pb.valid], ref, pair_bound(ref, S, C, True))


def check_dfeat(pb, dF, refs, what=""):
    """dF [N, HW, C] bf16"""
    dF = dF.cpu()
    for b in range(pb.N):
        if pb.counts[b] == 0:
            assert bool((dF[b] == 0).all()), f"image {b} has no pairs: its feature gradient must be exactly zero"
    return hold("pair_planes_dfeat_kernel", f"d F {what}", dF, refs.dF, pair_bound(refs.dF, refs.S_dF, refs.K_dF, True))


def check_dembed(pb, dE, refs, what=""):
    """dE [R, N, C] bf16 or fp32 that started as SENT_GRAD: the paired rows within the bound, every other row untouched"""
    dE = dE.cpu()
    paired = torch.zeros(pb.R, pb.N, dtype=torch.bool)
    paired[pb.slot_row[pb.vslots], pb.slot_img[pb.vslots]] = True
    assert int(paired.sum()) == len(pb.vslots), "the rows of the valid slots must be distinct"
    assert bool((dE[~paired] == SENT_GRAD).all()), "a row that is in no pair was written"
    name = "bf16" if dE.dtype == BF16 else "float"
    return hold(f"pair_planes_dembed_kernel + reduce<{name}>", f"d E {what}", dE[pb.slot_row[pb.vslots], pb.slot_img[pb.vslots]], refs.dE,
                pair_bound(refs.dE, refs.S_dE, refs.K_dE, dE.dtype == BF16))


# ---- emulation of the pair-plane kernels' index arithmetic, one fault at a time -------------------------------------------------------
PLANES_FAULTS = ("fragment", "pair_order", "slot_count", "tail", "image")
DFEAT_FAULTS = ("et_pad", "last_slot")
DEMBED_FAULTS = ("chunk_tail", "chunk_missing", "slot_row")


def _row_of_pair(pb, pr):
    off = int(pb.row_off[min(int(pr), len(pb.row_off) - 1)])
    return pb.embed.view(-1)[off:off + C]


def emu_planes(pb, fault=None):
    """fp32 accumulation, one rounding to bf16.  Faults: ``fragment`` channels 104..111 (step 3, lane group 1) missing for the
    second wave's pixels; ``pair_order`` slot index used as pair index; ``slot_count`` slot ``count`` written too (the clamped
    row's plane); ``tail`` the last 4-pixel group of a plane that is no multiple of 128 not written; ``image`` features of b - 1"""
    assert fault is None or fault in PLANES_FAULTS
    out = torch.full((pb.total, pb.HW), SENT_OUT, dtype=BF16)
    px = torch.arange(pb.HW)
    for b in range(pb.N):
        first, cnt = int(pb.first[b]), int(pb.counts[b])
        if cnt <= 0:
            continue
        F = feat_image(pb, b - 1 if fault == "image" and b > 0 and pb.counts[b - 1] > 0 else b).float()
        for j in range(cnt + (1 if fault == "slot_count" else 0)):
            s = first + min(j, cnt - 1)
            e = _row_of_pair(pb, s if fault == "pair_order" else pb.pair_of_slot[s]).float()
            acc = F @ e
            if fault == "fragment":
                wave1 = (px % 128 >= 32) & (px % 128 < 64)
                acc = torch.where(wave1, acc - F[:, 104:112] @ e[104:112], acc)
            n = pb.HW - 4 if fault == "tail" and pb.HW % 128 else pb.HW
            out[first + j, :n] = acc.to(BF16)[:n]
    return out


def emu_dfeat(pb, fault=None):
    """K = count rounded up to 64: G rows clamped to count - 1, Et zero for k >= count.  Faults: ``et_pad`` Et not zeroed (the
    clamped copies are added); ``last_slot`` the last slot left out"""
    assert fault is None or fault in DFEAT_FAULTS
    dF = torch.zeros(pb.N, pb.HW, C, dtype=BF16)
    for b in range(pb.N):
        first, cnt = int(pb.first[b]), int(pb.counts[b])
        if cnt <= 0:
            continue
        k = np.arange((cnt + 63) // 64 * 64)
        src = first + np.minimum(k, cnt - 1)
        Et = torch.stack([_row_of_pair(pb, pb.pair_of_slot[s]) for s in src]).float()
        live = torch.from_numpy(k < (cnt - 1 if fault == "last_slot" else cnt))
        if fault != "et_pad":
            Et = torch.where(live[:, None], Et, torch.zeros(()))
        dF[b] = (pb.G[src].float().T @ Et).to(BF16)
    return dF


def emu_dembed(pb, dtype, fault=None):
    """KS fp32 partial sums over pixel chunks, added in chunk order, one rounding to ``dtype``, written to the row of the slot's
    pair.  Faults: ``chunk_tail`` the last pixel of chunk 0 dropped; ``chunk_missing`` the last chunk's partial left out;
    ``slot_row`` the row of pair ``slot`` written instead of the row of the slot's pair"""
    assert fault is None or fault in DEMBED_FAULTS
    KS, ppc = pb.geom.KS, pb.geom.px_per_chunk
    dE = torch.full((pb.R * pb.N * C,), SENT_GRAD, dtype=dtype)
    for b in range(pb.N):
        if pb.counts[b] <= 0:
            continue
        sl = image_slots(pb, b)
        G = pb.G[sl].float().clone()
        if fault == "chunk_tail":
            G[:, ppc - 1] = 0.0
        part = torch.einsum("skp,kpc->ksc", G.view(len(sl), KS, ppc), feat_image(pb, b).float().view(KS, ppc, C))
        v = torch.zeros(len(sl), C)
        for kc in range(KS - 1 if fault == "chunk_missing" else KS):
            v = v + part[kc]
        for i, s in enumerate(sl):
            pr = s if fault == "slot_row" else pb.pair_of_slot[s]
            off = int(pb.row_off[min(int(pr), len(pb.row_off) - 1)])
            dE[off:off + C] = v[i].to(dtype)
    return dE.view(pb.R, pb.N, C)


# ---- matching-cost problems -----------------------------------------------------------------------------------------------------------
GT_HW = (16, 24)


def cost_problem(L, N, Q, counts, P, hw, seed, outside_group=None, **_):
    """group g = l * N + b (decoder output l, image b = group_image[g]); its queries are rows l * Qt + 3 + q of image b in the
    [L * Qt, N, 256] parent (Qt = Q + 3); its targets the tsamp rows t_first[g] .. + counts[b], with NaN rows before, between and
    behind the groups' ranges"""
    h, w = hw
    g = torch.Generator().manual_seed(seed)
    G, Qt = L * N, Q + 3
    counts = np.asarray(counts, dtype=np.int64)
    Tmax = int(counts.max())
    group_image = np.tile(np.arange(N), L).astype(np.int32)
    t_count = counts[group_image].astype(np.int32)
    embed = torch.full((L * Qt, N, C), NAN, dtype=BF16)
    embed_first = np.zeros(G, dtype=np.int64)
    for gi in range(G):
        l, b = divmod(gi, N)
        embed_first[gi] = (l * Qt + 3) * N * C + b * C
        if t_count[gi] > 0:
            embed[l * Qt + 3:(l + 1) * Qt, b] = (torch.randn(Q, C, generator=g) * EMBED_SCALE_COST).to(BF16)
    feat_stride = h * w * C + 64
    feat = torch.full((N * feat_stride,), NAN, dtype=BF16)
    for b in range(N):
        if counts[b] > 0:
            feat[b * feat_stride:b * feat_stride + h * w * C] = torch.randn(h * w * C, generator=g).to(BF16)
    coords = torch.rand(G, P, 2, generator=g) * 1.2 - 0.1
    planted = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.5 / w, 0.5 / w], [(w - 0.5) / w, (w - 0.5) / w], [2.0, -1.0], [-1.0, 2.0]])
    coords[:, :min(P, 6)] = planted[:min(P, 6)]
    if outside_group is not None:                                  # every footprint wholly outside the plane: logits exactly 0
        coords[outside_group, :, 0] = 1.3 + 0.2 * torch.rand(P, generator=g)
    masks = [torch.rand(int(c), *GT_HW, generator=g) < 0.4 for c in counts]
    t_first = np.zeros(G, dtype=np.int32)
    rows, r = [torch.full((2, P), NAN)], 2
    for gi in range(G):
        t_first[gi] = r
        if t_count[gi] > 0:
            rows.append(LR.point_sample(masks[group_image[gi]], coords[gi:gi + 1]).to(F32))
        rows.append(torch.full((1, P), NAN))
        r += int(t_count[gi]) + 1
    tsamp = torch.cat(rows)
    assert tsamp.shape[0] == r
    return SimpleNamespace(L=L, N=N, Q=Q, Qt=Qt, G=G, P=P, h=h, w=w, counts=counts, Tmax=Tmax, group_image=group_image, t_first=t_first,
                           t_count=t_count, embed=embed, embed_first=embed_first, row_stride=N * C, feat=feat, feat_stride=feat_stride,
                           coords=coords, masks=masks, tsamp=tsamp, outside_group=outside_group)


def group_embed(cp, gi):
    return cp.embed.view(-1)[cp.embed_first[gi]:].as_strided((cp.Q, C), (cp.row_stride, 1))


def group_feat(cp, gi):
    b = int(cp.group_image[gi])
    return cp.feat[b * cp.feat_stride:b * cp.feat_stride + cp.h * cp.w * C].view(cp.h * cp.w, C)


def logits_ref(E, F, coords, h, w):
    """logit(q, p) = sum_c E[q, c] * bilinear(F[:, :, c])(p): E [Q, C], F [h * w, C], coords [P, 2] -> [Q, P] fp64"""
    Fd = F.to(F64)
    Fs = torch.zeros(coords.shape[0], Fd.shape[1], dtype=F64)
    for idx, wt in LR._corner_terms(coords, h, w):
        Fs = Fs + Fd[idx] * wt[:, None]
    return E.to(F64) @ Fs.T


def cost_ref(cp):
    """-> list over the groups of [Q, t_count[g]] fp64 (None for a group without targets)"""
    out = []
    for gi in range(cp.G):
        T0, Tn = int(cp.t_first[gi]), int(cp.t_count[gi])
        x = logits_ref(group_embed(cp, gi), group_feat(cp, gi), cp.coords[gi], cp.h, cp.w) if Tn else None
        out.append(LR.match_cost_samples(x, cp.tsamp[T0:T0 + Tn], W_MASK, W_DICE) if Tn else None)
    return out


def check_cost(cp, cost, ref, what=""):
    """cost [G, Q, Tmax] fp32 that started as SENT_GRAD"""
    cost = cost.cpu()
    for gi in range(cp.G):
        assert bool((cost[gi, :, int(cp.t_count[gi]):] == SENT_GRAD).all()), f"group {gi}: entries t >= {cp.t_count[gi]} were written"
    live = [gi for gi in range(cp.G) if cp.t_count[gi] > 0]
    got = torch.cat([cost[gi, :, :int(cp.t_count[gi])].reshape(-1) for gi in live])
    want = torch.cat([ref[gi].reshape(-1) for gi in live])
    return hold("match_cost_fused_kernel", f"cost {what}", got, want, COST_ATOL + COST_RTOL * want.abs())


COST_FAULTS = ("no_lo", "corner", "tail", "tch", "t_first")


def emu_cost(cp, fault=None):
    """fp32 coordinates, weights and interpolation, the interpolated features as two bf16 planes (value and remainder), fp32
    sums.  Faults: ``no_lo`` remainder plane dropped; ``corner`` x0 + 1; ``tail`` the last tile not cut at P (clamped copies of
    point P - 1 counted); ``tch`` target TCH reads target TCH - 1's samples; ``t_first`` row sums taken at t instead of t_first + t"""
    assert fault is None or fault in COST_FAULTS
    cost = torch.full((cp.G, cp.Q, cp.Tmax), SENT_GRAD, dtype=F32)
    TCH, h, w, P = tch_of(cp.Tmax), cp.h, cp.w, cp.P
    tsum = cp.tsamp.sum(1)
    one = torch.ones((), dtype=F32)
    for gi in range(cp.G):
        T0, Tn = int(cp.t_first[gi]), int(cp.t_count[gi])
        if Tn <= 0:
            continue
        c = cp.coords[gi].to(F32)
        x, y = c[:, 0] * w - 0.5, c[:, 1] * h - 0.5
        xf, yf = torch.floor(x), torch.floor(y)
        lx, ly = x - xf, y - yf
        x0, y0 = xf.long() + (1 if fault == "corner" else 0), yf.long()
        F = group_feat(cp, gi).float()
        e = torch.zeros(P, C)
        for dy, wy in ((0, one - ly), (1, ly)):
            for dx, wx in ((0, one - lx), (1, lx)):
                xi, yi = x0 + dx, y0 + dy
                inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
                wt = torch.where(inside, wy * wx, torch.zeros(()))
                e = e + wt[:, None] * F[yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)]
        hi = e.to(BF16).float()
        lo = (e - hi).to(BF16).float()
        E = group_embed(cp, gi).float()
        X = E @ hi.T if fault == "no_lo" else E @ hi.T + E @ lo.T
        t = cp.tsamp[T0:T0 + Tn].clone()
        if fault == "tch" and Tn > TCH:
            t[TCH] = t[TCH - 1]
        if fault == "tail":
            idx = torch.arange((P + 31) // 32 * 32).clamp(max=P - 1)
            X, t = X[:, idx], t[:, idx]
        ex = torch.exp(-X.abs())
        s = torch.where(X >= 0, one, ex) / (1 + ex)
        sp, ss = (X.clamp(min=0) + torch.log(1 + ex)).sum(1), s.sum(1)
        st = tsum[:Tn] if fault == "t_first" else tsum[T0:T0 + Tn]
        cost[gi, :, :Tn] = W_MASK * (sp[:, None] - X @ t.T) / P + W_DICE * (1 - (2 * (s @ t.T) + 1) / (ss[:, None] + st[None, :] + 1))
    return cost


# the case every fault is held to (tests/test_mask_fused_cases_cpu.py); forward cases are (hw, counts) of the forward table
FWD_FAULT_CASE = {"fragment": ((10, 10), (15, 16)), "pair_order": ((8, 16), (17, 31)), "slot_count": ((11, 12), (32, 33)),
                  "tail": ((11, 12), (1,)), "image": ((13, 20), (48, 49, 0))}
DFEAT_FAULT_CASE = {"et_pad": "P3", "last_slot": "P2"}
DEMBED_FAULT_CASE = {"chunk_tail": ("P2", "P6"), "chunk_missing": ("P4", "P7"), "slot_row": ("P8",)}
COST_FAULT_CASE = {"no_lo": "C5", "corner": "C1", "tail": "C4", "tch": "C3", "t_first": "C2"}


def fwd_problem(hw, counts):
    return pair_problem(len(counts), hw, counts, seed=1000 + 37 * FWD_HW.index(hw) + FWD_COUNTS.index(counts), gap=2, backward=False)


def pair_case(name):
    return pair_problem(seed=2000 + int(name[1:]), **PAIR_CASES[name])


def cost_case(name):
    return cost_problem(seed=3000 + int(name[1:]), **COST_CASES[name])
