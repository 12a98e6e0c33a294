"""The point-sampled loss kernels of csrc/loss.hip restated in plain torch, fp64, in this project's own words: bilinear sampling
with explicit corners (pixel coordinate = c * size - 0.5, floor, four corners, zero outside the plane: no grid_sample), the four
mask-loss sums and their analytic gradient scattered into a plane, the mask + dice matching cost, the importance selection in
the kernels' exact output order, and the 32-pixels-per-word mask packing.  bf16 maps are read as their bf16-rounded values widened
to fp64.  tests/test_loss_restate_cpu.py holds this file to F.grid_sample, oracle/head_ref.matcher_cost and autograd;
tests/test_loss_routes_gpu.py holds every kernel route to it.  The problems of the selection tests are built here so that the CPU
test checks the input conditions of exactly the inputs the GPU test runs."""
import numpy as np
import torch

F64 = torch.float64
SELECT_TOL = 1e-5                 # a candidate whose fp64 |logit| is this close to the fp64 k-th value may go either way


def corners(coords, h, w):
    """coords [..., 2] (x, y) in plane units of [0, 1] -> (x0, y0 int64, lx, ly fp64): the pixel coordinate is c * size - 0.5,
    (x0, y0) its floor = the upper-left corner of the footprint, (lx, ly) the fractions towards x0 + 1 / y0 + 1"""
    c = coords.to(F64)
    x, y = c[..., 0] * w - 0.5, c[..., 1] * h - 0.5
    xf, yf = torch.floor(x), torch.floor(y)
    return xf.long(), yf.long(), x - xf, y - yf


def _corner_terms(coords, h, w):
    """the four (flat index clamped into the plane, weight with 0 for a corner outside the plane) of every point"""
    x0, y0, lx, ly = corners(coords, h, w)
    for dy, wy in ((0, 1.0 - ly), (1, ly)):
        for dx, wx in ((0, 1.0 - lx), (1, lx)):
            xi, yi = x0 + dx, y0 + dy
            inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            yield yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1), wy * wx * inside.to(F64)


def point_sample(planes, coords):
    """planes [R, h, w] (any dtype, read as fp64), coords [R, P, 2] or [1, P, 2] (one point set for every plane) -> [R, P] fp64"""
    R, h, w = planes.shape
    flat = planes.to(F64).reshape(R, h * w)
    out = torch.zeros(R, coords.shape[-2], dtype=F64)
    for idx, wt in _corner_terms(coords, h, w):
        out = out + flat.gather(1, idx.expand(R, -1)) * wt
    return out


def mask_loss_sums(pred, gt, coords):
    """pred [n, h, w] logits, gt [n, H, W] 0/1, coords [n, P, 2] -> [n, 4] = sums over the points of
    (BCE-with-logits(x, t), sigmoid(x) * t, sigmoid(x), t)"""
    x, t = point_sample(pred, coords), point_sample(gt, coords)
    s = torch.sigmoid(x)
    bce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    return torch.stack([bce.sum(1), (s * t).sum(1), s.sum(1), t.sum(1)], 1)


def mask_loss_grad(pred, gt, coords, g):
    """d/d pred of sum_i (g[i, 0] * bce_i + g[i, 1] * sum(s t)_i + g[i, 2] * sum(s)_i), g [n, >= 3] -> [n, h, w] fp64: per point
    dx = g0 (s - t) + (g1 t + g2) s (1 - s), scattered to the four corners with their weights (nothing for a corner outside)"""
    n, h, w = pred.shape
    x, t = point_sample(pred, coords), point_sample(gt, coords)
    s = torch.sigmoid(x)
    g = g.to(F64)
    dx = g[:, 0:1] * (s - t) + (g[:, 1:2] * t + g[:, 2:3]) * s * (1 - s)
    out = torch.zeros(n, h * w, dtype=F64)
    for idx, wt in _corner_terms(coords, h, w):
        out.scatter_add_(1, idx, dx * wt)
    return out.view(n, h, w)


def match_cost(masks, tgt, coords, w_mask, w_dice):
    """masks [Q, h, w] logits, tgt [T, H, W] 0/1, coords [1, P, 2] -> [Q, T] fp64: w_mask * (BCE of x against 1 where the target
    is set and against 0 where it is not, mean over the points) + w_dice * (1 - (2 s.t + 1) / (sum s + sum t + 1))"""
    return match_cost_samples(point_sample(masks, coords), point_sample(tgt, coords), w_mask, w_dice)


def match_cost_samples(x, t, w_mask, w_dice):
    """the cost of ``match_cost`` from given samples: x [Q, P] logits, t [T, P] target samples (read as fp64) -> [Q, T] fp64"""
    x, t = x.to(F64), t.to(F64)
    P = x.shape[1]
    softplus = lambda v: v.clamp(min=0) + torch.log1p(torch.exp(-v.abs()))
    cm = (softplus(-x) @ t.T + softplus(x) @ (1 - t).T) / P
    s = torch.sigmoid(x)
    cd = 1 - (2 * (s @ t.T) + 1) / (s.sum(1)[:, None] + t.sum(1)[None, :] + 1)
    return w_mask * cm + w_dice * cd


def select_order(vals, k):
    """vals [n, M] -> [n, k] int64 source indices in the kernels' output order: with thr = the k-th smallest |v|, the entries
    with |v| < thr in index order, then the first (k - their count) entries with |v| == thr in index order (-0.0 ties with 0.0)"""
    a = vals.abs()
    out = torch.empty(a.shape[0], k, dtype=torch.int64)
    for r in range(a.shape[0]):
        thr = a[r].kthvalue(k).values
        less = torch.nonzero(a[r] < thr).flatten()
        eq = torch.nonzero(a[r] == thr).flatten()
        out[r] = torch.cat([less, eq[:k - less.numel()]])
    return out


def pack_bits(masks):
    """masks [R, H, W] bool with H * W % 32 == 0 -> [R, H * W / 32] int32: bit j of word i of a row = its pixel 32 i + j"""
    R = masks.shape[0]
    px = masks.reshape(R, -1, 32).numpy().astype(np.uint64)
    words = (px << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32))


# ---- the problems of the selection tests (CPU: input conditions; GPU: the kernels) ------------------------------------------------
# (h, w), M candidates, k kept, seed.  M picks the instantiation of the fused kernel: <= 16384 -> 16 keys per thread, <= 37888 -> 37,
# else 40; 16385 and 37889 are the first sizes of the latter two, 40960 the cap.
SELECT_CASES = [((16, 16), 700, 1, 100), ((32, 48), 1024, 1024, 101), ((24, 40), 16385, 4000, 102), ((64, 64), 37889, 9408, 103),
                ((64, 64), 40960, 12544, 103)]
SELECT_ROWS = 3
SELECT_MAX_AMBIGUOUS = 4
# a third of the candidates wholly outside the plane: all of them have the key 0 exactly
OUTSIDE_CASE = {"hw": (24, 40), "M": 3000, "zeros": 1000, "ks": (1, 400, 1000, 1001, 2200), "seed": 104}


def select_problem(hw, M, seed, zeros=0):
    """-> (planes [SELECT_ROWS, h, w] bf16, coords [SELECT_ROWS, M, 2] f32 in [0, 1): every footprint has a corner in the
    plane); with ``zeros``, every third candidate up to that count lies wholly outside it (x in [1.2, 1.5]: logit exactly 0)"""
    g = torch.Generator().manual_seed(seed)
    planes = (torch.randn(SELECT_ROWS, *hw, generator=g) * 2).to(torch.bfloat16)
    coords = torch.rand(SELECT_ROWS, M, 2, generator=g)
    if zeros:
        coords[:, :3 * zeros:3, 0] = 1.2 + 0.3 * torch.rand(SELECT_ROWS, zeros, generator=g)
    return planes, coords


def select_bands(keys, k, tol=SELECT_TOL):
    """keys [M] fp64 |logit| -> (sure, amb) index tensors: below the k-th value by more than tol / within tol of it"""
    kth = keys.kthvalue(k).values
    return torch.nonzero(keys < kth - tol).flatten(), torch.nonzero((keys - kth).abs() <= tol).flatten()


def coords_to_index(coords_in, coords_out):
    """coords_in [M, 2] f32 (pairwise distinct), coords_out [k, 2] copies of some of its rows -> their indices [k] (-1: not a row)"""
    a = coords_in.contiguous().numpy().view(np.int64).ravel()
    b = coords_out.contiguous().numpy().view(np.int64).ravel()
    order = np.argsort(a, kind="stable")
    pos = np.clip(np.searchsorted(a[order], b), 0, len(a) - 1)
    idx = order[pos]
    return torch.from_numpy(np.where(a[idx] == b, idx, -1))


def check_selection(got, keys, k, tol=SELECT_TOL):
    """got [k] source indices in output order, keys [M] fp64: every candidate not within tol of the k-th value is in / out as in
    fp64, and the order is the kernels': with the candidates near the threshold taken out, index order; those candidates either
    in their index place or, as ties, in index order at the end"""
    sure, amb = select_bands(keys, k, tol)
    got = got.tolist()
    s_got, s_sure, s_amb = set(got), set(sure.tolist()), set(amb.tolist())
    assert len(s_got) == k and -1 not in s_got, "duplicate or foreign coordinates in the output"
    assert s_sure <= s_got, f"{len(s_sure - s_got)} candidates below the threshold are missing"
    assert s_got <= (s_sure | s_amb), f"{len(s_got - s_sure - s_amb)} candidates above the threshold were selected"
    assert [i for i in got if i not in s_amb] == sorted(s_sure), "entries below the threshold are not in index order"
    drops = [j for j in range(1, k) if got[j] < got[j - 1]]
    assert len(drops) <= 1, "output is not (index-ordered entries below the threshold) + (index-ordered ties)"
    if drops:
        assert set(got[drops[0]:]) <= s_amb, "the tie segment holds entries that are not near the threshold"
