"""CPU: tests/_loss_restate.py (explicit-corner fp64 restatement of the point-sampled loss kernels) held to F.grid_sample, to
oracle/head_ref.matcher_cost and to autograd, and the input conditions of the GPU selection cases (tests/test_loss_routes_gpu.py)
checked on the restatement alone."""
import pytest
import torch
import torch.nn.functional as F

import _loss_restate as LR

F64 = torch.float64


def _grid_sample(planes, coords):
    """planes [R, h, w], coords [R, P, 2] -> [R, P] through F.grid_sample in fp64"""
    return F.grid_sample(planes.to(F64)[:, None], 2.0 * coords.to(F64).unsqueeze(2) - 1.0, mode="bilinear", padding_mode="zeros",
                         align_corners=False)[:, 0, :, 0]


def _coords(g, R, P, h, w):
    """uniform in [-0.2, 1.2] with the edge cases in front: the plane's corners, pixel centres, pixel borders, points whose
    footprint is half / wholly outside"""
    c = torch.rand(R, P, 2, generator=g) * 1.4 - 0.2
    special = torch.tensor([[0.0, 0.0], [1.0, 1.0], [0.0, 1.0], [1.0, 0.0], [0.5 / w, 0.5 / h], [1.0 - 0.5 / w, 1.0 - 0.5 / h],
                            [2.5 / w, 1.5 / h], [1.0 / w, 2.0 / h], [-0.5 / w, 0.3], [0.3, 1.0 + 0.5 / h], [-1.5 / w, 0.5],
                            [0.5, 1.0 + 1.5 / h], [1.5, 1.5], [-0.6, 0.2]])
    c[:, :len(special)] = special
    return c


@pytest.mark.parametrize("hw", [(5, 7), (16, 24), (1, 1), (33, 2)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.bool])
def test_point_sample_equals_grid_sample(hw, dtype):
    g = torch.Generator().manual_seed(0)
    R, P = 4, 400
    x = torch.randn(R, *hw, generator=g) * 3
    x = (x > 0) if dtype == torch.bool else x.to(dtype)
    c = _coords(g, R, P, *hw)
    got = LR.point_sample(x, c)
    torch.testing.assert_close(got, _grid_sample(x, c), rtol=1e-12, atol=1e-12)
    # exact facts: a pixel centre returns the pixel, the plane's corner a quarter of the corner pixel, far outside 0
    xd = x.to(F64)
    if hw[0] >= 3 and hw[1] >= 3:                 # (the centre's fp32 coordinate is off by a rounding: 1e-5 of the pixel values)
        torch.testing.assert_close(got[:, 6], xd[:, 1, 2], rtol=0, atol=1e-5)
    torch.testing.assert_close(got[:, 0], 0.25 * xd[:, 0, 0], rtol=1e-14, atol=0)
    assert (got[:, 12] == 0).all() and (got[:, 13] == 0).all()
    # one shared point set = the same set given to every plane
    assert torch.equal(LR.point_sample(x, c[:1]), LR.point_sample(x, c[:1].expand(R, -1, -1)))


def test_match_cost_equals_the_oracle():
    from oracle import head_ref as O
    g = torch.Generator().manual_seed(1)
    Q, T, (h, w), (H, W), P = 7, 5, (16, 24), (40, 56), 500
    masks = (torch.randn(Q, h, w, generator=g) * 3).double()
    gts = torch.rand(T, H, W, generator=g) < 0.3
    coords = (torch.rand(1, P, 2, generator=g) * 1.2 - 0.1).double()
    ref = O.matcher_cost(torch.zeros(Q, 4, dtype=F64), masks, torch.zeros(T, dtype=torch.long), gts, coords, w_class=0.0, w_mask=5.0,
                         w_dice=3.0)
    # the oracle narrows the samples to fp32 before the losses (its `.float()`): 1e-6 is that rounding, not the restatement's
    torch.testing.assert_close(LR.match_cost(masks, gts, coords, 5.0, 3.0), ref.double(), rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("hw", [(5, 7), (16, 24)])
def test_mask_loss_sums_and_gradient_equal_autograd_through_grid_sample(hw):
    g = torch.Generator().manual_seed(2)
    n, (H, W), P = 4, (40, 56), 300
    pred = (torch.randn(n, *hw, generator=g) * 2).double().requires_grad_(True)
    gt = torch.rand(n, H, W, generator=g) < 0.4
    c = _coords(g, n, P, *hw)
    gs = torch.randn(n, 4, generator=g).double()
    x, t = _grid_sample(pred, c), _grid_sample(gt, c)
    s = x.sigmoid()
    ref = torch.stack([F.binary_cross_entropy_with_logits(x, t, reduction="none").sum(1), (s * t).sum(1), s.sum(1), t.sum(1)], 1)
    torch.testing.assert_close(LR.mask_loss_sums(pred.detach(), gt, c), ref.detach(), rtol=1e-12, atol=1e-12)
    (ref * gs).sum().backward()
    torch.testing.assert_close(LR.mask_loss_grad(pred.detach(), gt, c, gs), pred.grad, rtol=1e-11, atol=1e-12)
    # autograd through the restatement's own sums agrees with its analytic gradient as well
    p2 = pred.detach().clone().requires_grad_(True)
    (LR.mask_loss_sums(p2, gt, c) * gs).sum().backward()
    torch.testing.assert_close(LR.mask_loss_grad(pred.detach(), gt, c, gs), p2.grad, rtol=1e-11, atol=1e-12)


def test_select_order_is_the_kernel_order():
    v = torch.tensor([[3.0, -1.0, 0.5, 1.0, -0.5, 2.0, 0.5, -0.0, 0.0, -3.0]])
    assert LR.select_order(v, 1).tolist() == [[7]]                    # -0.0 and 0.0 tie: the first by index
    assert LR.select_order(v, 2).tolist() == [[7, 8]]
    assert LR.select_order(v, 3).tolist() == [[7, 8, 2]]              # thr 0.5: the zeros are below it, then the first 0.5
    assert LR.select_order(v, 6).tolist() == [[2, 4, 6, 7, 8, 1]]     # thr 1: below it in index order, then the first of the 1s
    assert LR.select_order(v, 10).tolist() == [[1, 2, 3, 4, 5, 6, 7, 8, 0, 9]]
    g = torch.Generator().manual_seed(3)
    r = torch.randn(3, 200, generator=g)
    for k in (1, 17, 200):
        idx = LR.select_order(r, k)
        for i in range(3):
            assert set(idx[i].tolist()) == set(r[i].abs().topk(k, largest=False).indices.tolist())


def test_pack_bits_layout():
    m = torch.zeros(2, 4, 16, dtype=torch.bool)
    m[0, 0, 0] = True; m[0, 1, 15] = True; m[0, 2, 3] = True; m[1, 3, 15] = True
    w = LR.pack_bits(m)
    assert w.dtype == torch.int32 and w.tolist() == [[1 - (1 << 31), 1 << 3], [0, -(1 << 31)]]
    g = torch.Generator().manual_seed(4)
    m = torch.rand(3, 12, 40, generator=g) < 0.4                      # rows of 40 pixels straddle the words
    w = LR.pack_bits(m).numpy().view("uint32")
    flat = m.reshape(3, -1)
    for r, i in ((0, 0), (1, 33), (2, 479), (2, 40), (1, 319)):
        assert bool((w[r, i // 32] >> (i % 32)) & 1) == bool(flat[r, i])


@pytest.mark.parametrize("hw,M,k,seed", LR.SELECT_CASES)
def test_selection_cases_have_few_candidates_near_the_threshold(hw, M, k, seed):
    """what tests/test_loss_routes_gpu.py relies on: distinct coordinates (an output row names its source), and at most
    SELECT_MAX_AMBIGUOUS candidates per row, the k-th itself included, whose fp64 |logit| is within SELECT_TOL of the k-th"""
    planes, coords = LR.select_problem(hw, M, seed)
    keys = LR.point_sample(planes, coords).abs()
    for r in range(LR.SELECT_ROWS):
        assert len(torch.unique(coords[r], dim=0)) == M
        sure, amb = LR.select_bands(keys[r], k)
        assert 1 <= len(amb) <= LR.SELECT_MAX_AMBIGUOUS, len(amb)
        assert k - len(amb) <= len(sure) <= k - 1
        # the fp64 order itself passes the check the GPU output is put to
        LR.check_selection(LR.select_order(keys[r:r + 1], k)[0], keys[r], k)
        assert torch.equal(LR.coords_to_index(coords[r], coords[r, sure]), sure)


def test_outside_case_ties_at_zero():
    """a third of the candidates have the key 0 exactly and nothing else lies within SELECT_TOL of 0, so for k up to that count
    the selection is exact: the first k of them by index"""
    oc = LR.OUTSIDE_CASE
    planes, coords = LR.select_problem(oc["hw"], oc["M"], oc["seed"], zeros=oc["zeros"])
    keys = LR.point_sample(planes, coords).abs()
    for r in range(LR.SELECT_ROWS):
        assert len(torch.unique(coords[r], dim=0)) == oc["M"]
        zero = torch.nonzero(keys[r] == 0).flatten()
        assert zero.tolist() == list(range(0, 3 * oc["zeros"], 3))
        assert int((keys[r] <= LR.SELECT_TOL).sum()) == oc["zeros"]
        for k in oc["ks"]:
            if k <= oc["zeros"]:
                assert LR.select_order(keys[r:r + 1], k)[0].tolist() == zero[:k].tolist()
            else:
                assert len(LR.select_bands(keys[r], k)[1]) <= LR.SELECT_MAX_AMBIGUOUS
