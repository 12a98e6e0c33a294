"""GPU: panoptic quality on the device (csrc/seg_pq.hip via mp_former_amd.inference.PanopticQuality) against the numpy restatement
of the reference's per-image arithmetic (tests/_pq_restate.py, itself checked against the reference's function in
tests/test_pq_cpu.py).  Expected values never come from the code under test.  tp / fp / fn must be equal and iou must be equal as
float64 bits."""
import numpy as np
import pytest
import torch

import _pq_restate as R
from test_infer_cpu import load_infer
from test_pq_cpu import assert_stats_equal, load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _pq(K, things=(), void_id=0):
    from mp_former_amd.inference import PanopticQuality
    return PanopticQuality(K, things, void_id=void_id, device=DEV)


def _dev_gt(gt, rgb):
    if rgb:
        return torch.from_numpy(R.id2rgb(gt)).to(DEV)
    return torch.from_numpy(np.asarray(gt, dtype=np.int32)).to(DEV)


def _dev_pred(pred):
    return torch.from_numpy(np.asarray(pred, dtype=np.int32)).to(DEV)


def _check(gt, pred, gts, preds, K, rgb, tag=""):
    """one image through a fresh object -> (device stats, expected stats), compared"""
    want = R.pq_single(gt, pred, gts, preds, K, 0)
    q = _pq(K)
    q.update(_dev_pred(pred), preds, _dev_gt(gt, rgb), gts)
    got = q.stats()
    assert_stats_equal(got, want, tag)
    assert got["tp"].dtype == np.int64 and got["iou"].dtype == np.float64
    return got


# ---- 1. the golden of the reference's own function, semantic route --------------------------------------------------------------
def test_golden_semantic_route():
    K, ignore, images = load_golden()
    q = _pq(K, void_id=ignore)
    for rerun in range(2):
        for n, im in enumerate(images):
            gt = torch.from_numpy(im["gt"]).to(DEV)
            q.update_semantic(torch.from_numpy(im["pred"]).to(DEV), gt if n != 1 else gt.to(torch.int64))
            assert_stats_equal(q.stats(), im["sum"], f"run {rerun}, after image {n}")
        q.reset()
        assert not any(q.stats()[k].any() for k in ("tp", "fp", "fn", "iou"))
    # one image alone, uint8 ground truth
    q.update_semantic(torch.from_numpy(images[2]["pred"]).to(DEV), torch.from_numpy(images[2]["gt"].astype(np.uint8)).to(DEV))
    assert_stats_equal(q.stats(), images[2]["single"], "image 2 alone")


# ---- 2. constructed panoptic cases ------------------------------------------------------------------------------------------------
def _scene(hw=(6, 10)):
    return np.zeros(hw, dtype=np.int64), np.zeros(hw, dtype=np.int64)


def _seg(i, c, crowd=None):
    return {"id": i, "category_id": c} if crowd is None else {"id": i, "category_id": c, "iscrowd": crowd}


def case_iou_exactly_half():
    gt, pred = _scene()
    gt[0, 0:3] = 7                   # area 3
    pred[0, 1:4] = 1                 # area 3, intersection 2; pred[0, 3] lies on another gt segment, not on VOID
    gt[0, 3] = 9
    return gt, pred, [_seg(7, 0, 0), _seg(9, 1, 0)], [_seg(1, 0)], 2, {"tp": [0, 0], "fp": [1, 0], "fn": [1, 1]}


def case_void_overlap_lifts_over_half():
    gt, pred = _scene()
    gt[0, 0:4] = 7                   # area 4
    gt[1, 0:2] = 9                   # pred pixels on another segment
    pred[0, 1:4] = 1                 # intersection 3
    pred[1, 0:2] = 1                 # 2 on gt 9: union 4 + 5 - 3 = 6 -> 0.5, no match ...
    g2, p2 = gt.copy(), pred.copy()
    g2[1, 0:2] = 0                   # ... and on VOID instead: union 4 + 5 - 3 - 2 = 4 -> 0.75
    return (gt, pred, [_seg(7, 0, 0), _seg(9, 1, 0)], [_seg(1, 0)], 2, {"tp": [0, 0], "fp": [1, 0], "fn": [1, 1]}), \
           (g2, p2, [_seg(7, 0, 0)], [_seg(1, 0)], 2, {"tp": [1, 0], "fp": [0, 0], "fn": [0, 0]})


def case_equal_iou_other_category():
    gt, pred = _scene()
    gt[2:4, 2:6] = 5
    pred[2:4, 2:6] = 3
    return gt, pred, [_seg(5, 0, 0)], [_seg(3, 1)], 2, {"tp": [0, 0], "fp": [0, 1], "fn": [1, 0]}


def case_fp_void_share():
    gt, pred = _scene()
    gt[0:2, 0:4] = 4                 # category 1: never matches the category-0 predictions
    pred[1, 2:6] = 1                 # area 4: 2 on gt 4, 2 on VOID -> share exactly 0.5: counted
    pred[3, 0:5] = 2                 # area 5 on VOID with ...
    gt[3, 0:2] = 4                   # ... 2 pixels on gt 4: share 3 / 5: skipped
    return gt, pred, [_seg(4, 1, 0)], [_seg(1, 0), _seg(2, 0)], 2, {"tp": [0, 0], "fp": [1, 0], "fn": [0, 1]}


def case_two_crowds_annotation_order():
    gt, pred = _scene()
    gt[0, 0:4] = 50                  # crowd, listed FIRST
    gt[2, 0:4] = 20                  # crowd, listed LAST: it is the one the reference keeps, although its id is the smaller
    gt[4, 0:6] = 30                  # a plain segment under both predictions' remaining pixels
    pred[0, 0:4] = 1
    pred[4, 0:2] = 1                 # pred 1: 4 of 6 on crowd 50 (not the winner): counted
    pred[2, 0:4] = 2
    pred[4, 2:4] = 2                 # pred 2: 4 of 6 on crowd 20 (the winner): skipped
    gts = [_seg(50, 0, 1), _seg(30, 1, 0), _seg(20, 0, 1)]
    return gt, pred, gts, [_seg(1, 0), _seg(2, 0)], 2, {"tp": [0, 0], "fp": [1, 0], "fn": [0, 1]}


def case_listed_gt_without_pixels():
    gt, pred = _scene()
    gt[1:3, 1:5] = 3
    pred[1:3, 1:5] = 1
    return gt, pred, [_seg(3, 0, 0), _seg(8, 1, 0)], [_seg(1, 0)], 2, {"tp": [1, 0], "fp": [0, 0], "fn": [0, 1]}


def case_large_ids_and_table_ends():
    """ids above 65536 (all three RGB bytes in use) and matches on the smallest and the largest id of both tables; the tables are
    not contiguous, so this is the binary search"""
    gt, pred = _scene((8, 12))
    gids = [3, 65537, 70001, 16777215]
    pids = [2, 900, 40000, 16000000]
    for n, (g, p) in enumerate(zip(gids, pids)):
        gt[2 * n, 0:6] = g
        pred[2 * n, 0:6] = p
    pred[2, 0:6] = 0                 # the second pair does not overlap: a hole in the middle
    pred[3, 0:6] = 900
    gt[3, 0:6] = 12345               # (on an unlisted id, not on VOID: the prediction counts)
    gts = [_seg(g, n % 3, 0) for n, g in enumerate(gids)]
    preds = [_seg(p, n % 3) for n, p in enumerate(pids)]
    return gt, pred, gts, preds, 3, {"tp": [2, 0, 1], "fp": [0, 1, 0], "fn": [0, 1, 0]}


def case_unlisted_gt_id():
    gt, pred = _scene()
    gt[0:2, 0:4] = 333               # not listed and not VOID: no discount for the prediction on it
    gt[3, 0:4] = 6
    pred[0:2, 0:4] = 1
    pred[3, 0:4] = 2
    return gt, pred, [_seg(6, 0, 0)], [_seg(1, 0), _seg(2, 0)], 1, {"tp": [1], "fp": [1], "fn": [0]}


def case_no_prediction_kept():
    gt, pred = _scene()
    gt[0:2, 0:4] = 5
    gt[3, 0:4] = 6
    return gt, pred, [_seg(5, 0, 0), _seg(6, 1, 0), _seg(9, 1, 1)], [], 2, {"tp": [0, 0], "fp": [0, 0], "fn": [1, 1]}


def case_no_ground_truth():
    gt, pred = _scene()
    gt[0, 0:3] = 77                  # unlisted
    pred[0, 0:4] = 1                 # 3 unlisted + 1 VOID: counted
    pred[2, 0:4] = 2                 # all on VOID: skipped
    return gt, pred, [], [_seg(1, 0), _seg(2, 1)], 2, {"tp": [0, 0], "fp": [1, 0], "fn": [0, 0]}


CASES = {
    "iou_exactly_half": case_iou_exactly_half,
    "void_overlap_below": lambda: case_void_overlap_lifts_over_half()[0],
    "void_overlap_lifts": lambda: case_void_overlap_lifts_over_half()[1],
    "equal_iou_other_category": case_equal_iou_other_category,
    "fp_void_share": case_fp_void_share,
    "two_crowds_annotation_order": case_two_crowds_annotation_order,
    "listed_gt_without_pixels": case_listed_gt_without_pixels,
    "large_ids_and_table_ends": case_large_ids_and_table_ends,
    "unlisted_gt_id": case_unlisted_gt_id,
    "no_prediction_kept": case_no_prediction_kept,
    "no_ground_truth": case_no_ground_truth,
}


@pytest.mark.parametrize("rgb", [False, True], ids=["int32", "rgb"])
@pytest.mark.parametrize("name", list(CASES))
def test_constructed_panoptic_cases(name, rgb):
    gt, pred, gts, preds, K, by_hand = CASES[name]()
    assert gt.shape[0] <= 16 and gt.shape[1] <= 24
    want = R.pq_single(gt, pred, gts, preds, K, 0)
    for k, v in by_hand.items():             # the case is what its name says (restatement against the count worked out by hand)
        assert want[k].tolist() == v, (name, k, want[k])
    _check(gt, pred, gts, preds, K, rgb, name)


# ---- 3. shapes: odd sizes, several workgroups' worth of runs, both table forms ---------------------------------------------------
def _blocky(g, hw, values, cell):
    H, W = hw
    small = g.choice(values, size=((H + cell - 1) // cell, (W + cell - 1) // cell))
    return np.kron(small, np.ones((cell, cell), dtype=np.int64))[:H, :W]


def _random_image(hw, nseg, K, seed, contiguous_pred):
    """gt: nseg segments (random ids up to 2^24, some crowd, some VOID); prediction: the same partition with blocks moved to other
    segments and to VOID, so that some pairs match, some miss and some predictions lie on VOID / crowd."""
    g = np.random.default_rng(seed)
    index = _blocky(g, hw, np.arange(nseg + 1), 3 if nseg > 100 else 5)                 # 0 = VOID
    gid = np.concatenate(([0], np.sort(g.choice(np.arange(1, 1 << 24), size=nseg, replace=False))))
    pid = np.arange(nseg + 1) if contiguous_pred else np.concatenate(([0], np.sort(g.choice(np.arange(1, 1 << 24), size=nseg, replace=False))))
    cat = np.arange(nseg + 1) % K
    crowd = g.random(nseg + 1) < 0.1
    pindex = index.copy()
    move = _blocky(g, hw, np.array([0, 0, 0, 1]), 2).astype(bool)
    pindex[move] = _blocky(g, hw, np.arange(nseg + 1), 4)[move]
    gt, pred = gid[index], pid[pindex]
    order = g.permutation(np.arange(1, nseg + 1))                                          # annotation order != id order
    gts = [_seg(int(gid[i]), int(cat[i]), int(crowd[i])) for i in order]
    present = [i for i in np.unique(pindex) if i != 0]
    preds = [_seg(int(pid[i]), int(cat[i])) for i in g.permutation(present)]
    return gt, pred, gts, preds


@pytest.mark.parametrize("rgb", [False, True], ids=["int32", "rgb"])
@pytest.mark.parametrize("hw,nseg,contiguous,variant", [((61, 83), 40, True, "lds"), ((97, 131), 40, False, "lds"),
                                                         ((61, 83), 200, False, "global"), ((97, 131), 200, True, "global")])
def test_random_shapes_and_both_table_forms(hw, nseg, contiguous, variant, rgb):
    from mp_former_amd import _lib
    K = 7
    gt, pred, gts, preds = _random_image(hw, nseg, K, seed=hw[0] + nseg, contiguous_pred=contiguous)
    assert (len(gts) + 2) * (nseg + 2) * 4 > 128 * 1024 or variant == "lds"
    _lib.profile_enable(True)
    try:
        got = _check(gt, pred, gts, preds, K, rgb, f"{hw} {nseg}")
        torch.cuda.synchronize()
        n_variant = _lib.profile_get(f"seg_pq_pairs_kernel<{variant}>")[0]
        n_all = _lib.profile_get("seg_pq_pairs_kernel")[0]
        n_match = _lib.profile_get("seg_pq_match_kernel")[0]
    finally:
        _lib.profile_enable(False)
    assert n_variant == n_all == 1 and n_match == 1, (n_variant, n_all, n_match)
    assert _lib.last_kernel() == "seg_pq_match_kernel"
    assert got["tp"].sum() > 0 and got["fp"].sum() > 0 and got["fn"].sum() > 0, "the image exercises all three counters"


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------
def test_unlisted_prediction_raises_at_stats_and_reset_clears_it():
    gt, pred, gts, preds, K, _ = case_fp_void_share()
    q = _pq(K)
    q.update(_dev_pred(pred), preds[:1], _dev_gt(gt, False), gts)                  # id 2 is in the map and not listed
    with pytest.raises(ValueError, match="segments_info"):
        q.stats()
    q.reset()
    q.update(_dev_pred(pred), preds + [_seg(9, 1)], _dev_gt(gt, False), gts)       # id 9 is listed and has no pixel
    with pytest.raises(ValueError, match="segments_info"):
        q.stats()
    q.reset()
    q.update(_dev_pred(pred), preds, _dev_gt(gt, True), gts)
    assert_stats_equal(q.stats(), R.pq_single(gt, pred, gts, preds, K, 0))
    # the semantic route: a predicted label that is no class
    s = _pq(3, void_id=255)
    lab = torch.tensor([[0, 1, 2, 7], [0, 1, 2, 2]], dtype=torch.int32, device=DEV)
    s.update_semantic(lab, lab.clamp(max=2))
    with pytest.raises(ValueError):
        s.stats()
    s.reset()
    s.update_semantic(lab.clamp(max=2), lab)                                          # a gt label that is no class is fine
    want = R.pq_single_semantic(lab.cpu().numpy(), lab.clamp(max=2).cpu().numpy(), 3, 255)
    assert_stats_equal(s.stats(), want)


# ---- 5. update never synchronises -------------------------------------------------------------------------------------------------
def test_updates_do_not_synchronise():
    K = 7
    a = _random_image((61, 83), 40, K, seed=1, contiguous_pred=True)
    b = _random_image((61, 83), 40, K, seed=2, contiguous_pred=False)
    sem_p = torch.from_numpy((a[1] % K).astype(np.int32)).to(DEV)
    sem_g = torch.from_numpy((b[1] % K).astype(np.int32)).to(DEV)
    dev = [(_dev_pred(x[1]), x[3], _dev_gt(x[0], rgb), x[2]) for x, rgb in ((a, False), (b, True))]
    q, s = _pq(K), _pq(K, void_id=255)
    for args in dev:                                                                  # warm: scratch, counters, LDS attribute
        q.update(*args)
    s.update_semantic(sem_p, sem_g)
    q.reset()
    s.reset()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for args in dev:
            q.update(*args)
        s.update_semantic(sem_p, sem_g)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    want = R.add_stats(R.pq_single(a[0], a[1], a[2], a[3], K, 0), R.pq_single(b[0], b[1], b[2], b[3], K, 0))
    assert_stats_equal(q.stats(), want)
    assert_stats_equal(s.stats(), R.pq_single_semantic(b[1] % K, a[1] % K, K, 255))


# ---- 6. end to end: postprocess -> update -----------------------------------------------------------------------------------------
def test_postprocess_result_goes_straight_into_update():
    from mp_former_amd.inference import postprocess
    z, cfg, padded = load_infer("infer_all")
    K = cfg.num_classes
    res = postprocess(torch.from_numpy(z["pred_logits"]).to(DEV), torch.from_numpy(z["pred_masks"]).to(DEV), z["image_sizes"], padded,
                      z["output_sizes"], cfg)
    q = _pq(K, cfg.thing_ids)
    total = R.zero_stats(K)
    for n in range(len(res)):
        fid = z[f"f32_{n}_pan_ids"].astype(np.int64)
        fseg = [_seg(int(i), int(c)) for i, _, c in z[f"f32_{n}_pan_segments"].tolist()]
        # ground truth: the fixture's own segments shifted by two columns under new ids, a VOID band on top, and one segment of a
        # class nobody predicts
        gt = np.roll(fid, 2, axis=1) * 1000
        gt[:3] = 0
        gt[-4:, :9] = 77
        gts = [_seg(s["id"] * 1000, s["category_id"], 0) for s in fseg] + [_seg(77, K - 1, 0)]
        ids, info = res[n]["panoptic_seg"]
        assert ids.is_cuda and ids.dtype == torch.int32
        q.update(ids, info, _dev_gt(gt, n == 0), gts)
        total = R.add_stats(total, R.pq_single(gt, fid, gts, fseg, K, 0))
    assert total["tp"].sum() > 0 and total["fn"].sum() > 0
    assert_stats_equal(q.stats(), total)
    r = q.results()
    assert set(r) == {"PQ", "SQ", "RQ", "PQ_th", "SQ_th", "RQ_th", "PQ_st", "SQ_st", "RQ_st"} and 0 < r["PQ"] <= 100


# ---- 7. accumulation and combine ---------------------------------------------------------------------------------------------------
def test_accumulation_and_combine_of_two_half_runs():
    from mp_former_amd.inference import PanopticQuality
    K = 7
    images = [_random_image((33, 47), 12, K, seed=10 + n, contiguous_pred=bool(n % 2)) for n in range(5)]
    singles = [R.pq_single(gt, pred, gts, preds, K, 0) for gt, pred, gts, preds in images]

    def run(subset, rgb):
        q = _pq(K)
        for gt, pred, gts, preds in subset:
            q.update(_dev_pred(pred), preds, _dev_gt(gt, rgb), gts)
        return q.stats()

    def seq(parts):
        t = R.zero_stats(K)
        for p in parts:
            t = R.add_stats(t, p)
        return t
    full = run(images, False)
    assert_stats_equal(full, seq(singles), "five updates")
    halves = [run(images[:3], True), run(images[3:], False)]
    assert_stats_equal(halves[0], seq(singles[:3]))
    assert_stats_equal(halves[1], seq(singles[3:]))
    both = PanopticQuality.combine(halves)
    for k in ("tp", "fp", "fn"):
        np.testing.assert_array_equal(both[k], full[k])
    assert both["iou"].tobytes() == (seq(singles[:3])["iou"] + seq(singles[3:])["iou"]).tobytes()
    # against the full run only the order of the five additions differs: each rounds by at most eps / 2 of a partial sum that is
    # no larger than the total (every term is positive), so the two totals are within 5 eps of each other
    np.testing.assert_allclose(both["iou"], full["iou"], rtol=5 * np.finfo(np.float64).eps, atol=0)
