"""GPU: Boundary AP on the device (csrc/seg_boundary.hip and mpf_seg_ap_match_boundary via mp_former_amd.inference: mask_boundaries,
InstanceAP(iou_type="boundary"); d2_plugin.InstanceAPEvaluator(iou_types=...)) against the numpy restatement of boundary-iou-api
(tests/_boundary_restate.py, itself held to scipy in tests/test_boundary_ap_cpu.py) driving the restatement of the COCO evaluation
(tests/_ap_restate.py).  Expected values never come from the code under test.  Everything is compared for equality: packed words,
booleans, ranks, and float64 arrays as bits."""
import functools

import numpy as np
import pytest
import torch

import _ap_restate as R
import _boundary_restate as B
from test_ap_cpu import assert_stats_equal, bits, load_golden
from test_boundary_ap_cpu import DS, SHAPES, make_mask

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _words(t):
    return _np(t).view(np.uint64)


def _dev_bits(masks):
    """numpy's packing, on the device: the inputs do not depend on pack_masks"""
    return torch.from_numpy(R.pack_columns(masks).view(np.int64)).to(DEV)


@functools.lru_cache(maxsize=None)
def _case_masks(H, W):
    """the masks of one shape, made once: empty, all ones, density 0.5, blobs, density 0.9"""
    return {"empty": np.zeros((H, W), dtype=bool), "ones": make_mask("ones", H, W, 0), "half": make_mask("half", H, W, H * 100 + W),
            "blobs": make_mask("blobs", H, W, H * 100 + W + 1), "dense": make_mask("dense", H, W, H * 100 + W + 2)}


@functools.lru_cache(maxsize=None)
def _want_words(H, W, kind, d):
    """the restatement's boundary of one mask as packed words, computed once and shared"""
    return R.pack_columns(B.mask_to_boundary(_case_masks(H, W)[kind], d)[None])[0]


def _check(got, H, W, kinds, d):
    assert got.dtype == torch.int64 and tuple(got.shape) == (len(kinds), (H * W + 63) // 64) and got.device == DEV
    want = np.stack([_want_words(H, W, k, d) for k in kinds])
    np.testing.assert_array_equal(_words(got), want, err_msg=f"{H}x{W} d={d} {kinds}")
    _, tail = R.unpack_columns(_np(got), H, W)
    assert not tail.any(), "bits at or past H * W must be zero"


# ---- 1. mask_boundaries -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda o: f"{o[0]}x{o[1]}")
def test_mask_boundaries_equal_the_restatement(hw, M):
    """word-aligned and unaligned columns, H = 1, W = 1, H * W % 64 != 0; d beyond H, beyond W and beyond one word"""
    from mp_former_amd.inference import mask_boundaries
    H, W = hw
    groups = [("empty",), ("ones",), ("half",), ("blobs",)] if M == 1 else [("empty", "ones", "half"), ("blobs", "dense", "half")]
    for kinds in groups:
        dev = _dev_bits(np.stack([_case_masks(H, W)[k] for k in kinds]))
        for d in DS:
            _check(mask_boundaries(dev, (H, W), d=d), H, W, kinds, d)
    # a d past every window, and the ratio form
    _check(mask_boundaries(dev, (H, W), d=10 ** 6), H, W, kinds, max(H, W))      # no window fits: the boundary is the mask
    _check(mask_boundaries(dev, (H, W), dilation_ratio=0.05), H, W, kinds, B.boundary_dilation(H, W, 0.05))
    _check(mask_boundaries(dev, (H, W)), H, W, kinds, B.boundary_dilation(H, W, 0.02))


@pytest.mark.parametrize("H,W,d", [(257, 300, 9), (96, 1030, 5)], ids=["257x300", "96x1030"])
def test_mask_boundaries_across_column_bands(H, W, d):
    """A band is max(64, 4 d) columns rounded up to the 64 / gcd(H, 64) columns after which the stream is on a word again: 64 columns
    in both cases (quantum 64 for H = 257, 2 for H = 96), so 257 x 300 takes 5 bands and 96 x 1030 takes 17, the last one partial,
    with every band edge inside the image and the halo of d columns read from the neighbours."""
    from mp_former_amd.inference import mask_boundaries
    kinds = ("blobs", "dense", "ones")
    dev = _dev_bits(np.stack([_case_masks(H, W)[k] for k in kinds]))
    before = dev.clone()
    _check(mask_boundaries(dev, (H, W), d=d), H, W, kinds, d)
    assert torch.equal(dev, before), "the input was modified"
    assert _want_words(H, W, "dense", d).any() and (_want_words(H, W, "blobs", d) != R.pack_columns(_case_masks(H, W)["blobs"][None])[0]).any()


def _box_erode(m, d):
    """the separable box form by running sums (held to the restatement below, and to scipy in the CPU tests): for the large images"""
    L = 2 * d + 1
    H, W = m.shape
    p = np.zeros((H + 2 * d, W + 2 * d), dtype=np.int32)
    p[d:d + H, d:d + W] = m
    c = np.concatenate([np.zeros((1, p.shape[1]), dtype=np.int32), np.cumsum(p, axis=0, dtype=np.int32)])
    ty = ((c[L:] - c[:-L]) == L).astype(np.int32)
    c = np.concatenate([np.zeros((H, 1), dtype=np.int32), np.cumsum(ty, axis=1, dtype=np.int32)], axis=1)
    return (c[:, L:] - c[:, :-L]) == L


def _rectangles(H, W, seed, n=12):
    g = np.random.default_rng(seed)
    m = np.zeros((H, W), dtype=bool)
    for _ in range(n):
        h, w = int(g.integers(H // 8, H // 2)), int(g.integers(W // 8, W // 2))
        y, x = int(g.integers(-h // 2, H - h // 2)), int(g.integers(-w // 2, W - w // 2))
        m[max(0, y):y + h, max(0, x):x + w] = True
    m &= g.random((H, W)) < 0.99999                      # a few one-pixel holes: each opens a (2d+1)-square
    return m


@pytest.mark.parametrize("H,W,d", [(1024, 1024, 29), (2000, 3000, 72), (769, 726, 362)], ids=["1024x1024", "2000x3000", "769x726-direct"])
def test_mask_boundaries_of_large_images(H, W, d):
    """1024 x 1024 (d of ratio 0.02; 16 words per column, 9 bands), 2000 x 3000 (d of ratio 0.02; 32 words per column x 320 columns
    x 2 buffers = the whole 160 KiB of LDS, 18 bands) and a d whose halo does not fit the LDS with any band (13 words x (724 + 64)
    columns x 2 > 160 KiB): the direct kernel."""
    from mp_former_amd.inference import mask_boundaries
    if d != 362:
        m = _rectangles(H, W, H + d)
    else:
        m = np.ones((H, W), dtype=bool)
        m[762, 725] = False                             # of the 2 x 45 pixels with a whole window, those with x = 363, y >= 400 lose it
        small = _case_masks(61, 83)["dense"]
        np.testing.assert_array_equal(_box_erode(small, 2), B.erode(small, 2))
    er = _box_erode(m, d)
    assert er.any() and (m & ~er).any()
    if d == 362:
        assert int(er.sum()) == 2 * 45 - 7
    got = mask_boundaries(_dev_bits(m[None]), (H, W), d=d)
    np.testing.assert_array_equal(_words(got), R.pack_columns((m & ~er)[None]))


def test_mask_boundaries_of_a_view_and_of_no_mask():
    from mp_former_amd.inference import mask_boundaries
    H, W, kinds = 37, 50, ("half", "blobs", "dense")
    wide = torch.zeros((3, 2 * ((H * W + 63) // 64)), dtype=torch.int64, device=DEV)
    view = wide[:, ::2]                                  # not contiguous
    view.copy_(_dev_bits(np.stack([_case_masks(H, W)[k] for k in kinds])))
    before = wide.clone()
    _check(mask_boundaries(view, (H, W), d=2), H, W, kinds, 2)
    assert torch.equal(wide, before), "the input was modified"
    empty = mask_boundaries(view[:0], (H, W))
    assert tuple(empty.shape) == (0, (H * W + 63) // 64) and empty.dtype == torch.int64 and empty.device == DEV


# ---- 2. the smaller of the two IoUs, through the count-driven entry -----------------------------------------------------------------
def _match_counts(mask, bnd, crowd, rule):
    """one detection, one ground truth, counts (inter, area_d, area_g) of the masks and of the boundaries -> matched, ignored [Tn]"""
    from mp_former_amd import _lib
    from mp_former_amd.inference import AP_CROWD_RULES
    i32 = lambda v: torch.tensor([v], dtype=torch.int32, device=DEV)       # noqa: E731
    thrs = np.linspace(.5, 0.95, 10)
    settings = torch.from_numpy(np.concatenate([thrs, [0.0, 1e10]])).to(DEV)
    m, b = [i32(v) for v in mask], [i32(v) for v in bnd]
    score, cat, gcat, gcrowd = torch.tensor([0.5], device=DEV), i32(0), i32(0), i32(crowd)
    garea = torch.tensor([float(mask[2])], dtype=torch.float64, device=DEV)
    rec = torch.full((1, 4), -1, dtype=torch.int64, device=DEV)
    npig = torch.zeros(1, dtype=torch.int64, device=DEV)
    ws = torch.zeros(16, dtype=torch.uint8, device=DEV)
    _lib.call("mpf_seg_ap_match_boundary", DEV, m[0].data_ptr(), m[1].data_ptr(), m[2].data_ptr(), b[0].data_ptr(), b[1].data_ptr(),
              b[2].data_ptr(), 1, 1, score.data_ptr(), cat.data_ptr(), gcat.data_ptr(), gcrowd.data_ptr(), garea.data_ptr(),
              settings.data_ptr(), 10, settings.data_ptr() + 80, 1, 1, 100, AP_CROWD_RULES[rule], 0, rec.data_ptr(), npig.data_ptr(),
              ws.data_ptr(), ws.numel(), _lib.stream_ptr(DEV))
    r = _np(rec).view(np.uint64)[0]
    assert int(_np(npig)[0]) == (0 if crowd else 1)
    unpack = lambda w: np.array([(int(w) >> t) & 1 for t in range(10)], dtype=bool)      # noqa: E731
    return unpack(r[2]), unpack(r[3]), thrs


@pytest.mark.parametrize("rule", ["coco", "union"])
def test_the_smaller_of_the_two_ious_is_matched(rule):
    nine, six = (9, 9, 10), (6, 6, 10)                  # inter, area_d, area_g: 9 / 10 and 6 / 10
    for mask, bnd in ((nine, six), (six, nine)):
        matched, ignored, thrs = _match_counts(mask, bnd, 0, rule)
        assert matched.tolist() == [True] * 3 + [False] * 7 and not ignored.any(), (mask, bnd, matched)
        np.testing.assert_array_equal(matched, thrs <= 6 / 10)
    both, _, _ = _match_counts(nine, nine, 0, rule)
    assert both.tolist() == [True] * 9 + [False]         # the test above is the min, not a property of either set of counts
    # a crowd ground truth: "coco" divides each intersection by the detection's own count, "union" by the plain union
    a, b = (9, 10, 20), (6, 10, 12)
    for mask, bnd in ((a, b), (b, a)):
        matched, ignored, thrs = _match_counts(mask, bnd, 1, rule)
        want = min(9 / 10, 6 / 10) if rule == "coco" else min(9 / (10 + 20 - 9), 6 / (10 + 12 - 6))
        np.testing.assert_array_equal(matched, thrs <= want, err_msg=f"{rule} {mask} {bnd}")
        np.testing.assert_array_equal(ignored, matched)  # matched to a crowd: ignored; unmatched: area 10 or 6 is inside the range
        assert matched.any() == (rule == "coco")
    none, _, _ = _match_counts((0, 9, 10), nine, 0, rule)
    assert not none.any()                                # an intersection of 0 is an IoU of 0


# ---- 3. the golden scenes -----------------------------------------------------------------------------------------------------------
def _update(ap, dts, gts, pack_gt=False, areas=True, counts=False, **kw):
    """one image into ``ap``; masks packed by numpy (or the ground truth by pack_masks)"""
    from mp_former_amd.inference import mask_pair_counts, pack_masks
    shape = (dts + gts)[0]["mask"].shape
    dm = np.stack([d["mask"] for d in dts]) if dts else np.zeros((0,) + shape, dtype=bool)
    gm = np.stack([x["mask"] for x in gts]) if gts else np.zeros((0,) + shape, dtype=bool)
    gt_bits = pack_masks(torch.from_numpy(gm.astype(np.uint8)).to(DEV)) if pack_gt else _dev_bits(gm)
    dt_bits = _dev_bits(dm)
    if counts:
        kw["pair_counts"] = mask_pair_counts(dt_bits, gt_bits)
    ap.update(dt_bits, torch.tensor([d["score"] for d in dts], dtype=torch.float32).to(DEV),
              torch.tensor([d["category"] for d in dts], dtype=torch.int64).to(DEV), gt_bits,
              [x["category"] for x in gts], np.asarray([x["iscrowd"] for x in gts], dtype=np.int64),
              np.asarray([x["area"] for x in gts], dtype=np.float64) if areas else None, **kw)


@functools.lru_cache(maxsize=None)
def _golden_want(ratio, rule, name):
    """the restatement's records after each image, and its accumulate / summarize of all: computed once per setting"""
    g = load_golden()
    s = g[name]
    with B.patched(ratio):
        after = [R.expected_stats(g["images"][:n + 1], g["K"], s["area_rngs"], s["max_dets"], g["iou_thrs"], rule)
                 for n in range(len(g["images"]))]
        ev = R.evaluate(g["images"], g["K"], s["area_rngs"], s["max_dets"], g["iou_thrs"], rule)
    acc = R.accumulate(ev, g["K"], len(g["images"]), s["area_rngs"], s["max_dets"], g["iou_thrs"], g["rec_thrs"])
    return after, acc, R.summarize(acc, s["max_dets"], g["iou_thrs"])


@pytest.mark.parametrize("rule", ["union", "coco"])
@pytest.mark.parametrize("name", ["coco", "small"])
@pytest.mark.parametrize("ratio", [0.02, 0.1])
def test_golden_scenes_image_by_image(ratio, name, rule):
    from mp_former_amd.inference import InstanceAP
    g = load_golden()
    s = g[name]
    after, acc_want, stats_want = _golden_want(ratio, rule, name)
    ap = InstanceAP(g["K"], area_rngs=s["area_rngs"], max_dets=s["max_dets"], crowd_rule=rule, device=DEV, iou_type="boundary",
                    dilation_ratio=ratio)
    for rerun in range(2):
        for n, (dts, gts) in enumerate(g["images"]):
            _update(ap, dts, gts, pack_gt=(n == 1), areas=(rule == "coco"), size=g["sizes"][n])
            assert_stats_equal(ap.stats(), after[n], f"run {rerun}, after image {n}")
        acc = ap.accumulate()
        for k in ("precision", "recall", "scores"):
            assert bits(acc[k]) == bits(acc_want[k]), k
        assert bits(ap.summarize()) == bits(stats_want)
        ap.reset()
    mask_only = R.expected_stats(g["images"], g["K"], s["area_rngs"], s["max_dets"], g["iou_thrs"], rule)
    assert not np.array_equal(mask_only["matched"], after[-1]["matched"]), "these scenes tell the two scores apart"


def test_segm_records_are_unchanged_and_pair_counts_are_taken():
    from mp_former_amd.inference import InstanceAP
    g = load_golden()
    s = g["coco"]
    mk = lambda t: InstanceAP(g["K"], area_rngs=s["area_rngs"], max_dets=s["max_dets"], device=DEV, iou_type=t)      # noqa: E731
    plain, sized, counted, bnd, bnd_counted = mk("segm"), mk("segm"), mk("segm"), mk("boundary"), mk("boundary")
    for n, (dts, gts) in enumerate(g["images"]):
        _update(plain, dts, gts)
        _update(sized, dts, gts, size=g["sizes"][n])                    # a size does not change the mask score
        _update(counted, dts, gts, counts=True)
        _update(bnd, dts, gts, size=g["sizes"][n])
        _update(bnd_counted, dts, gts, size=g["sizes"][n], counts=True)
    want = R.expected_stats(g["images"], g["K"], s["area_rngs"], s["max_dets"], g["iou_thrs"], "coco")
    for ap in (plain, sized, counted):
        assert_stats_equal(ap.stats(), want)
    assert_stats_equal(bnd_counted.stats(), bnd.stats())
    assert_stats_equal(bnd.stats(), _golden_want(0.02, "coco", "coco")[0][-1])
    with pytest.raises(ValueError, match="pair_counts"):
        dts, gts = g["images"][0]
        _update(plain, dts, gts, pair_counts=(torch.zeros((1, 1), dtype=torch.int32, device=DEV),) * 3)


def test_boundary_update_makes_no_device_to_host_copy():
    from mp_former_amd.inference import InstanceAP
    g = load_golden()
    ap = InstanceAP(g["K"], device=DEV, iou_type="boundary")
    dts, gts = g["images"][0]
    dm, gm = _dev_bits(np.stack([d["mask"] for d in dts])), _dev_bits(np.stack([x["mask"] for x in gts]))
    sc = torch.tensor([d["score"] for d in dts], dtype=torch.float32).to(DEV)
    cl = torch.tensor([d["category"] for d in dts]).to(DEV)
    gc, cr = [x["category"] for x in gts], [x["iscrowd"] for x in gts]
    ap.update(dm, sc, cl, gm, gc, cr, size=g["sizes"][0])               # warm: buffers allocated
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ap.update(dm, sc, cl, gm, gc, cr, size=g["sizes"][0])
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert len(ap.stats()["scores"]) == 2 * len(dts)


# ---- 4. the evaluator ---------------------------------------------------------------------------------------------------------------
def test_evaluator_with_both_types_equals_two_separate_runs():
    from mp_former_amd.d2_plugin import InstanceAPEvaluator
    from mp_former_amd.inference import InstanceAP, instance_bits, pack_masks
    from test_ap_gpu import _fixture_scene
    z, cfg, padded, lg, mk, dense, images, gt_dev = _fixture_scene()
    K = cfg.num_classes
    packed = instance_bits(lg, mk, z["image_sizes"], padded, z["output_sizes"], cfg)
    outputs = [dense[0], {"instances": packed[-1]}]                     # one image as dense masks, one as packed bits
    inputs = [{"instances": gt_dev[0]}, {"instances": gt_dev[-1]}]
    ev = InstanceAPEvaluator(K, device=DEV, iou_types=("segm", "boundary"))
    ev.reset()
    ev.process(inputs, outputs)
    got = ev.evaluate()
    assert list(got) == ["segm", "boundary"]
    for t in ("segm", "boundary"):
        ap = InstanceAP(K, device=DEV, iou_type=t)
        for i in (0, -1):
            b, gt = packed[i], gt_dev[i]
            ap.update(b["bits"], b["scores"], b["pred_classes"], pack_masks(gt.gt_masks.tensor), gt.gt_classes, gt.gt_iscrowd,
                      size=tuple(b["size"]))
        assert_stats_equal(ev.aps[t].stats(), ap.stats(), t)
        want = ap.results()
        assert got[t].keys() == want.keys()
        for k, v in want.items():
            assert got[t][k] == v or (np.isnan(v) and np.isnan(got[t][k])), (t, k)
    # the boundary score of this scene against the restatement, and below the mask score
    two = [images[0], images[-1]]
    with B.patched(0.02):
        want = R.expected_stats(two, K, R.COCO_AREA_RNGS, (1, 10, 100))
    assert_stats_equal(ev.aps["boundary"].stats(), want)
    assert got["boundary"]["AP"] <= got["segm"]["AP"] and got["segm"]["AP"] > 0
    only = InstanceAPEvaluator(K, device=DEV)                           # the default: the mask score alone, the same numbers
    only.process(inputs, outputs)
    alone = only.evaluate()
    assert set(alone) == {"segm"}
    for k, v in got["segm"].items():
        assert alone["segm"][k] == v or (np.isnan(v) and np.isnan(alone["segm"][k])), k
