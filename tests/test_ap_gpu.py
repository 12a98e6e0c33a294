"""GPU: instance mask AP on the device (csrc/seg_ap.hip via mp_former_amd.inference: pack_masks, instance_bits, mask_pair_counts,
InstanceAP; d2_plugin.InstanceAPEvaluator) against numpy and the restatement of the reference's COCO evaluation
(tests/_ap_restate.py, itself held to the reference's own code in tests/test_ap_cpu.py).  Expected values never come from the code
under test.  Everything is compared for equality: packed words, integer counts, booleans, ranks, and float64 arrays as bits."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _ap_restate as R
from test_ap_cpu import assert_stats_equal, bits, golden_stats, load_golden
from test_infer_cpu import load_infer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


def _words(t):
    return _np(t).view(np.uint64)


def _dev_bits(masks):
    """numpy's packing, on the device: the inputs of the matching tests do not depend on pack_masks"""
    return torch.from_numpy(R.pack_columns(masks).view(np.int64)).to(DEV)


def _random_masks(g, M, H, W, p=0.5):
    m = g.random((M, H, W)) < p
    if M >= 1:
        m[0] = False                                    # an empty mask
    if M >= 2:
        m[1] = True                                     # a full mask
    if M >= 4:
        m[3] = m[2]                                     # two identical masks
    return m


# ---- 1. pack_masks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bool, torch.uint8, torch.float32], ids=["bool", "u8", "f32"])
@pytest.mark.parametrize("M", [1, 3])
@pytest.mark.parametrize("hw", [(1, 1), (1, 64), (7, 9), (64, 1), (37, 50), (65, 63)], ids=lambda o: f"{o[0]}x{o[1]}")
def test_pack_masks_equals_numpy(hw, M, dtype):
    from mp_former_amd.inference import pack_masks
    H, W = hw
    g = np.random.default_rng(H * 100 + W + M)
    m = g.random((M, H, W)) < 0.5
    if dtype == torch.float32:
        v = np.where(m, g.choice(np.array([-2.5, 1e-30, 1.0, 255.0], dtype=np.float32), size=m.shape), np.float32(0)).astype(np.float32)
        v[~m & (g.random(m.shape) < 0.5)] = -0.0        # minus zero is zero
    elif dtype == torch.uint8:
        v = np.where(m, g.integers(1, 256, size=m.shape), 0).astype(np.uint8)
    else:
        v = m
    got = pack_masks(torch.from_numpy(v).to(DEV))
    assert got.dtype == torch.int64 and tuple(got.shape) == (M, (H * W + 63) // 64) and got.device == DEV
    np.testing.assert_array_equal(_words(got), R.pack_columns(m))
    back, tail = R.unpack_columns(_np(got), H, W)
    np.testing.assert_array_equal(back, m)
    assert not tail.any(), "bits at or past H * W must be zero"


def test_pack_masks_of_a_view_and_of_no_mask():
    from mp_former_amd.inference import pack_masks
    g = np.random.default_rng(5)
    m = g.random((4, 9, 14)) < 0.5
    t = torch.from_numpy(m).to(DEV)
    np.testing.assert_array_equal(_words(pack_masks(t[:, 1:8, 2:11])), R.pack_columns(m[:, 1:8, 2:11]))    # not contiguous
    assert tuple(pack_masks(t[:0]).shape) == (0, 2)


# ---- 2. instance_bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["infer_instance", "infer_all"])
def test_instance_bits_equal_the_dense_masks_of_postprocess(name, variant):
    from mp_former_amd.inference import instance_bits, postprocess
    from test_infer_gpu import test_fixture_parity
    test_fixture_parity(name, variant)                  # postprocess itself still gives the reference's results
    z, cfg, padded = load_infer(name)
    lg = torch.from_numpy(z["pred_logits"]).to(DEV)
    mk = torch.from_numpy(z["pred_masks" if variant == "f32" else "pred_masks_bf16"]).to(DEV)
    if variant == "bf16":
        mk = mk.to(torch.bfloat16)
    dense = postprocess(lg, mk, z["image_sizes"], padded, z["output_sizes"], cfg)
    got = instance_bits(lg, mk, z["image_sizes"], padded, z["output_sizes"], cfg)
    assert len(got) == len(dense) and not cfg.instance_masks == "bits"
    for n, (d, b) in enumerate(zip(dense, got)):
        ins = d["instances"]
        H, W = (int(v) for v in z["output_sizes"][n])
        assert set(b) == {"bits", "size", "scores", "pred_classes"} and tuple(b["size"]) == (H, W)
        assert torch.equal(b["scores"], ins.scores) and torch.equal(b["pred_classes"], ins.pred_classes), (name, n)
        assert b["bits"].dtype == torch.int64 and tuple(b["bits"].shape) == (len(ins), (H * W + 63) // 64)
        back, tail = R.unpack_columns(_np(b["bits"]), H, W)
        np.testing.assert_array_equal(back, _np(ins.pred_masks) > 0.5, err_msg=f"{name}/{variant}/{n}")
        assert not tail.any() and len(ins) > 0
        np.testing.assert_array_equal(_words(b["bits"]), R.pack_columns(_np(ins.pred_masks)))


def test_instance_bits_with_no_instance_kept():
    from mp_former_amd.inference import InferenceConfig, instance_bits
    from test_infer_eval_gpu import IMAGE, OUT, PADDED, _inputs
    lg, mk = _inputs(19, 37, torch.float32)
    cfg = InferenceConfig(num_classes=19, num_queries=37, panoptic_on=True, thing_ids=frozenset())
    b = instance_bits(lg, mk, [IMAGE], PADDED, [OUT], cfg)[0]
    assert tuple(b["bits"].shape) == (0, (OUT[0] * OUT[1] + 63) // 64) and b["scores"].numel() == 0 and b["pred_classes"].numel() == 0


# ---- 3. mask_pair_counts ----------------------------------------------------------------------------------------------------------
def _pair_counts_numpy(a, b):
    n = a.shape[1] * a.shape[2]
    fa, fb = a.reshape(a.shape[0], n), b.reshape(b.shape[0], n)
    inter = fa.astype(np.float32) @ fb.astype(np.float32).T             # exact below 2^24 pixels
    return inter.astype(np.int32), fa.sum(1).astype(np.int32), fb.sum(1).astype(np.int32)


@pytest.mark.parametrize("T,G,hw", [(1, 1, (1, 1)), (3, 2, (7, 9)), (100, 1, (37, 50)), (1, 130, (33, 56)), (100, 130, (61, 83)),
                                    (100, 20, (480, 719)), (0, 5, (7, 9)), (4, 0, (7, 9)), (0, 0, (7, 9))],
                         ids=lambda v: "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v))
def test_mask_pair_counts_equal_numpy(T, G, hw):
    from mp_former_amd.inference import mask_pair_counts
    H, W = hw
    g = np.random.default_rng(T * 1000 + G)
    a, b = _random_masks(g, T, H, W, 0.4), _random_masks(g, G, H, W, 0.6)
    if T >= 5 and G >= 5:
        b[4] = a[4]                                     # identical across the two sides
    want = _pair_counts_numpy(a, b)
    da, db = _dev_bits(a), _dev_bits(b)
    for run in range(2):                                # the second call finds nothing of the first
        inter, area_a, area_b = mask_pair_counts(da, db)
        assert inter.dtype == area_a.dtype == area_b.dtype == torch.int32 and tuple(inter.shape) == (T, G)
        for got, w, what in zip((inter, area_a, area_b), want, ("inter", "area_a", "area_b")):
            np.testing.assert_array_equal(_np(got), w.reshape(got.shape), err_msg=f"run {run} {what}")
    if T and G:
        swapped = mask_pair_counts(db, da)
        np.testing.assert_array_equal(_np(swapped[0]), want[0].T)
        if hw == (1, 1):
            assert want[0].tolist() == [[0]] and _np(mask_pair_counts(db, db)[0]).tolist() == [[0]]
            full = _dev_bits(np.ones((1, 1, 1), dtype=bool))
            assert _np(mask_pair_counts(full, full)[0]).tolist() == [[1]]


# ---- 4. the golden scenes ---------------------------------------------------------------------------------------------------------
def _update(ap, dts, gts, pack_gt=False, areas=True, order=None):
    """one image into ``ap``; detections in the order given (or `order`), masks packed by numpy (or the ground truth by pack_masks)"""
    from mp_former_amd.inference import pack_masks
    if order is not None:
        dts = [dts[i] for i in order]
    shape = (dts + gts)[0]["mask"].shape
    dm = np.stack([d["mask"] for d in dts]) if dts else np.zeros((0,) + shape, dtype=bool)
    gm = np.stack([x["mask"] for x in gts]) if gts else np.zeros((0,) + shape, dtype=bool)
    gt_bits = pack_masks(torch.from_numpy(gm.astype(np.uint8)).to(DEV)) if pack_gt else _dev_bits(gm)
    ap.update(_dev_bits(dm), torch.tensor([d["score"] for d in dts], dtype=torch.float32).to(DEV),
              torch.tensor([d["category"] for d in dts], dtype=torch.int64).to(DEV), gt_bits,
              [x["category"] for x in gts], np.asarray([x["iscrowd"] for x in gts], dtype=np.int64),
              np.asarray([x["area"] for x in gts], dtype=np.float64) if areas else None)


@pytest.mark.parametrize("rule", ["union", "coco"])
@pytest.mark.parametrize("name", ["coco", "small"])
def test_golden_scenes_image_by_image(rule, name):
    from mp_former_amd.inference import InstanceAP
    g = load_golden()
    s, z = g[name], g[rule, name]
    ap = InstanceAP(g["K"], area_rngs=s["area_rngs"], max_dets=s["max_dets"], crowd_rule=rule, device=DEV)
    for rerun in range(2):
        for n, (dts, gts) in enumerate(g["images"]):
            _update(ap, dts, gts, pack_gt=(n == 1), areas=(rule == "coco"))     # the golden's areas are the pixel counts
            want = R.expected_stats(g["images"][:n + 1], g["K"], s["area_rngs"], s["max_dets"], g["iou_thrs"], rule)
            assert_stats_equal(ap.stats(), want, f"run {rerun}, after image {n}")
        got = ap.stats()
        assert_stats_equal(got, golden_stats(g, rule, name), "against the golden")
        acc = ap.accumulate()
        for k in ("precision", "recall", "scores"):
            assert bits(acc[k]) == bits(z[k]), k
        assert bits(ap.summarize()) == bits(z["stats"])
        ap.reset()
        assert ap.stats()["scores"].shape == (0,) and not ap.stats()["npig"].any()
    # one image alone, through a fresh object
    one = InstanceAP(g["K"], area_rngs=s["area_rngs"], max_dets=s["max_dets"], crowd_rule=rule, device=DEV)
    _update(one, *g["images"][2], areas=False)
    assert_stats_equal(one.stats(), golden_stats(g, rule, name, images=[2]), "image 2 alone")


def test_records_grow_by_doubling():
    from mp_former_amd.inference import InstanceAP
    g = load_golden()
    s = g["small"]
    ap = InstanceAP(g["K"], area_rngs=s["area_rngs"], max_dets=s["max_dets"], device=DEV)
    reps = 40                                           # 40 x 22 detections: past the first 256 records and the doubled 512
    for _ in range(reps):
        for dts, gts in g["images"]:
            _update(ap, dts, gts)
    got, one = ap.stats(), golden_stats(g, "coco", "small")
    n = len(one["scores"])
    assert len(got["scores"]) == reps * n and ap._rec.shape[0] >= reps * n
    for k in ("scores", "category", "rank", "matched", "ignored"):
        np.testing.assert_array_equal(got[k], np.concatenate([one[k]] * reps), err_msg=k)
    np.testing.assert_array_equal(got["image"], np.concatenate([one["image"] + 3 * r for r in range(reps)]))
    np.testing.assert_array_equal(got["npig"], one["npig"] * reps)


def test_update_makes_no_device_to_host_copy():
    from mp_former_amd.inference import InstanceAP
    g = load_golden()
    ap = InstanceAP(g["K"], device=DEV)
    dts, gts = g["images"][0]
    dm, gm = _dev_bits(np.stack([d["mask"] for d in dts])), _dev_bits(np.stack([x["mask"] for x in gts]))
    sc = torch.tensor([d["score"] for d in dts], dtype=torch.float32).to(DEV)
    cl = torch.tensor([d["category"] for d in dts]).to(DEV)
    gc, cr = [x["category"] for x in gts], [x["iscrowd"] for x in gts]
    ap.update(dm, sc, cl, gm, gc, cr)                   # warm: buffers allocated
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ap.update(dm, sc, cl, gm, gc, cr)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert len(ap.stats()["scores"]) == 2 * len(dts)


# ---- 5. constructed single-image cases --------------------------------------------------------------------------------------------
HW = (7, 29)            # 203 positions: odd H, no multiple of 64
SMALL_RNGS = [[0, 1e10], [0, 8], [8, 30], [30, 1e10]]


def _m(*runs):
    """a mask of row-major position runs (start, length)"""
    m = np.zeros(HW[0] * HW[1], dtype=bool)
    for s, n in runs:
        m[s:s + n] = True
    return m.reshape(HW)


def _dt(i, c, score, *runs):
    m = _m(*runs)
    return {"id": i, "category": c, "score": float(np.float32(score)), "mask": m, "area": float(m.sum())}


def _gt(i, c, crowd, *runs, area=None):
    m = _m(*runs)
    return {"id": i, "category": c, "iscrowd": crowd, "mask": m, "area": float(m.sum()) if area is None else float(area)}


def _case(dts, gts, K=2, rule="coco", rngs=SMALL_RNGS, max_dets=(1, 2, 100), order=None):
    """one image through a fresh object against the restatement -> the device stats, detections in score order"""
    from mp_former_amd.inference import InstanceAP
    ap = InstanceAP(K, area_rngs=rngs, max_dets=max_dets, crowd_rule=rule, device=DEV)
    if order is not None:
        dts = [dts[i] for i in order]
    _update(ap, dts, gts)
    got = ap.stats()
    assert_stats_equal(got, R.expected_stats([(dts, gts)], K, rngs, max_dets, R.IOU_THRS, rule))
    return got


@pytest.mark.parametrize("rule", ["coco", "union"])
def test_case_iou_exactly_on_each_threshold(rule):
    """category i: a ground truth of 20 pixels and a detection of 10 + i of them: IoU (10 + i) / 20 matches up to threshold i"""
    dts = [_dt(i + 1, i, 0.5, (20 * i, 10 + i)) for i in range(10)]
    gts = [_gt(i + 1, i, 0, (20 * i, 20)) for i in range(10)]
    got = _case(dts, gts, K=10, rule=rule)
    for i in range(10):
        row = got["matched"][list(got["category"]).index(i), 0]
        assert row[:i + 1].all() and not row[i + 1:].any(), (i, row)


def test_case_iou_one_and_the_empty_sides():
    got = _case([_dt(1, 0, 0.9, (5, 12))], [_gt(1, 0, 0, (5, 12))])
    assert got["matched"][0, 0].all() and not got["ignored"][0, 0].any() and got["npig"][0, 0] == 1     # min(t, 1 - 1e-10) lets 1.0 match
    got = _case([_dt(1, 0, 0.9, (5, 12)), _dt(2, 1, 0.8, (40, 3))], [])                                 # no ground truth
    assert not got["matched"].any() and not got["npig"].any() and got["ignored"][0, 1].all() and not got["ignored"][0, 2].any()
    got = _case([], [_gt(1, 0, 0, (5, 12)), _gt(2, 1, 1, (40, 9))])                                     # no detection
    assert got["scores"].shape == (0,) and got["npig"].tolist() == [[1, 0, 1, 0], [0, 0, 0, 0]]
    got = _case([_dt(1, 0, 0.9, (5, 12))], [_gt(1, 1, 0, (5, 12))])                                     # a category without detection
    assert not got["matched"].any() and got["npig"][1, 0] == 1 and got["npig"][0].sum() == 0


def test_case_crowd_only_and_a_crowd_matched_by_three():
    crowd = _gt(1, 0, 1, (0, 100))
    dts = [_dt(1, 0, 0.9, (0, 10)), _dt(2, 0, 0.8, (20, 12)), _dt(3, 0, 0.7, (95, 10)), _dt(4, 0, 0.6, (150, 9))]
    got = _case(dts, [crowd])
    assert got["npig"].sum() == 0
    assert got["matched"][:2, 0].all() and got["ignored"][:2, 0].all()           # inside the crowd: IoU = inter / own area = 1
    assert got["matched"][2, 0, 0] and not got["matched"][2, 0, 1]               # half inside: 0.5
    assert not got["matched"][3].any() and not got["ignored"][3, 0].any()        # outside: a plain false positive in "all"
    union = _case(dts, [crowd], rule="union")
    assert not union["matched"].any()                                            # the plain union: 10 / 100
    three = _case(dts[:2] + [_dt(5, 0, 0.75, (40, 15))], [crowd, _gt(2, 0, 0, (120, 20))])
    assert three["matched"][:, 0, 0].all() and three["ignored"][:, 0, 0].all() and three["npig"][0, 0] == 1


def test_case_break_rule_and_equal_iou():
    # detection 1: IoU 16/20 with the plain gt 1, and 18/20 of its own area inside the crowd listed after it
    dts = [_dt(1, 0, 0.9, (0, 20))]
    gts = [_gt(1, 0, 0, (4, 16)), _gt(2, 0, 1, (0, 18), (100, 40))]
    got = _case(dts, gts)
    assert got["matched"][0, 0, :7].all() and not got["ignored"][0, 0, :7].any()          # up to 0.8 the plain gt keeps it
    assert got["matched"][0, 0, 7:9].all() and got["ignored"][0, 0, 7:9].all()            # above, the crowd takes it (0.9)
    assert not got["matched"][0, 0, 9]
    # the crowd listed FIRST is still visited last
    assert_stats_equal(_case(dts, gts[::-1]), got)
    # two ground truths with the same pixels: the later one wins, the next detection gets the other
    same = [_gt(1, 0, 0, (30, 10)), _gt(2, 0, 0, (30, 10), area=100)]
    got = _case([_dt(1, 0, 0.9, (30, 10)), _dt(2, 0, 0.8, (30, 10))], same)
    # in the range [8, 30] gt 2 (area 100) is ignored: visited last, after a match on gt 1 the loop stops there
    assert got["matched"][:, 0].all() and not got["ignored"][:, 0].any()
    assert got["matched"][:, 2].all() and not got["ignored"][0, 2].any() and got["ignored"][1, 2].all()
    assert not got["ignored"][0, 3].any() and got["ignored"][1, 3].all()                  # in [30, 1e10] the roles swap, the outcome stays


def test_case_max_det_ties_and_unsorted_scores():
    gts = [_gt(1, 0, 0, (0, 10)), _gt(2, 0, 0, (20, 10)), _gt(3, 0, 0, (40, 10)), _gt(4, 1, 0, (60, 10))]
    dts = [_dt(1, 0, 0.5, (0, 10)), _dt(2, 0, 0.7, (20, 10)), _dt(3, 1, 0.7, (60, 10)), _dt(4, 0, 0.7, (40, 10)), _dt(5, 0, 0.5, (100, 10)),
           _dt(6, 1, 0.9, (120, 4))]
    got = _case(dts, gts, max_dets=(1, 2, 3))
    assert got["scores"].tolist() == [np.float32(v) for v in (0.9, 0.7, 0.7, 0.7, 0.5, 0.5)]
    assert got["category"].tolist() == [1, 0, 1, 0, 0, 0] and got["rank"].tolist() == [0, 0, 1, 1, 2, 3]    # ties keep the input order
    assert got["matched"][4, 0].all() and not got["matched"][5].any() and not got["ignored"][5].any()       # the fourth of category 0 is dropped
    other = _case(dts, gts, max_dets=(1, 2, 3), order=[4, 0, 5, 3, 2, 1])
    assert other["rank"].tolist() == [0, 0, 1, 1, 2, 3] and not other["matched"][4:].any()      # now detection 1 is the one dropped
    assert not other["ignored"][4, 0].any()                                                        # and detection 5 a false positive
    acc_in = {**got}
    from mp_former_amd.inference import InstanceAP
    ap = InstanceAP(2, area_rngs=SMALL_RNGS, max_dets=(1, 2, 3))
    ev = R.evaluate([(dts, gts)], 2, SMALL_RNGS, (1, 2, 3))
    want = R.accumulate(ev, 2, 1, SMALL_RNGS, (1, 2, 3))
    for k in ("precision", "recall", "scores"):
        assert bits(ap.accumulate(acc_in)[k]) == bits(want[k]), k


def test_case_gt_areas_move_a_ground_truth_across_a_range_edge():
    dts = [_dt(1, 0, 0.9, (0, 10))]
    by_pixels = _case(dts, [_gt(1, 0, 0, (0, 10))])                   # 10 pixels: in [8, 30]
    assert by_pixels["npig"][0].tolist() == [1, 0, 1, 0] and not by_pixels["ignored"][0, 2].any() and by_pixels["ignored"][0, 1].all()
    moved = _case(dts, [_gt(1, 0, 0, (0, 10), area=7.5)])             # the annotation says 7.5: in [0, 8]
    assert moved["npig"][0].tolist() == [1, 1, 0, 0] and not moved["ignored"][0, 1].any() and moved["ignored"][0, 2].all()
    edge = _case(dts, [_gt(1, 0, 0, (0, 10), area=8.0)])              # on the edge: in both
    assert edge["npig"][0].tolist() == [1, 1, 1, 0]


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------
def _fixture_scene(n_gt=6, shift=2):
    """the infer_instance fixture through postprocess, and a ground truth made of its first predictions shifted by `shift` pixels"""
    from mp_former_amd.inference import postprocess
    z, cfg, padded = load_infer("infer_instance")
    lg, mk = torch.from_numpy(z["pred_logits"]).to(DEV), torch.from_numpy(z["pred_masks"]).to(DEV)
    dense = postprocess(lg, mk, z["image_sizes"], padded, z["output_sizes"], cfg)
    images, gt_dev = [], []
    for n, d in enumerate(dense):
        ins = d["instances"]
        pm, sc, cl = _np(ins.pred_masks) > 0.5, _np(ins.scores), _np(ins.pred_classes)
        dts = [{"id": i + 1, "category": int(cl[i]), "score": float(sc[i]), "mask": pm[i], "area": float(pm[i].sum())} for i in range(len(sc))]
        pick = [i for i in range(len(sc)) if pm[i].any()][:n_gt]
        gm = np.stack([np.roll(pm[i], (shift * (j % 3), shift * (j % 2)), (0, 1)) for j, i in enumerate(pick)])     # the first: a copy
        gts = [{"id": j + 1, "category": int(cl[i]), "iscrowd": int(j == 1), "mask": gm[j], "area": float(gm[j].sum())}
               for j, i in enumerate(pick)]
        images.append((dts, gts))
        gt_dev.append(SimpleNamespace(gt_masks=SimpleNamespace(tensor=torch.from_numpy(gm).to(DEV)),
                                      gt_classes=torch.tensor([x["category"] for x in gts]), gt_iscrowd=[x["iscrowd"] for x in gts]))
    return z, cfg, padded, lg, mk, dense, images, gt_dev


def test_end_to_end_on_the_fixture_logits():
    from mp_former_amd.d2_plugin import InstanceAPEvaluator
    from mp_former_amd.inference import InstanceAP, instance_bits, pack_masks
    z, cfg, padded, lg, mk, dense, images, gt_dev = _fixture_scene()
    K = cfg.num_classes
    ap = InstanceAP(K, device=DEV)
    for b, gt in zip(instance_bits(lg, mk, z["image_sizes"], padded, z["output_sizes"], cfg), gt_dev):
        ap.update(b["bits"], b["scores"], b["pred_classes"], pack_masks(gt.gt_masks.tensor), gt.gt_classes, gt.gt_iscrowd)
    ev = R.evaluate(images, K, R.COCO_AREA_RNGS, (1, 10, 100))
    want = R.accumulate(ev, K, len(images), R.COCO_AREA_RNGS, (1, 10, 100))
    assert_stats_equal(ap.stats(), R.expected_stats(images, K, R.COCO_AREA_RNGS, (1, 10, 100), eval_imgs=ev))
    acc = ap.accumulate()
    for k in ("precision", "recall", "scores"):
        assert bits(acc[k]) == bits(want[k]), k
    stats = R.summarize(want, (1, 10, 100))
    assert bits(ap.summarize()) == bits(stats) and stats[0] > 0 and stats[8] > 0
    res = ap.results()
    assert res["AP"] == float(stats[0] * 100) and res["AP50"] == float(stats[1] * 100)
    # the evaluator: dense predictions as postprocess returns them, and the packed form of instance_bits
    inputs = [{"instances": gt} for gt in gt_dev]
    e1 = InstanceAPEvaluator(K, device=DEV)
    e1.reset()
    e1.process(inputs, dense)
    e2 = InstanceAPEvaluator(K, device=DEV)
    e2.process(inputs, [{"instances": b} for b in instance_bits(lg, mk, z["image_sizes"], padded, z["output_sizes"], cfg)])
    r1, r2 = e1.evaluate(), e2.evaluate()
    assert set(r1) == {"segm"} and r1["segm"].keys() == res.keys()
    for k, v in res.items():
        for r in (r1, r2):
            assert r["segm"][k] == v or (np.isnan(v) and np.isnan(r["segm"][k])), k
    e1.reset()
    assert all(np.isnan(v) for v in e1.evaluate()["segm"].values())


# ---- 7. memory and route ----------------------------------------------------------------------------------------------------------
def test_memory_and_kernels_of_the_bits_route():
    from mp_former_amd import _lib
    from mp_former_amd.inference import InferenceConfig, InstanceAP, instance_bits, pack_masks, postprocess
    from test_infer_gpu import _coco_inputs
    K, T, H, W = 80, 100, 256, 256
    logits, masks = _coco_inputs(K, hw=(64, 64), seed=3)
    lg, mk = logits.to(DEV), masks.to(DEV)
    cfg = InferenceConfig(num_classes=K)
    g = np.random.default_rng(1)
    gt = torch.from_numpy(np.kron(g.random((20, 16, 16)) < 0.3, np.ones((16, 16), dtype=bool)).astype(bool)).to(DEV)
    gt_cls = torch.from_numpy(g.integers(0, K, 20)).to(DEV)
    crowd = torch.zeros(20, dtype=torch.int32, device=DEV)
    ap = InstanceAP(K, device=DEV)

    def native():
        b = instance_bits(lg, mk, [(H, W)], (H, W), [(H, W)], cfg)[0]
        ap.update(b["bits"], b["scores"], b["pred_classes"], pack_masks(gt), gt_cls, crowd)
        return b

    def peak(fn):
        fn()                                            # warm: scratch and record buffers allocated
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        r = fn()
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        del r
        return p
    p_native = peak(native)
    p_dense = peak(lambda: postprocess(lg, mk, [(H, W)], (H, W), [(H, W)], cfg))
    print(f"peak increase: bits route {p_native / 2**20:.2f} MiB, dense masks {p_dense / 2**20:.2f} MiB")
    assert p_native < T * H * W, (p_native, T * H * W)
    assert p_dense >= 4 * T * H * W
    _lib.profile_enable(True)
    try:
        native()
        torch.cuda.synchronize()
        n = {k: _lib.profile_get(k)[0] for k in ("seg_instance_kernel", "seg_instance_scores", "seg_rle_bits_kernel", "seg_rle_count_kernel",
                                                 "seg_pack_masks_kernel", "seg_mask_pairs_kernel", "seg_ap_match_kernel")}
    finally:
        _lib.profile_enable(False)
    assert n["seg_instance_kernel"] == 0, "the dense-mask pass ran on the bits route"
    assert n["seg_instance_scores"] == 1 and n["seg_rle_bits_kernel"] == 1 and n["seg_rle_count_kernel"] == 0
    assert n["seg_pack_masks_kernel"] == 1 and n["seg_mask_pairs_kernel"] == 1 and n["seg_ap_match_kernel"] == 1
