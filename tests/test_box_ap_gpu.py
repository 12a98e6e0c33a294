"""GPU: box AP on the device (mpf_seg_ap_match_box and mpf_seg_bits_boxes via mp_former_amd.inference.InstanceAP(iou_type="bbox"))
against the numpy restatement of pycocotools' bbIou and evaluateImg (tests/_box_restate.py) on the accumulate / summarize of
tests/_ap_restate.py.  Expected values never come from the code under test.  The image sizes, K = 4 and the "small" setting are
those of tests/golden/make_golden_ap.py: all four area ranges are populated and the truncation to max_dets happens."""
import functools

import numpy as np
import pytest
import torch

import _ap_restate as R
import _box_restate as X
from test_ap_cpu import assert_stats_equal

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
K = 4
SIZES = ((37, 50), (33, 56), (61, 83))
AREA_RNGS = [[0, 1e10], [0, 64], [64, 400], [400, 1e10]]
MAX_DETS = [1, 3, 5]
RULES = ("coco", "union")


def _np(t):
    return t.detach().cpu().numpy()


def _dev_bits(masks, size):
    masks = np.asarray(masks, dtype=bool).reshape((-1,) + tuple(size))
    return torch.from_numpy(R.pack_columns(masks).view(np.int64)).to(DEV)


def _shape(g, H, W, blob):
    """a seeded rectangle, with a blob (a few pixels dilated twice) attached in half of the cases"""
    h, w = int(g.integers(2, max(3, H // 2))), int(g.integers(2, max(3, W // 2)))
    if g.random() < 0.35:
        h, w = int(g.integers(2, 7)), int(g.integers(2, 7))          # the two lower ranges of the "small" setting
    y, x = int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1))
    m = np.zeros((H, W), dtype=bool)
    m[y:y + h, x:x + w] = True
    if blob:
        b = np.zeros((H, W), dtype=bool)
        b[min(H - 1, y + int(g.integers(0, h + 3))), min(W - 1, x + int(g.integers(0, w + 3)))] = True
        for _ in range(2):
            p = np.zeros((H + 2, W + 2), dtype=bool)
            p[1:-1, 1:-1] = b
            b = p[:-2, 1:-1] | p[2:, 1:-1] | p[1:-1, :-2] | p[1:-1, 2:] | p[1:-1, 1:-1]
        m |= b
    return m


@functools.lru_cache(maxsize=None)
def _scenes():
    """five images: the three sizes, then one without detections and one without ground truths.  -> [(size, dts, gts)] with dense
    "mask"s; every image with ground truths has a crowd; the detections are shifted copies of the ground truths (many IoUs), some
    unrelated shapes, and score ties"""
    g = np.random.default_rng(20240607)
    out, did, gid = [], 0, 0
    for n, (H, W) in enumerate(SIZES + SIZES[:2]):
        gts, dts = [], []
        for j in range(0 if n == 4 else 9):
            gid += 1
            crowd = int(j == 0)
            m = _shape(g, H, W, blob=bool(j % 2))
            if crowd:
                m[H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = True
            gts.append({"id": gid, "category": int(0 if j < 3 else g.integers(0, 3)), "iscrowd": crowd, "mask": m})
        src = [x["mask"] for x in gts] or [_shape(g, H, W, False) for _ in range(4)]
        cats = [x["category"] for x in gts] or [0, 1, 1, 2]
        for j in range(0 if n == 3 else 16):
            did += 1
            if j < 12:
                k = j % len(src)
                m = np.roll(src[k], (int(g.integers(-2, 3)), int(g.integers(-2, 3))), (0, 1))
                cat = cats[k] if g.random() < 0.85 else int(g.integers(0, K))
            else:
                m, cat = _shape(g, H, W, blob=bool(j % 2)), int(g.integers(0, K))
            score = float(np.float32(np.round(g.random(), 1 if j % 3 == 0 else 4)))
            if j == 1 and gts:                           # one exact copy at the top: a true positive at every threshold
                m, cat, score = src[1], cats[1], float(np.float32(0.97))
            dts.append({"id": did, "category": cat, "score": score, "mask": m})
        out.append(((H, W), dts, gts))
    return out


def _images(route, seed=5):
    """the scenes as the restatement takes them.  "bits": boxes = those of the masks, a ground truth's area its pixel count;
    "float": the same boxes moved and resized by non-integer amounts, a ground truth's area w * h"""
    g = np.random.default_rng(seed)
    images = []
    for size, dts, gts in _scenes():
        sides = []
        for items in (dts, gts):
            boxes = X.xyxy_to_xywh(X.boxes_of(np.stack([x["mask"] for x in items]))) if items else np.zeros((0, 4))
            if route == "float":
                boxes = boxes + g.random(boxes.shape) * [1.5, 1.5, 2.0, 2.0] - [0.75, 0.75, 0.5, 0.5]
            sides.append(boxes)
        nd = [dict(d, box=b, area=float(b[2]) * float(b[3])) for d, b in zip(dts, sides[0])]
        ng = [dict(x, box=b, area=float(x["mask"].sum()) if route == "bits" else float(b[2]) * float(b[3])) for x, b in zip(gts, sides[1])]
        images.append((nd, ng))
    return images


@functools.lru_cache(maxsize=None)
def _want(route, rule):
    return X.expected(_images(route), K, AREA_RNGS, MAX_DETS, R.IOU_THRS, rule)


def _ap(rule, iou_type="bbox"):
    from mp_former_amd.inference import InstanceAP
    return InstanceAP(K, area_rngs=AREA_RNGS, max_dets=MAX_DETS, crowd_rule=rule, device=DEV, iou_type=iou_type)


def _fields(dts, gts):
    return (torch.tensor([d["score"] for d in dts], dtype=torch.float32).to(DEV), [d["category"] for d in dts],
            [x["category"] for x in gts], [x["iscrowd"] for x in gts])


def test_the_scenes_cover_what_the_issue_asks_for():
    scenes = _scenes()
    assert [s[0] for s in scenes[:3]] == list(SIZES)
    assert all(any(x["iscrowd"] for x in gts) for _, _, gts in scenes if gts)
    assert not scenes[3][1] and scenes[3][2] and scenes[4][1] and not scenes[4][2]
    per = {}
    for n, (_, dts, _) in enumerate(scenes):
        for d in dts:
            per[n, d["category"]] = per.get((n, d["category"]), 0) + 1
    assert max(per.values()) > MAX_DETS[-1], "no truncation"
    for route in ("bits", "float"):
        stats, summary = _want(route, "coco")
        assert (stats["npig"].sum(0) > 0).all(), "a range holds no ground truth"
        m, ig = stats["matched"][:, 0], stats["ignored"][:, 0]
        tp, fp = (m & ~ig).any(0), (~m & ~ig).any(0)
        # the masks' boxes hold unshifted copies (IoU 1); the moved float boxes reach the lower thresholds only
        assert (tp.all() if route == "bits" else tp[:3].all()) and fp.all(), "a threshold without a true or a false positive"
        assert (m & ig).any(), "no detection matched to a crowd"
        assert (~stats["matched"] & stats["ignored"]).any(), "no unmatched detection ignored through its area"
        assert summary[1] > 0 and summary[8] > 0
    fl = np.concatenate([d["box"] for d in _images("float")[0][0]])
    assert (fl != np.round(fl)).all()
    assert not np.array_equal(_want("bits", "coco")[0]["matched"], _want("bits", "union")[0]["matched"]), "the crowd rules agree"


@pytest.mark.parametrize("rule", RULES)
def test_boxes_derived_from_the_bits(rule):
    stats_want, summary_want = _want("bits", rule)
    ap = _ap(rule)
    for (size, dts, gts), (nd, ng) in zip(_scenes(), _images("bits")):
        sc, cl, gc, cr = _fields(dts, gts)
        ap.update(_dev_bits([d["mask"] for d in dts], size), sc, cl, _dev_bits([x["mask"] for x in gts], size), gc, cr, size=size)
    assert_stats_equal(ap.stats(), stats_want, f"bits {rule}")
    np.testing.assert_allclose(ap.summarize(), summary_want, rtol=0, atol=1e-12)


@pytest.mark.parametrize("rule", RULES)
def test_float_boxes_passed_in(rule):
    stats_want, summary_want = _want("float", rule)
    ap = _ap(rule)
    for n, (nd, ng) in enumerate(_images("float")):
        sc, cl, gc, cr = _fields(nd, ng)
        db = np.stack([d["box"] for d in nd]) if nd else np.zeros((0, 4))
        gb = np.stack([x["box"] for x in ng]) if ng else np.zeros((0, 4))
        if n % 2:                                        # device tensors, and host arrays
            db, gb = torch.from_numpy(db).to(DEV), torch.from_numpy(gb).to(DEV)
        ap.update(None, sc, cl, None, gc, cr, dt_boxes=db, gt_boxes=gb)
    assert_stats_equal(ap.stats(), stats_want, f"float {rule}")
    np.testing.assert_allclose(ap.summarize(), summary_want, rtol=0, atol=1e-12)
    from mp_former_amd import _lib
    assert "seg_ap_match_kernel<box>" in _lib.last_kernel()


def test_mixed_sides_and_given_areas():
    """detections from bits against given ground-truth boxes with given areas"""
    images = _images("float")
    bits_images = _images("bits")
    mixed = [([dict(d) for d in bd], [dict(x, area=float(7 * i + 3)) for i, x in enumerate(fg)])
             for (bd, _), (_, fg) in zip(bits_images, images)]
    stats_want, _ = X.expected(mixed, K, AREA_RNGS, MAX_DETS, R.IOU_THRS, "coco")
    ap = _ap("coco")
    for (size, dts, gts), (nd, ng) in zip(_scenes(), mixed):
        sc, cl, gc, cr = _fields(dts, gts)
        gb = np.stack([x["box"] for x in ng]) if ng else np.zeros((0, 4))
        ap.update(_dev_bits([d["mask"] for d in dts], size), sc, cl, None, gc, cr, gt_areas=[x["area"] for x in ng], size=size, gt_boxes=gb)
    assert_stats_equal(ap.stats(), stats_want, "mixed")


@pytest.mark.parametrize("rule", RULES)
def test_equal_iou_takes_the_later_ground_truth(rule):
    """a 4 x 4 detection over two 2 x 4 ground truths: both IoUs are 8 / 16 = the first threshold exactly.  It takes the later one,
    so the second detection, which is that ground truth's own box and misses the other, finds it taken at 0.5 and free above."""
    dt = np.array([[0, 0, 4, 4], [2, 0, 2, 4]], dtype=np.float64)
    gt = np.array([[0, 0, 2, 4], [2, 0, 2, 4]], dtype=np.float64)
    assert X.bb_iou(dt, gt, [0, 0], rule).tolist() == [[0.5, 0.5], [0.0, 1.0]]
    ap = _ap(rule)
    ap.update(None, [0.9, 0.8], [1, 1], None, [1, 1], [0, 0], dt_boxes=dt, gt_boxes=gt)
    got = ap.stats()
    assert got["matched"][0, 0].tolist() == [True] + [False] * 9
    assert got["matched"][1, 0].tolist() == [False] + [True] * 9
    dts = [{"id": i + 1, "category": 1, "score": s, "box": dt[i], "area": 16.0 if i == 0 else 8.0} for i, s in enumerate((0.9, 0.8))]
    gts = [{"id": i + 1, "category": 1, "iscrowd": 0, "box": gt[i], "area": 8.0} for i in range(2)]
    assert_stats_equal(got, X.expected([(dts, gts)], K, AREA_RNGS, MAX_DETS, R.IOU_THRS, rule)[0], "tie")


@pytest.mark.parametrize("rule", RULES)
def test_no_operation_of_the_iou_is_contracted(rule):
    """ten non-integer pairs whose IoU changes in the last bit when gw * gh + dw * dh or (...) - w * h becomes a fused multiply-add,
    each against a threshold that sits on the larger of the two values (tests/test_box_abi_cpu.py pins that the two arithmetics
    decide differently there): the records are those of the separately rounded operations"""
    from mp_former_amd.inference import InstanceAP
    dts, gts, thrs = X.contraction_scene()
    n = len(dts)
    ev = X.evaluate([(dts, gts)], n, [[0, 1e10]], (1, 10, 100), thrs, rule)
    want = R.expected_stats([(dts, gts)], n, [[0, 1e10]], (1, 10, 100), thrs, rule, eval_imgs=ev)
    on_own = want["matched"][np.arange(n), 0, np.arange(n)]
    assert on_own.any() and not on_own.all()
    ap = InstanceAP(n, iou_thrs=thrs, area_rngs=[[0, 1e10]], crowd_rule=rule, device=DEV, iou_type="bbox")
    ap.update(None, [d["score"] for d in dts], [d["category"] for d in dts], None, [x["category"] for x in gts], [0] * n,
              dt_boxes=np.stack([d["box"] for d in dts]), gt_boxes=np.stack([x["box"] for x in gts]))
    got = ap.stats()
    np.testing.assert_array_equal(got["matched"][np.arange(n), 0, np.arange(n)], on_own)
    assert_stats_equal(got, want, f"contraction {rule}")


@pytest.mark.parametrize("rule", RULES)
def test_filled_rectangles_score_the_same_as_masks(rule):
    """needs no restatement: the mask of an axis-aligned filled rectangle is its box, so "bbox" and "segm" give the same records"""
    g = np.random.default_rng(11)
    box_ap, mask_ap = _ap(rule, "bbox"), _ap(rule, "segm")
    for H, W in SIZES:
        def rects(n):
            out = []
            for _ in range(n):
                h, w = int(g.integers(1, H // 2)), int(g.integers(1, W // 2))
                out.append((int(g.integers(0, H - h + 1)), int(g.integers(0, W - w + 1)), h, w))
            return out

        def fill(rs):
            ms = np.zeros((len(rs), H, W), dtype=bool)
            for m, (y, x, h, w) in zip(ms, rs):
                m[y:y + h, x:x + w] = True
            return ms
        gr = rects(8)
        moved = [(min(y + 1, H - h), max(x - 2, 0), h, w) for y, x, h, w in gr]        # still whole rectangles inside the image
        gm, dm = fill(gr), fill(gr[:1] + moved[1:] + rects(6))
        args = (_dev_bits(dm, (H, W)), torch.from_numpy(g.random(len(dm)).astype(np.float32)).to(DEV), g.integers(0, 2, len(dm)),
                _dev_bits(gm, (H, W)), g.integers(0, 2, len(gm)), [1] + [0] * (len(gm) - 1))
        box_ap.update(*args, size=(H, W))
        mask_ap.update(*args, size=(H, W))
    got, want = box_ap.stats(), mask_ap.stats()
    assert_stats_equal(got, want, rule)
    assert got["matched"].any() and got["ignored"].any() and not got["matched"].all()


def test_bbox_update_makes_no_device_to_host_copy():
    size, dts, gts = _scenes()[0]
    ap = _ap("coco")
    sc, cl, gc, cr = _fields(dts, gts)
    args = (_dev_bits([d["mask"] for d in dts], size), sc, torch.tensor(cl).to(DEV), _dev_bits([x["mask"] for x in gts], size), gc, cr)
    ap.update(*args, size=size)                          # warm: buffers allocated
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ap.update(*args, size=size)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert len(ap.stats()["scores"]) == 2 * len(dts)


def test_bbox_argument_checks():
    size, dts, gts = _scenes()[0]
    sc, cl, gc, cr = _fields(dts, gts)
    db, gb = _dev_bits([d["mask"] for d in dts], size), _dev_bits([x["mask"] for x in gts], size)
    ap = _ap("coco")
    with pytest.raises(ValueError, match="size"):
        ap.update(db, sc, cl, gb, gc, cr)
    with pytest.raises(ValueError, match="dt_boxes or dt_bits"):
        ap.update(None, sc, cl, gb, gc, cr, size=size)
    with pytest.raises(ValueError, match="dt_boxes"):
        ap.update(db, sc, cl, gb, gc, cr, size=size, dt_boxes=np.zeros((len(dts) + 1, 4)))
    with pytest.raises(ValueError, match="bbox"):
        _ap("coco", "segm").update(db, sc, cl, gb, gc, cr, dt_boxes=np.zeros((len(dts), 4)))
    assert ap._images == 0 and ap._n == 0, "nothing was recorded"
