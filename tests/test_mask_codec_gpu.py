"""GPU: COCO ground truth decoded on the device (csrc/seg_codec.hip via mp_former_amd.inference.polygon_bits / rle_bits /
segmentation_bits / unpack_masks / polygon_masks, and the "annotations" / "segmentations" branches of the d2_plugin evaluators)
against the plain Python restatement of pycocotools' rleFrPoly / rleMerge / rleDecode (tests/_codec_restate.py, pinned to tables in
tests/test_mask_codec_cpu.py), packed by numpy (tests/_ap_restate.pack_columns).  Everything is integer equality."""
import functools

import numpy as np
import pytest
import torch

import _ap_restate as R
import _codec_restate as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# the shapes of tests/test_mask_boxes_gpu.py: many columns per word; a column is exactly one word; every column straddles a word
# boundary; the tail word partly past H * W; a column spans three words; more words (1057) than the fill workgroup has threads; and
# more (4137) than four times that
SHAPES = [(5, 7), (64, 3), (65, 4), (37, 50), (130, 9), (130, 520), (257, 1030)]
# random rings per shape: 4 x 520 = 2080 at the small shapes, where the host restatement is quick
N_RANDOM = {(5, 7): 520, (64, 3): 520, (65, 4): 520, (37, 50): 520, (130, 9): 60, (130, 520): 16, (257, 1030): 8}
SMALL = SHAPES[:4]


def _np(t):
    return t.detach().cpu().numpy()


def _words(t):
    return _np(t).view(np.uint64)


def _random_rings(H, W, n, g):
    rings = []
    for i in range(n):
        k = int(g.integers(3, 9))
        xy = g.uniform([-3, -3], [W + 3, H + 3], size=(k, 2))
        if i % 3 == 1:
            xy = np.round(xy)                                # integer vertices
        elif i % 3 == 2:
            xy = np.round(xy * 2) / 2                        # half-integer vertices
        rings.append(xy.reshape(-1).tolist())
    return rings


def _special_rings(H, W):
    """name -> ring"""
    return {
        "on 0, W, H": [0, 0, W, 0, W, H, 0, H],
        "outside, above left": [-3, -3, -1, -3, -1, -1],
        "outside, right": [W + 1, 0, W + 3, 0, W + 3, H, W + 1, H],
        "outside, below": [0, H + 0.5, W, H + 0.5, W / 2, H + 3],
        "covering": [-3, -3, W + 3, -3, W + 3, H + 3, -3, H + 3],
        "repeated vertices": [1, 1, 1, 1, W - 1, 1, W - 1, 1, W - 1, H - 1, W - 1, H - 1, 1, H - 1],
        "collinear": [0, 0, W / 2, H / 2, W, H],
        "zero area, there and back": [1, 1, W - 1, H - 2, 1, 1],
        "one point three times": [2, 1, 2, 1, 2, 1],
        "bow-tie": [0, 0, W, H, W, 0, 0, H],
        "star": [W / 2, 0, W * 0.8, H, 0, H * 0.4, W, H * 0.4, W * 0.2, H],
        "left half, on the border": [0, 0, W / 2, 0, W / 2, H, 0, H],
        "negative to inside": [-2.5, -1.5, W / 2 + 0.25, H / 3, 1.5, H + 2.5],
    }


@functools.lru_cache(maxsize=None)
def _polygon_scene(H, W):
    """-> (names, objects as polygon_bits takes them, expected uint64 [M, nwords]) of one shape, made once"""
    g = np.random.default_rng(H * 1000 + W)
    names, objs = [], []
    for i, ring in enumerate(_random_rings(H, W, N_RANDOM[(H, W)], g)):
        names.append(f"random #{i} {ring}")
        objs.append([ring])
    for name, ring in _special_rings(H, W).items():
        names.append(name)
        objs.append([ring])
    a = [1, 1, W * 0.7, 1, W * 0.7, H * 0.7, 1, H * 0.7]
    b = [W * 0.4, H * 0.4, W - 0.5, H * 0.4, W - 0.5, H - 0.5, W * 0.4, H - 0.5]
    d1, d2, d3 = [0, 0, W / 3, 0, 0, H / 3], [W / 2, 0, W, 0, W, H / 3], [0, H / 2 + 1, W, H, 0, H]
    for name, obj in (("two overlapping rings", [a, b]), ("two overlapping rings, swapped", [b, a]), ("three disjoint rings", [d1, d2, d3]),
                      ("three disjoint rings, reordered", [d3, d1, d2]), ("no ring", []), ("a ring twice", [a, a]),
                      ("one ring after the empty entry", [b])):
        names.append(name)
        objs.append(obj)
    dense = np.stack([C.poly_mask(obj, H, W) for obj in objs])
    return tuple(names), objs, R.pack_columns(dense), dense


@pytest.mark.parametrize("hw", SHAPES, ids=lambda o: f"{o[0]}x{o[1]}")
def test_polygon_bits_equal_the_restatement(hw):
    from mp_former_amd import _lib
    from mp_former_amd.inference import polygon_bits, polygon_masks, unpack_masks
    H, W = hw
    names, objs, want, dense = _polygon_scene(H, W)
    i = names.index
    assert dense[i("on 0, W, H")].all() and dense[i("covering")].all() and not dense[i("outside, right")].any()
    assert not dense[i("outside, above left")].any() and not dense[i("one point three times")].any() and not dense[i("no ring")].any()
    np.testing.assert_array_equal(dense[i("two overlapping rings")], dense[i("two overlapping rings, swapped")])
    np.testing.assert_array_equal(dense[i("a ring twice")], C.poly_mask(objs[i("a ring twice")][:1], H, W))     # a union, not an XOR
    got = polygon_bits(objs, (H, W), device=DEV)
    assert "seg_toggles_fill_kernel" in _lib.last_kernel()
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape and got.device == DEV
    got = _words(got)
    for n, name in enumerate(names):
        assert got[n].tolist() == want[n].tolist(), f"{H}x{W} {name}"
    # one object alone, the rings of all objects as ONE object (their union), and a second run (the toggles are atomics)
    k = i("bow-tie")
    np.testing.assert_array_equal(_words(polygon_bits(objs[k:k + 1], (H, W), device=DEV)), want[k:k + 1])
    n_some = min(40, N_RANDOM[(H, W)])                      # (the random rings come first)
    some = [o[0] for o in objs[:n_some]]
    np.testing.assert_array_equal(_words(polygon_bits([some, some[::-1]], (H, W), device=DEV)),
                                  R.pack_columns(np.stack([dense[:n_some].any(0)] * 2)))
    np.testing.assert_array_equal(_words(polygon_bits(objs, (H, W), device=DEV)), want)
    # dense targets: the device form of convert_coco_poly_to_mask
    pick = [0, 1, k, i("two overlapping rings"), i("no ring")]
    masks = polygon_masks([objs[j] for j in pick], (H, W), device=DEV)
    assert masks.dtype == torch.bool and tuple(masks.shape) == (len(pick), H, W)
    np.testing.assert_array_equal(_np(masks), dense[pick])
    f32 = unpack_masks(torch.from_numpy(want[pick].view(np.int64)).to(DEV), (H, W), dtype=torch.float32)
    assert f32.dtype == torch.float32
    np.testing.assert_array_equal(_np(f32), dense[pick].astype(np.float32))


def test_a_ring_longer_than_the_stage_and_no_object():
    from mp_former_amd import _lib
    from mp_former_amd.inference import polygon_bits
    H, W = 257, 1030
    stage = _lib.lib().mpf_seg_poly_stage_edges()
    g = np.random.default_rng(5)
    rings = []
    for k in (stage + 1, 2 * stage + 477, stage, stage - 1):          # past one stage, past two, exactly one, just under
        t = np.sort(g.uniform(0, 2 * np.pi, k))
        r = g.uniform(60, 125, k)
        rings.append(np.stack([500.25 + 3.5 * r * np.cos(t), 128.5 + r * np.sin(t)], axis=1).reshape(-1).tolist())
    rings.append([v for j in range(stage + 40) for v in ((j * 7) % (W + 4) - 2, (j * 13) % (H + 4) - 2)])     # long edges, self-intersecting
    objs = [[r] for r in rings] + [rings[:2]]
    want = R.pack_columns(np.stack([C.poly_mask(o, H, W) for o in objs]))
    assert all(w.any() for w in want)
    np.testing.assert_array_equal(_words(polygon_bits(objs, (H, W), device=DEV)), want)
    # no object at all; objects without a ring only
    empty = polygon_bits([], (H, W), device=DEV)
    assert tuple(empty.shape) == (0, (H * W + 63) // 64) and empty.dtype == torch.int64 and empty.device == DEV
    none = polygon_bits([[], []], (37, 50), device=DEV)
    assert tuple(none.shape) == (2, 29) and not _np(none).any()


@functools.lru_cache(maxsize=None)
def _rle_scene(H, W):
    """-> (names, run lengths, dense bool [M, H, W])"""
    HW = H * W
    g = np.random.default_rng(H * 77 + W)
    names, runs = ["empty", "full", "zero-length runs in the middle", "zero-length runs at both ends"], [[HW], [0, HW]]
    runs.append([2, 0, 1, 3, 0, 0, 0, 4, HW - 10, 0])
    runs.append([0, 0, 0, 5, 0, 0, HW - 5, 0, 0])
    if (H, W) in SMALL:
        names += ["every pixel alternating", "every pixel alternating, from 1"]
        runs += [[1] * HW, [0] + [1] * HW]
    n = 3 if HW < 10000 else 1
    for p in (0.5, 0.01):
        for i in range(n):
            names.append(f"random {p} #{i}")
            runs.append(C.encode(g.random((H, W)) < p))
    dense = np.stack([C.decode(c, H, W) for c in runs])
    return tuple(names), runs, dense


@pytest.mark.parametrize("hw", SHAPES, ids=lambda o: f"{o[0]}x{o[1]}")
def test_rle_bits_equal_the_restatement_and_close_the_loop(hw):
    from mp_former_amd import _lib
    from mp_former_amd.inference import bits_rle, pack_masks, rle_bits, rle_compress, unpack_masks
    H, W = hw
    names, runs, dense = _rle_scene(H, W)
    want = R.pack_columns(dense)
    assert not dense[0].any() and dense[1].all() and dense[2].sum() == 3 + 4 and dense[3].sum() == 5
    rles = [{"size": [H, W], "counts": c} for c in runs]
    got = rle_bits(rles, device=DEV)
    assert "seg_toggles_fill_kernel" in _lib.last_kernel()
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape and got.device == DEV
    for n, name in enumerate(names):
        assert _words(got)[n].tolist() == want[n].tolist(), f"{H}x{W} {name}"
    # the same as strings and bytes, with the size given
    texts = [C.to_string(c) for c in runs]
    as_str = [{"size": [H, W], "counts": t if n % 2 else t.encode()} for n, t in enumerate(texts)]
    np.testing.assert_array_equal(_words(rle_bits(as_str, size=(H, W), device=DEV)), want)
    assert [rle_compress(r)["counts"] for r in rles] == texts
    # against the kernels that exist: pack_masks of the dense masks, bits_rle back to the canonical counts, unpack_masks
    dev_dense = torch.from_numpy(dense).to(DEV)
    packed = pack_masks(dev_dense)
    canonical = [{"size": [H, W], "counts": C.encode(d)} for d in dense]
    assert torch.equal(rle_bits(canonical, device=DEV), packed)
    assert torch.equal(got, packed)
    assert bits_rle(got, (H, W)) == canonical
    assert torch.equal(unpack_masks(packed, (H, W)), dev_dense)
    u8 = unpack_masks(packed[2:], (H, W), dtype=torch.uint8)
    assert u8.dtype == torch.uint8 and torch.equal(u8, dev_dense[2:].to(torch.uint8))
    assert tuple(rle_bits([], size=(H, W), device=DEV).shape) == (0, want.shape[1])
    assert tuple(unpack_masks(packed[:0], (H, W)).shape) == (0, H, W)


@pytest.mark.parametrize("hw", [(37, 50), (130, 520)], ids=lambda o: f"{o[0]}x{o[1]}")
def test_segmentation_bits_takes_the_mixed_forms_in_input_order(hw):
    from mp_former_amd.inference import segmentation_bits
    H, W = hw
    _, objs, _, _ = _polygon_scene(H, W)
    _, runs, _ = _rle_scene(H, W)
    rle = lambda c: {"size": [H, W], "counts": c}            # noqa: E731
    segms = [None, objs[0], rle(runs[4]), rle(C.to_string(runs[5])), None, objs[-6] + objs[3], rle(runs[2]), [], objs[7],
             rle(C.to_string(runs[1]).encode())]
    want = R.pack_columns(np.stack([C.segm_mask(s, H, W) for s in segms]))
    assert want[1].any() and want[2].any() and not want[0].any() and not want[7].any()
    np.testing.assert_array_equal(_words(segmentation_bits(segms, (H, W), device=DEV)), want)
    # one kind with gaps, the other kind with gaps, nothing but gaps, nothing
    for pick in ([0, 1, 4, 5, 7, 8], [4, 2, 0, 3, 9], [0, 4], []):
        got = segmentation_bits([segms[j] for j in pick], (H, W), device=DEV)
        assert tuple(got.shape) == (len(pick), want.shape[1])
        np.testing.assert_array_equal(_words(got), want[pick])


# ---- the evaluators -------------------------------------------------------------------------------------------------------------------
def _same_results(a, b):
    assert a.keys() == b.keys()
    for t in a:
        assert a[t].keys() == b[t].keys()
        for k, v in a[t].items():
            assert v == b[t][k] or (np.isnan(v) and np.isnan(b[t][k])), (t, k, v, b[t][k])


def test_instance_evaluator_takes_coco_annotations():
    from mp_former_amd.d2_plugin import InstanceAPEvaluator
    from mp_former_amd.inference import pack_masks
    H, W, K = 40, 56, 3
    ids = {1: 0, 18: 1, 44: 2}
    sq = lambda x0, y0, x1, y1: [x0, y0, x1, y0, x1, y1, x0, y1]      # noqa: E731
    crowd = np.zeros((H, W), dtype=bool)
    crowd[5:30, 30:50] = True
    small = np.zeros((H, W), dtype=bool)
    small[0:10, 0:4] = True
    images = [
        # every annotation with "area" and "bbox": both are used (areas that differ from the pixel counts, so that it shows)
        [{"segmentation": [sq(2, 3, 20, 22)], "category_id": 1, "iscrowd": 0, "area": 900.0, "bbox": [2.0, 3.0, 18.0, 19.0]},
         {"segmentation": [sq(25, 4, 50, 16), sq(25, 20, 50, 36)], "category_id": 18, "area": 1200.5, "bbox": [25.0, 4.0, 25.0, 32.0]},
         {"segmentation": {"size": [H, W], "counts": C.encode(crowd)}, "category_id": 44, "iscrowd": 1, "area": 500.0,
          "bbox": [30.0, 5.0, 20.0, 25.0]},
         {"segmentation": {"size": [H, W], "counts": C.to_string(C.encode(small))}, "category_id": 1,
          "area": 40.0, "bbox": [0.0, 0.0, 10.0, 10.0]}],
        # one annotation without "area" and one without "bbox": the pixel counts and the masks' boxes
        [{"segmentation": [[4.5, 4.5, 30.5, 6.0, 18.0, 33.5]], "category_id": 44, "bbox": [4.5, 4.5, 26.0, 29.0]},
         {"segmentation": [sq(30, 10, 54, 38)], "category_id": 18, "area": 672.0}],
        [],                                                  # an image without annotations
    ]
    g = np.random.default_rng(3)
    inputs_a, inputs_d, outputs = [], [], []
    for anns in images:
        dense = np.stack([C.segm_mask(a["segmentation"], H, W) for a in anns]) if anns else np.zeros((0, H, W), dtype=bool)
        # predictions: every ground truth shifted a little, and two loose boxes
        pm = [np.roll(m, (1, 2), (0, 1)) for m in dense] + [np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)]
        pm[-2][1:9, 1:9] = True
        pm[-1][20:39, 2:30] = True
        pred = {"bits": pack_masks(torch.from_numpy(np.stack(pm)).to(DEV)), "size": (H, W),
                "scores": torch.from_numpy(g.random(len(pm)).astype(np.float32)).to(DEV),
                "pred_classes": torch.tensor([ids[a["category_id"]] for a in anns] + [0, 1], device=DEV)}
        outputs.append({"instances": pred})
        inputs_a.append({"annotations": anns})
        gt = {"gt_masks": torch.from_numpy(dense), "gt_classes": torch.tensor([ids[a["category_id"]] for a in anns], dtype=torch.int64),
              "gt_iscrowd": [a.get("iscrowd", 0) for a in anns]}
        if anns and all("area" in a for a in anns):
            gt["gt_areas"] = [a["area"] for a in anns]
        if anns and all("bbox" in a for a in anns):
            gt["gt_boxes"] = torch.tensor([[a["bbox"][0], a["bbox"][1], a["bbox"][0] + a["bbox"][2], a["bbox"][1] + a["bbox"][3]]
                                           for a in anns], dtype=torch.float64)
        inputs_d.append({"instances": gt})
    ev_a = InstanceAPEvaluator(K, device=DEV, iou_types=("segm", "bbox"), dataset_id_to_contiguous=ids)
    ev_d = InstanceAPEvaluator(K, device=DEV, iou_types=("segm", "bbox"))
    ev_a.process(inputs_a, outputs)
    ev_d.process(inputs_d, outputs)
    res_a, res_d = ev_a.evaluate(), ev_d.evaluate()
    _same_results(res_a, res_d)
    assert res_a["segm"]["AP"] > 0 and res_a["bbox"]["AP"] > 0
    # the areas of the annotations were used: without them the numbers of the size ranges change
    for inp in inputs_d:
        inp["instances"].pop("gt_areas", None)
    ev_n = InstanceAPEvaluator(K, device=DEV, iou_types=("segm",))
    ev_n.process(inputs_d, outputs)
    assert ev_n.evaluate()["segm"] != res_a["segm"]
    # identity mapping: the category ids are the classes
    ev_i = InstanceAPEvaluator(50, device=DEV)
    ev_i.process(inputs_a, [{"instances": dict(o["instances"], pred_classes=torch.tensor(
        [a["category_id"] for a in anns] + [1, 18], device=DEV))} for o, anns in zip(outputs, images)])
    assert ev_i.evaluate()["segm"]["AP"] == res_a["segm"]["AP"]
    with pytest.raises(ValueError, match="dataset_id_to_contiguous"):
        InstanceAPEvaluator(K, device=DEV, dataset_id_to_contiguous={1: 0}).process(inputs_a[:1], outputs[:1])


def test_video_evaluator_takes_segmentations():
    from mp_former_amd.d2_plugin import YTVISEvaluatorHIP
    from mp_former_amd.inference import pack_masks
    H, W, F, K = 36, 44, 3, 4
    sq = lambda x0, y0, x1, y1: [x0, y0, x1, y0, x1, y1, x0, y1]      # noqa: E731
    blob = np.zeros((H, W), dtype=bool)
    blob[10:30, 5:25] = True
    rle = lambda m: {"size": [H, W], "counts": C.encode(m)}  # noqa: E731
    segs = [[[sq(3, 3, 20, 20)], None, [sq(5, 5, 22, 22), sq(30, 2, 40, 12)]],
            [rle(blob), dict(rle(np.roll(blob, 3, 1)), counts=C.to_string(C.encode(np.roll(blob, 3, 1)))), None],
            [None, None, [[24.5, 20.0, 43.0, 21.5, 30.0, 35.5]]]]
    classes, crowd = [2, 0, 3], [0, 0, 0]
    dense = np.stack([np.stack([C.segm_mask(s, H, W) for s in tube]) for tube in segs])
    assert dense[0, 0].any() and not dense[0, 1].any() and dense[2, 2].any()
    pm = np.concatenate([np.roll(dense, 1, 3), np.roll(dense[:1], 6, 2)])
    T = pm.shape[0]
    out = {"bits": pack_masks(torch.from_numpy(pm.reshape(T * F, H, W)).to(DEV)).view(T, F, -1), "size": (H, W),
           "pred_scores": torch.tensor([0.9, 0.8, 0.7, 0.6], device=DEV), "pred_labels": torch.tensor([2, 0, 3, 2], device=DEV),
           "frame_area": torch.from_numpy(pm.reshape(T, F, -1).sum(-1).astype(np.int32)).to(DEV)}
    ev_s, ev_d = YTVISEvaluatorHIP(K, device=DEV), YTVISEvaluatorHIP(K, device=DEV)
    ev_s.process([{"instances": {"segmentations": segs, "gt_classes": classes, "gt_iscrowd": crowd}}], out)
    ev_d.process([{"instances": {"gt_masks": torch.from_numpy(dense), "gt_classes": classes, "gt_iscrowd": crowd}}], out)
    res = ev_s.evaluate()
    _same_results(res, ev_d.evaluate())
    assert res["segm"]["AP"] > 0
    with pytest.raises(ValueError, match=r"\[G\]\[3\]"):
        ev_s.process([{"instances": {"segmentations": [segs[0][:2]], "gt_classes": [2]}}], out)
