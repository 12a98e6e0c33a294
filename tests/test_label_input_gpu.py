"""GPU: the label-map input path (mp_former_amd.label_input, csrc/label_input.hip, the output-side flip of csrc/img_resample.hip and
the d2_plugin mappers) against the numpy restatement of the reference's mappers (tests/_label_restate.py).  Every comparison is
integer equality."""
import numpy as np
import pytest
import torch

import _label_restate as L
import _resample_restate as R

pytestmark = pytest.mark.gpu

PAD = 0xFFFFFF
TARGETS = ((64, 19), (11, 200))


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _sources():
    g = np.random.default_rng(42)
    u8 = g.integers(0, 7, size=(37, 53)).astype(np.uint8)
    u8[g.random((37, 53)) < 0.1] = 255
    i32 = g.integers(0, 70001, size=(130, 70)).astype(np.int32)
    i32[40:90, 10:50] = 70000
    rgb = g.integers(0, 256, size=(41, 29, 3)).astype(np.uint8)
    rgb[5:20, 3:17] = (7, 1, 2)
    return {"u8": u8, "i32": i32, "rgb": rgb}


SOURCES = _sources()


def _ids(a, kind):
    return L.rgb2id(a) if kind == "rgb" else a.astype(np.int64)


# ---- resample_labels ------------------------------------------------------------------------------------------------------------------
def _want_resampled(src, kind, p, rule, pad_id, canvas, semseg):
    out = np.full(canvas, pad_id, dtype=np.int64)
    ids = _ids(src, kind)
    if semseg:                                               # resize, crop, flip the crop, pad
        full = L.resize_nearest(ids, p.resized[0], p.resized[1], rule)
        win = full[p.offset[0]:p.offset[0] + p.crop[0], p.offset[1]:p.offset[1] + p.crop[1]]
        out[:win.shape[0], :win.shape[1]] = win[:, ::-1] if p.flip else win
    else:                                                    # flip, resize, crop, pad
        win = L.label_lsj(ids, p.flip, p.resized, p.offset, p.crop, pad_id, rule)
        out[:p.crop[0], :p.crop[1]] = win
    return out


@pytest.mark.parametrize("rule", ["pil", "torch"])
@pytest.mark.parametrize("target", TARGETS, ids=lambda t: "to%dx%d" % t)
@pytest.mark.parametrize("kind", ["u8", "i32", "rgb"])
def test_resample_labels_equals_the_restated_mappers(dev, kind, target, rule):
    from mp_former_amd import augment as A
    from mp_former_amd import label_input as LI
    src = SOURCES[kind]
    H, W = src.shape[:2]
    rh, rw = target
    off = (min(5, rh - 1), min(3, rw - 1))
    crop = (rh - off[0] + 6, max(1, (rw - off[1]) // 2))     # valid < crop on the y axis, the crop cuts the x axis
    valid = (rh - off[0], crop[1])
    canvas = (crop[0] + 2, crop[1] + 5)
    params = [A.LSJParams(False, (H, W), (rh, rw), (0, 0), (rh, rw), (rh, rw)),
              A.LSJParams(True, (H, W), (rh, rw), off, crop, valid),
              A.SemSegParams((H, W), (rh, rw), off, valid, valid, True, canvas),
              A.SemSegParams((H, W), (rh, rw), (0, 0), (rh, rw), (rh, rw), False, (rh, rw))]
    full_canvas = (max(canvas[0], rh), max(canvas[1], rw))
    t = torch.from_numpy(src)
    wide = torch.zeros((H, W + 9) + src.shape[2:], dtype=t.dtype)
    wide[:, :W] = t                                          # a device source with a row stride larger than W
    srcs = [t, wide.to(dev)[:, :W], t.to(dev), t]
    pad_id = PAD if kind == "rgb" else 255
    got = LI.resample_labels(srcs, params, kind, pad_id, canvas=full_canvas, device=dev, rule=rule)
    assert got.dtype == torch.int32 and tuple(got.shape) == (4,) + full_canvas and got.device == dev
    for b, p in enumerate(params):
        want = _want_resampled(src, kind, p, rule, pad_id, full_canvas, isinstance(p, A.SemSegParams))
        np.testing.assert_array_equal(got[b].cpu().numpy(), want, err_msg=f"image {b}")
    again = LI.resample_labels(srcs, params, kind, pad_id, canvas=full_canvas, device=dev, rule=rule)
    assert torch.equal(got, again)


def test_resample_labels_rule_defaults_and_argument_errors(dev):
    from mp_former_amd import augment as A
    from mp_former_amd import label_input as LI
    src = SOURCES["u8"]
    t = torch.from_numpy(src)
    sem = A.SemSegParams((37, 53), (50, 70), (0, 0), (50, 70), (50, 70), False, (50, 70))
    lsj = A.resize_params(37, 53, (50, 70))
    np.testing.assert_array_equal(LI.resample_labels([t], [sem], "u8", 255, device=dev)[0].cpu().numpy(), L.resize_nearest(src, 50, 70, "torch"))
    np.testing.assert_array_equal(LI.resample_labels([t], [lsj], "u8", 255, device=dev)[0].cpu().numpy(), L.resize_nearest(src, 50, 70, "pil"))
    assert LI.resample_labels([], [], "u8", 255, canvas=(4, 5), device=dev).shape == (0, 4, 5)
    with pytest.raises(ValueError, match="one kind per batch"):
        LI.resample_labels([t, torch.from_numpy(SOURCES["i32"])], [lsj, A.resize_params(130, 70, (5, 5))], "u8", 255, device=dev)
    with pytest.raises(ValueError, match="one kind per batch"):
        LI.resample_labels([torch.from_numpy(SOURCES["rgb"])], [A.resize_params(41, 29, (5, 5))], "u8", 255, device=dev)
    with pytest.raises(ValueError, match="smaller than the crop"):
        LI.resample_labels([t], [lsj], "u8", 255, canvas=(49, 70), device=dev)
    with pytest.raises(ValueError, match="kind must be"):
        LI.resample_labels([t], [lsj], "u16", 255, device=dev)


# ---- window_counts --------------------------------------------------------------------------------------------------------------------
def _count_source(K, ignore, shape, dtype):
    g = np.random.default_rng(K)
    a = g.integers(0, K, size=shape).astype(dtype)
    a[g.random(shape) < 0.15] = ignore
    a[: shape[0] // 3, : shape[1] // 2] = K - 1             # a large uniform region: the area rule has something to reject
    return a


@pytest.mark.parametrize("rule", ["torch", "pil"])
@pytest.mark.parametrize("K", [2, 151, 1024])
def test_window_counts_equal_np_unique_on_the_restated_resize(dev, K, rule):
    from mp_former_amd import augment as A
    from mp_former_amd import label_input as LI
    assert LI.MAX_CLASSES == 1024
    ignore = 255 if K <= 255 else 65535
    dtype = np.uint8 if K <= 255 else np.int32
    shapes = ((37, 53), (130, 70))
    resized = ((64, 19), (70, 200))
    srcs = [_count_source(K, ignore, s, dtype) for s in shapes]
    params = [A.SemSegDraw(s, r, (1, 1), ((0, 0),), True, (1, 1)) for s, r in zip(shapes, resized)]
    # 1 x 1, the whole map, one that straddles the boundary between two row bands (32 window rows each), one inside a band
    windows = [[(r[0] - 1, r[1] - 1, 1, 1), (0, 0, r[0], r[1]), (3, 2, 40, r[1] - 5), (30, 1, 5, 7)] for r in resized]
    got = LI.window_counts([torch.from_numpy(s) for s in srcs], params, windows, K, ignore, device=dev, rule=rule)
    assert got.dtype == torch.int32 and tuple(got.shape) == (2, 4, K) and not got.is_cuda
    for b, (s, r) in enumerate(zip(srcs, resized)):
        full = L.resize_nearest(s.astype(np.int64), r[0], r[1], rule)
        for t, (y0, x0, h, w) in enumerate(windows[b]):
            labels, cnt = np.unique(full[y0:y0 + h, x0:x0 + w], return_counts=True)
            want = np.zeros(K, dtype=np.int64)
            want[labels[labels != ignore]] = cnt[labels != ignore]
            np.testing.assert_array_equal(got[b, t].numpy(), want, err_msg=f"image {b} window {t}")
    # the rule applied to the counts is the rule applied to the map
    for b, r in enumerate(resized):
        full = L.resize_nearest(srcs[b].astype(np.int64), r[0], r[1], rule)
        for area in (0.5, 0.75, 1.0):
            i = A.choose_category_crop(got[b, 1:3].numpy(), 2, area)
            boxes = windows[b][1:3]
            want = L.choose_from_counts(np.stack([np.bincount(full[y:y + h, x:x + w].ravel()[full[y:y + h, x:x + w].ravel() != ignore],
                                                              minlength=K)[:K] for (y, x, h, w) in boxes]), area)
            assert i == want


def test_window_counts_raise_on_a_label_outside_the_classes(dev):
    from mp_former_amd import augment as A
    from mp_former_amd import label_input as LI
    src = _count_source(5, 255, (37, 53), np.uint8)
    src[20, 30] = 9
    p = A.SemSegDraw((37, 53), (37, 53), (1, 1), ((0, 0),), False, (1, 1))
    t = torch.from_numpy(src)
    with pytest.raises(ValueError, match="neither in 0 .. 4 nor the ignore label 255"):
        LI.window_counts([t], [p], [[(0, 0, 37, 53)]], 5, 255, device=dev)
    got = LI.window_counts([t], [p], [[(0, 0, 20, 53)]], 5, 255, device=dev)     # a window that misses it
    assert int(got.sum()) == int((src[:20] != 255).sum())
    neg = torch.from_numpy(src.astype(np.int32))
    neg[2, 2] = -3
    with pytest.raises(ValueError, match="neither in"):
        LI.window_counts([neg], [p], [[(0, 0, 37, 53)]], 5, 255, device=dev)


# ---- label_bits -----------------------------------------------------------------------------------------------------------------------
BIG = (1 << 24) + 12345


def _id_map(H, W, nid=300):
    """ids 0 .. nid-1 in blobs, one id above 2^24, the pad id on the right edge; id 3 and id 100003 never occur"""
    g = np.random.default_rng(H * 1000 + W)
    m = g.integers(0, nid, size=(H, W)).astype(np.int64)
    yy, xx = np.mgrid[:H, :W]
    m[(yy // 5 + xx // 3) % 3 == 0] = 7                      # runs along both axes
    m[(yy + xx) % 11 == 0] = BIG
    m[m == 3] = 4
    m[:, W - 1] = PAD
    return m.astype(np.int32)


@pytest.mark.parametrize("W", [1, 7, 64, 200])
@pytest.mark.parametrize("H", [1, 63, 64, 65, 130])
def test_label_bits_equal_the_restatement_and_pack_masks(dev, H, W):
    from mp_former_amd import label_input as LI
    from mp_former_amd.inference import pack_masks, unpack_masks
    m = _id_map(H, W)
    canvas = torch.full((H + 3, W + 5), -1, dtype=torch.int32)
    canvas[:H, :W] = torch.from_numpy(m)
    canvas = canvas.to(dev)
    ids = [7, 3, BIG, 7, PAD, 0, 100003, 299]               # present, absent, above 2^24, a duplicate, the pad id
    want_bits, want_areas = L.id_bits(m, ids)
    for id_map, size in ((canvas, (H, W)), (canvas[:H, :W], None)):          # a region of a canvas; a view with a row stride > W
        bits, areas = LI.label_bits(id_map, ids, size)
        assert bits.dtype == torch.int64 and tuple(bits.shape) == (len(ids), (H * W + 63) // 64) and areas.dtype == torch.int32
        np.testing.assert_array_equal(bits.cpu().numpy(), want_bits)
        np.testing.assert_array_equal(areas.cpu().numpy(), want_areas)
    dense = torch.stack([canvas[:H, :W] == k for k in ids])
    assert torch.equal(bits, pack_masks(dense))
    assert torch.equal(unpack_masks(bits, (H, W)), dense)
    pop = np.array([sum(bin(int(w) & 0xFFFFFFFFFFFFFFFF).count("1") for w in row) for row in bits.cpu().numpy()])
    np.testing.assert_array_equal(areas.cpu().numpy(), pop)
    assert int(areas[1]) == 0 and int(areas[6]) == 0 and torch.equal(bits[0], bits[3]) and int(areas[4]) == H
    again, areas2 = LI.label_bits(canvas, ids, (H, W))
    assert torch.equal(bits, again) and torch.equal(areas, areas2)


@pytest.mark.parametrize("T", [0, 1, 3, 256, 300])
def test_label_bits_list_lengths_up_to_more_than_one_launch(dev, T):
    from mp_former_amd import label_input as LI
    assert LI.MAX_IDS == 255
    H, W = 130, 200
    m = _id_map(H, W)
    ids = list(range(T - 1, -1, -1))                         # descending: the rows come back in the caller's order
    bits, areas = LI.label_bits(torch.from_numpy(m).to(dev), ids)
    want_bits, want_areas = L.id_bits(m, ids)
    assert tuple(bits.shape) == (T, (H * W + 63) // 64) and tuple(areas.shape) == (T,)
    np.testing.assert_array_equal(bits.cpu().numpy(), want_bits)
    np.testing.assert_array_equal(areas.cpu().numpy(), want_areas)


def test_label_bits_argument_errors(dev):
    from mp_former_amd import label_input as LI
    m = torch.zeros((8, 10), dtype=torch.int32, device=dev)
    with pytest.raises(ValueError, match="int32"):
        LI.label_bits(m.long(), [1])
    with pytest.raises(ValueError, match="inside the map"):
        LI.label_bits(m, [1], (9, 10))
    with pytest.raises(ValueError, match="fit int32"):
        LI.label_bits(m, [1 << 31])


def test_targets_from_an_id_map(dev):
    from mp_former_amd import label_input as LI
    m = _id_map(40, 50)
    segs = [{"id": 7, "category_id": 17, "iscrowd": 0}, {"id": 299, "category_id": 2, "iscrowd": 1},
            {"id": 3, "category_id": 5, "iscrowd": 0}, {"id": BIG, "category_id": 1, "iscrowd": 0}]
    t = LI.panoptic_targets(torch.from_numpy(m).to(dev), segs)
    masks = np.stack([m == 7, m == 3, m == BIG])
    assert t["labels"].tolist() == [17, 5, 1] and t["labels"].dtype == torch.int64
    np.testing.assert_array_equal(t["masks"].cpu().numpy(), masks)
    assert t["boxes"].dtype == torch.float32
    np.testing.assert_array_equal(t["boxes"].cpu().numpy(), L.boxes(masks))
    np.testing.assert_array_equal(t["bits"].cpu().numpy(), L.pack(masks))
    empty = LI.panoptic_targets(torch.from_numpy(m).to(dev), [])
    assert tuple(empty["masks"].shape) == (0, 40, 50) and tuple(empty["boxes"].shape) == (0, 4) and tuple(empty["labels"].shape) == (0,)
    s = LI.semantic_targets(torch.from_numpy(m).to(dev), [0, 4, 7], (33, 41))
    masks = np.stack([m[:33, :41] == k for k in (0, 4, 7)])
    np.testing.assert_array_equal(s["masks"].cpu().numpy(), masks)
    np.testing.assert_array_equal(s["boxes"].cpu().numpy(), L.boxes(masks))
    assert s["labels"].tolist() == [0, 4, 7] and s["areas"].tolist() == masks.reshape(3, -1).sum(axis=1).tolist()


# ---- the image: a flip applied to the output --------------------------------------------------------------------------------------------
def _image(h, w, seed):
    g = np.random.default_rng(seed)
    img = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img[::3] = 255 - img[::3] // 4                           # hard edges: rounding differences show
    return img


def test_image_flip_out_is_the_mirrored_resize_and_not_flip_in(dev):
    from mp_former_amd import augment as A
    img = _image(37, 53, 1)
    resized, off, crop, canvas = (64, 19), (5, 3), (40, 12), (48, 16)
    full = R.resize(img, *resized)
    win = full[off[0]:off[0] + crop[0], off[1]:off[1] + crop[1]]
    want = np.full((3,) + canvas, 128, dtype=np.uint8)      # the mapper pads the flipped crop to its canvas with 128
    want[:, :crop[0], :crop[1]] = win[:, ::-1].transpose(2, 0, 1)
    sem = A.SemSegParams((37, 53), resized, off, crop, crop, True, canvas)
    got = A.resample_images([torch.from_numpy(img)], [sem], device=dev)
    assert tuple(got.shape) == (1, 3) + canvas
    np.testing.assert_array_equal(got[0].cpu().numpy(), want)
    # valid < crop: the mirror is of the valid columns, the pad stays at the bottom right
    small = A.SemSegParams((37, 53), (20, 9), (0, 2), (32, 16), (20, 7), True, (32, 16))
    want = np.zeros((3, 32, 16), dtype=np.uint8)
    want[:, :32, :16] = 128
    want[:, :20, :7] = R.resize(img, 20, 9)[:, 2:9][:, ::-1].transpose(2, 0, 1)
    np.testing.assert_array_equal(A.resample_images([torch.from_numpy(img)], [small], device=dev)[0].cpu().numpy(), want)
    # flip(resize(x)) cropped is not the crop of resize(flip(x)): the same record with the flip on the other side reads another
    # window.  (For the WHOLE width the two orders gave equal bytes in every size pair searched on the CPU, about ten thousand: PIL's
    # tables came out mirror-symmetric in all of them, so only a case with an off-centre crop tells the two flags apart.)
    out_side = np.full((3,) + canvas, 128, dtype=np.uint8)
    out_side[:, :crop[0], :crop[1]] = win[:, ::-1].transpose(2, 0, 1)
    in_side = R.lsj_image(img, True, resized, off, crop)
    assert (out_side[:, :crop[0], :crop[1]] != in_side).any(), "the case no longer tells the two flips apart"
    got_in = A.resample_images([torch.from_numpy(img)], [A.LSJParams(True, (37, 53), resized, off, crop, crop)], device=dev)[0]
    np.testing.assert_array_equal(got_in.cpu().numpy(), in_side)
    np.testing.assert_array_equal(got[0].cpu().numpy(), out_side)
    # and without a flip the record's last word changes nothing
    whole = ((37, 20), (0, 0), (37, 20), (37, 20))
    plain = A.resample_images([torch.from_numpy(img)], [A.SemSegParams((37, 53), *whole, False, (37, 20))], device=dev)[0]
    assert torch.equal(plain, A.resample_images([torch.from_numpy(img)], [A.LSJParams(False, (37, 53), *whole)], device=dev)[0])
    np.testing.assert_array_equal(plain.cpu().numpy(), R.resize(img, 37, 20).transpose(2, 0, 1))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
SIZES = ((60, 80), (57, 83), (80, 61))


def _dataset(tmp_path):
    """three images with a panoptic PNG (ids as RGB) and a semantic PNG (class ids, 255 = ignore), and their dataset dicts"""
    Image = pytest.importorskip("PIL.Image")
    dicts = []
    for n, (h, w) in enumerate(SIZES):
        g = np.random.default_rng(100 + n)
        img = _image(h, w, 10 + n)
        yy, xx = np.mgrid[:h, :w]
        seg = ((yy // 17) * 5 + xx // 23).astype(np.int64)                      # blocks of 17 x 23
        ids = 1000 * (seg + 1) + 70000 * (seg % 3)                              # ids that need all three channels
        pan = np.stack([ids % 256, (ids // 256) % 256, ids // 65536], axis=2).astype(np.uint8)
        sem = (seg % 4).astype(np.uint8)
        sem[:, :int(w * 0.55)] = 0                                             # one class dominates the left: windows there are rejected
        sem[g.random((h, w)) < 0.05] = 255
        sem[:12, :] = 255
        segments = [{"id": int(i), "category_id": int(i // 1000 % 7), "iscrowd": int(k == 2)} for k, i in enumerate(np.unique(ids))]
        segments.append({"id": 999999, "category_id": 3, "iscrowd": 0})        # in the json, nowhere in the PNG
        files = {}
        for name, a in (("img", img), ("pan", pan), ("sem", sem)):
            files[name] = str(tmp_path / f"{name}{n}.png")
            Image.fromarray(a).save(files[name])
        dicts.append({"file_name": files["img"], "pan_seg_file_name": files["pan"], "sem_seg_file_name": files["sem"], "height": h,
                      "width": w, "image_id": n, "segments_info": segments, "_arrays": (img, pan, sem)})
    return dicts


class _Stub:
    """a model that records what its forward is given"""

    def __init__(self, device):
        self.training, self.device, self.seen = True, device, []

    def forward(self, batched_inputs):
        self.seen.append(batched_inputs)
        return len(batched_inputs)


def test_panoptic_mapper_end_to_end(dev, tmp_path):
    from mp_former_amd import d2_plugin as P
    dicts = _dataset(tmp_path)
    mapper = P.COCOPanopticLSJDeviceMapper(True, image_size=32, min_scale=0.1, max_scale=2.0, random_flip="horizontal", image_format="RGB")
    np.random.seed(3)
    batch = [mapper({k: v for k, v in d.items() if k not in ("_arrays", "sem_seg_file_name")}) for d in dicts]
    for x, d in zip(batch, dicts):
        np.testing.assert_array_equal(x["image_raw"].numpy(), d["_arrays"][0])
        np.testing.assert_array_equal(x["pan_raw"].numpy(), d["_arrays"][1])
        assert "pan_seg_file_name" not in x and x["image_id"] == d["image_id"]
    out = P.native_panoptic_inputs(batch, dev)
    padded = cropped = empty = flipped = 0
    for x, o, d in zip(batch, out, dicts):
        p = x["lsj"]
        img, classes, masks, boxes = L.panoptic_mapper(d["_arrays"][0], d["_arrays"][1], d["segments_info"], p.flip, p.resized, p.offset, p.crop)
        np.testing.assert_array_equal(o["image"].cpu().numpy(), img)
        inst = o["instances"]
        assert inst.gt_classes.dtype == torch.int64 and inst.gt_masks.dtype == torch.bool
        np.testing.assert_array_equal(inst.gt_classes.cpu().numpy(), classes)
        np.testing.assert_array_equal(inst.gt_masks.cpu().numpy(), masks)
        np.testing.assert_array_equal(inst.gt_boxes.tensor.cpu().numpy(), boxes)
        assert tuple(inst.image_size) == (32, 32) and "image_raw" not in o and "pan_raw" not in o
        padded += p.valid != p.crop
        cropped += p.resized[0] > 32 or p.resized[1] > 32
        empty += int((masks.reshape(len(masks), -1).sum(axis=1) == 0).sum())
        flipped += p.flip
    assert padded and cropped and empty and flipped, "the draws of this seed must cover pad, crop, empty segments and a flip"
    # the model hook: training gets the formed dicts, eval is passed through
    model = _Stub(dev)
    P.install_native_panoptic_lsj(model)
    assert model.forward(batch) == 3
    seen = model.seen[-1]
    assert all("instances" in s and s["image"].is_cuda for s in seen)
    assert torch.equal(seen[1]["instances"].gt_masks, out[1]["instances"].gt_masks)
    model.training = False
    model.forward(batch)
    assert model.seen[-1] is batch


@pytest.mark.parametrize("max_area", [0.75, 1.0])
def test_semantic_mapper_end_to_end(dev, tmp_path, max_area):
    from mp_former_amd import augment as A
    from mp_former_amd import d2_plugin as P
    dicts = _dataset(tmp_path)
    mapper = P.SemanticDeviceMapper(True, min_size=(24, 40, 64), max_size=100, sampling="choice", crop_enabled=True, crop_type="absolute",
                                    crop_size=(32, 32), single_category_max_area=max_area, color_aug_ssd=False, image_format="RGB",
                                    ignore_label=255, size_divisibility=32, num_classes=4)
    np.random.seed(1)
    batch = [mapper({k: v for k, v in d.items() if k not in ("_arrays", "pan_seg_file_name", "segments_info")}) for d in dicts]
    for x, d in zip(batch, dicts):
        np.testing.assert_array_equal(x["sem_seg_raw"].numpy(), d["_arrays"][2])
        assert len(x["semseg"].origins) == (10 if max_area < 1.0 else 1) and "sem_seg_file_name" not in x
    out = P.native_semantic_inputs(batch, dev, 4, 255, max_area)
    padded = flipped = later = 0
    for x, o, d in zip(batch, out, dicts):
        s = x["semseg"]
        img, sem, classes, masks, boxes, i = L.semantic_mapper(d["_arrays"][0], d["_arrays"][2], s.resized, s.origins, s.crop, s.flip, 32, 255,
                                                               max_area)
        np.testing.assert_array_equal(o["image"].cpu().numpy(), img)
        assert o["sem_seg"].dtype == torch.int64
        np.testing.assert_array_equal(o["sem_seg"].cpu().numpy(), sem)
        inst = o["instances"]
        np.testing.assert_array_equal(inst.gt_classes.cpu().numpy(), classes)
        np.testing.assert_array_equal(inst.gt_masks.cpu().numpy(), masks)
        np.testing.assert_array_equal(inst.gt_boxes.tensor.cpu().numpy(), boxes)
        assert tuple(inst.image_size) == (32, 32)
        padded += s.crop != (32, 32)
        flipped += s.flip
        later += i > 0
    assert padded and flipped, "the draws of this seed must cover a pad and a flip"
    if max_area < 1.0:
        assert later, "the draws of this seed must reject a first window"
    # the areas of label_bits are the chosen window's counts
    from mp_former_amd import label_input as LI
    _, targets = LI.semantic_batch(batch, 4, 255, max_area, device=dev)
    for t in targets:
        assert t["areas"].cpu().tolist() == t["counts"].tolist() and isinstance(t["params"], A.SemSegParams)
    model = _Stub(dev)
    P.install_native_semantic_input(model, mapper)
    assert model.forward(batch) == 3
    assert torch.equal(model.seen[-1][2]["sem_seg"], out[2]["sem_seg"]) and "sem_seg_raw" not in model.seen[-1][2]
    model.training = False
    model.forward(batch)
    assert model.seen[-1] is batch
