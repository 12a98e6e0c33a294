"""GPU: the video training input (mp_former_amd.clip_input, csrc/clip_input.hip, the d2_plugin hook) against the numpy restatement
of the reference's video mapper and prepare_targets (tests/_clip_restate.py).  Every comparison is byte equality.

The kernel cases put every (source, resized size, flip) combination that fits a canvas into ONE launch per canvas, at the smallest
shapes that reach each edge: 64 x 64 is the kernel's tile, so the resized sizes sit at 63 / 64 / 65 on each axis, at 1 x 1, across
several tiles (100, 128, 129, 130) and scale one axis up while the other goes down; the source heights 37 (bit columns straddle the
64-bit words) and 64 (they do not); the canvas widths 144, 132 and 133 take the 16-byte, the 4-byte and the 1-byte store."""
import types

import numpy as np
import pytest
import torch

import _clip_restate as CR
import _codec_restate as C
import _label_restate as L

pytestmark = pytest.mark.gpu

RESIZED = ((64, 64), (63, 65), (65, 63), (100, 20), (20, 130), (1, 1), (128, 129))
CANVASES = ((130, 144), (128, 132), (131, 133), (64, 64))


@pytest.fixture(scope="module")
def dev():
    import __graft_entry__ as g
    g.build()
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _sources():
    g = np.random.default_rng(17)
    out = [g.random((37, 45)) < 0.45, g.random((64, 40)) < 0.3, np.zeros((37, 45), dtype=bool), np.ones((64, 40), dtype=bool)]
    for y, x in ((0, 0), (0, 44), (36, 0), (36, 44)):        # a single set pixel in each source corner
        m = np.zeros((37, 45), dtype=bool)
        m[y, x] = True
        out.append(m)
    return out


SOURCES = _sources()


def _bits(mask, dev):
    return torch.from_numpy(L.pack(mask[None])[0].copy()).to(dev)


def _params(src, resized, flip):
    from mp_former_amd.augment import SemSegParams
    return SemSegParams(tuple(src), tuple(resized), (0, 0), tuple(resized), tuple(resized), bool(flip), tuple(resized))


def _launch_cases(canvas, dev):
    """-> (planes for resample_mask_bits, the expected bool [P, Hc, Wc])"""
    planes, want = [], []
    for i, m in enumerate(SOURCES):
        b = _bits(m, dev)
        for resized in RESIZED:
            if resized[0] > canvas[0] or resized[1] > canvas[1]:
                continue
            for flip in (False, True):
                planes.append((b, m.shape, _params(m.shape, resized, flip)))
                want.append(CR.pad_to(CR.resize_mask(m, resized, flip), canvas))
        if m.shape[0] <= canvas[0] and m.shape[1] <= canvas[1]:
            planes.append((b, m.shape, None))                # an identity plane next to table planes of other source sizes
            want.append(CR.pad_to(m, canvas))
        if i == 1:
            planes.append((None, None, None))                # an empty plane through a NULL src
            want.append(np.zeros(canvas, dtype=bool))
    return planes, np.stack(want)


@pytest.mark.parametrize("canvas", CANVASES, ids=lambda c: "canvas%dx%d" % c)
def test_resample_mask_bits_equals_decode_resize_flip_pad(dev, canvas):
    from mp_former_amd import clip_input as CI
    planes, want = _launch_cases(canvas, dev)
    P = len(planes)
    assert P > 8
    out = torch.full((P,) + canvas, 0xFF, dtype=torch.uint8, device=dev)     # the pad must be WRITTEN: 0 after a 0xFF pre-fill
    masks, areas = CI.resample_mask_bits(planes, canvas, device=dev, out=out)
    assert masks.dtype == torch.bool and tuple(masks.shape) == (P,) + canvas and masks.data_ptr() == out.data_ptr()
    assert areas.dtype == torch.int32 and tuple(areas.shape) == (P,)
    want_t = torch.from_numpy(want.astype(np.uint8)).to(dev)
    assert torch.equal(out, want_t), [i for i in range(P) if not torch.equal(out[i], want_t[i])][:8]
    assert torch.equal(areas.cpu(), torch.from_numpy(want.reshape(P, -1).sum(axis=1).astype(np.int32)))      # the popcount
    assert int(areas.max()) > 0 and int(areas.min()) == 0
    # a fresh output, twice: bit-identical; and the records in a permuted dst order
    a, aa = CI.resample_mask_bits(planes, canvas, device=dev)
    b, ba = CI.resample_mask_bits(planes, canvas, device=dev)
    assert torch.equal(a.view(torch.uint8), out) and torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and torch.equal(aa, ba)
    perm = np.random.default_rng(3).permutation(P)
    c, ca = CI.resample_mask_bits(planes, canvas, device=dev, dst=perm.tolist())
    idx = torch.from_numpy(perm).to(dev)
    assert torch.equal(c[idx].view(torch.uint8), out) and torch.equal(ca[idx], areas)


def test_resample_mask_bits_edges(dev):
    from mp_former_amd import clip_input as CI
    masks, areas = CI.resample_mask_bits([], (40, 48), device=dev)           # P == 0: nothing launched
    assert tuple(masks.shape) == (0, 40, 48) and masks.dtype == torch.bool and tuple(areas.shape) == (0,)
    m = SOURCES[0]
    b = _bits(m, dev)
    masks, areas = CI.resample_mask_bits([(None, None, None), (b, m.shape, None)], (37, 45), device=dev)
    assert not masks[0].any() and int(areas[0]) == 0
    assert torch.equal(masks[1].cpu(), torch.from_numpy(m)) and int(areas[1]) == int(m.sum())
    # a size pair where PIL's accumulated rule is not (int)((x + 0.5) * in / out): 2 -> 7 columns
    two = np.array([[True, False]] * 14)
    got, _ = CI.resample_mask_bits([(_bits(two, dev), two.shape, _params(two.shape, (49, 7), False))], (49, 7), device=dev)
    np.testing.assert_array_equal(got[0].cpu().numpy(), CR.resize_mask(two, (49, 7), False))
    assert got[0, 0].tolist() == [True] * 4 + [False] * 3                   # the multiplied form would give 3 + 4
    with pytest.raises(ValueError, match="smaller than the size"):
        CI.resample_mask_bits([(b, m.shape, _params(m.shape, (50, 50), False))], (49, 50), device=dev)
    with pytest.raises(ValueError, match="parameters say"):
        CI.resample_mask_bits([(b, m.shape, _params((36, 45), (50, 50), False))], (50, 50), device=dev)
    with pytest.raises(ValueError, match="must be int64"):
        CI.resample_mask_bits([(b[:-1], m.shape, None)], (50, 50), device=dev)
    with pytest.raises(ValueError, match="permutation"):
        CI.resample_mask_bits([(b, m.shape, None)] * 2, (50, 50), device=dev, dst=[0, 0])


# ---- clips ------------------------------------------------------------------------------------------------------------------------------
K = 40                                                       # num_classes: the class of a dummy row


def _rle(mask, form):
    counts = C.encode(mask)
    if form == "str":
        counts = C.to_string(counts)
    elif form == "bytes":
        counts = C.to_string(counts).encode("ascii")
    return {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": counts}


def _blob(shape, y0, y1, x0, x1):
    m = np.zeros(shape, dtype=bool)
    m[y0:y1, x0:x1] = True
    return m


def _clips():
    """two clips of different source sizes, with 2 and 3 frames -> the samples of clip_batch and the (src, geometry) of each"""
    g = np.random.default_rng(23)
    # clip A: 37 x 45, two frames, the second one reduced and flipped
    srcA, geoA = (37, 45), [((30, 36), False), ((20, 24), True)]
    rows_kept = set(L.nearest_pil(37, 20).tolist())
    lost_row = next(y for y in range(37) if y not in rows_kept)              # a source row the 37 -> 20 resize never reads
    speck = np.zeros(srcA, dtype=bool)
    speck[lost_row, 10] = True
    a0 = [
        {"id": 7, "category_id": 3, "iscrowd": 0, "segmentation": _rle(_blob(srcA, 4, 20, 5, 30), "list")},
        {"id": 3, "category_id": 8, "iscrowd": 0, "segmentation": _rle(_blob(srcA, 22, 33, 2, 12), "str")},
        {"id": 20, "category_id": 1, "iscrowd": 1, "segmentation": _rle(_blob(srcA, 0, 37, 0, 45), "list")},      # a crowd: a dummy row
        {"id": 9, "category_id": 6, "iscrowd": 0, "segmentation": _rle(np.zeros(srcA, dtype=bool), "list")},        # empty everywhere
        {"id": 30, "category_id": 2, "iscrowd": 0, "segmentation": _rle(g.random(srcA) < 0.3, "bytes")},           # leaves after frame 0
        {"id": 15, "category_id": 4, "iscrowd": 0, "segmentation": [[6.2, 3.1, 40.7, 5.5, 33.0, 30.9, 8.4, 26.0], [1.0, 1.0, 9.5, 1.5, 4.0, 8.0]]},
    ]
    a1 = [
        {"id": 7, "category_id": 3, "iscrowd": 0, "segmentation": _rle(_blob(srcA, 6, 25, 8, 35), "str")},
        {"id": 3, "category_id": 8, "iscrowd": 0, "segmentation": _rle(speck, "list")},                            # shrinks to nothing: id -1
        {"id": 12, "category_id": 5, "iscrowd": 0, "segmentation": _rle(g.random(srcA) < 0.5, "list")},            # enters in frame 1
        {"id": 20, "category_id": 1, "iscrowd": 1, "segmentation": _rle(_blob(srcA, 0, 37, 0, 45), "list")},
        {"id": 9, "category_id": 6, "iscrowd": 0, "segmentation": _rle(np.zeros(srcA, dtype=bool), "str")},
        {"id": 15, "category_id": 4, "iscrowd": 0, "segmentation": [[10.0, 10.0, 30.0, 12.0, 20.5, 33.3]]},
    ]
    # clip B: 64 x 40, three frames, the last one enlarged
    srcB, geoB = (64, 40), [((48, 30), True), ((48, 30), False), ((70, 44), True)]
    b = [[{"id": 101, "category_id": 11, "iscrowd": 0, "segmentation": _rle(g.random(srcB) < 0.4, "list")},
          {"id": 205, "category_id": 12, "iscrowd": 0, "segmentation": [[2.0, 3.0, 35.5, 6.0, 30.0, 60.0, 5.0, 50.5]]}] for _ in range(3)]
    b[1] = b[1][:1]                                                                                              # 205 is away in frame 1
    samples = []
    for src, geo, annos in ((srcA, geoA, [a0, a1]), (srcB, geoB, b)):
        samples.append({"image_raw": [torch.from_numpy(g.integers(0, 256, size=src + (3,), dtype=np.uint8)) for _ in geo],
                        "clip": tuple(_canvas32(_params(src, r, f)) for r, f in geo), "annotations": annos, "num_classes": K})
    return samples, [(srcA, geoA), (srcB, geoB)]


def _canvas32(p):
    import dataclasses
    return dataclasses.replace(p, canvas=tuple((v + 31) // 32 * 32 for v in p.resized))


CANVAS = (96, 64)                                            # the largest frame (70 x 44) rounded up to 32


@pytest.fixture(scope="module")
def clips():
    samples, geometry = _clips()
    frames = [CR.clip_instances(s["annotations"], src, geo, K) for s, (src, geo) in zip(samples, geometry)]
    return samples, geometry, frames


def test_restated_clip_has_every_case(clips):
    _, _, frames = clips
    ids = np.stack([f[1] for f in frames[0]], axis=1)        # clip A [G, F]
    rows = {tuple(r) for r in ids.tolist()}
    assert (7, 7) in rows and (3, -1) in rows and (-1, 12) in rows and (30, -1) in rows and (15, 15) in rows
    assert sum(tuple(r) == (-1, -1) for r in ids.tolist()) == 2    # the crowd and the mask that is empty everywhere: dropped
    last = dict(zip(ids[:, 0].tolist(), frames[0][-1][0].tolist()))
    assert last[30] == K and last[7] == 3                    # the clip's classes are the LAST frame's: a dummy where 30 has left


def test_clip_batch_equals_the_restated_mapper_and_prepare_targets(dev, clips):
    from mp_former_amd import clip_input as CI
    from mp_former_amd.video_losses import prepare_video_targets
    samples, geometry, frames = clips
    got_frames, targets = CI.clip_batch(samples, device=dev)
    assert got_frames.dtype == torch.uint8 and tuple(got_frames.shape) == (5, 3) + CANVAS and len(targets) == 2
    mean, std = [123.675, 116.280, 103.530], [58.395, 57.120, 57.375]
    norm, _ = CI.clip_batch(samples, dtype=torch.float32, mean=mean, std=std, device=dev)
    at = 0
    for s, (src, geo), fr, t in zip(samples, geometry, frames, targets):
        imgs = [im.numpy() for im in s["image_raw"]]
        assert t["frames"] == (at, at + len(geo))
        assert torch.equal(got_frames[at:at + len(geo)].cpu(), CR.clip_frames(imgs, geo, CANVAS))
        want = CR.clip_frames(imgs, geo, CANVAS, mean, std)
        assert torch.equal(norm[at:at + len(geo)].cpu().view(torch.int32), want.view(torch.int32))
        at += len(geo)
        ref = CR.prepare_targets(fr, CANVAS)
        lib = prepare_video_targets([torch.from_numpy(f[2]).to(dev) for f in fr], [torch.from_numpy(f[1]).to(dev) for f in fr],
                                    torch.from_numpy(fr[-1][0]).to(dev), CANVAS)
        assert t["masks"].dtype == torch.bool and t["labels"].dtype == torch.int64 and t["ids"].dtype == torch.int64
        for k in ("labels", "ids", "masks"):
            assert torch.equal(t[k].cpu(), ref[k]), k
            assert torch.equal(t[k], lib[k]), k
    assert targets[0]["ids"].shape == (5, 2) and targets[1]["ids"].shape == (2, 3)
    again_frames, again = CI.clip_batch(samples, device=dev)
    assert torch.equal(again_frames, got_frames) and all(torch.equal(a["masks"], t["masks"]) for a, t in zip(again, targets))


def test_clip_targets_keeps_the_mappers_rows(dev, clips):
    from mp_former_amd import clip_input as CI
    samples, geometry, frames = clips
    for s, (src, geo), fr in zip(samples, geometry, frames):
        t = CI.clip_targets(s["annotations"], s["clip"], K, canvas=CANVAS, device=dev)
        G = len(fr[0][0])
        assert tuple(t["masks"].shape) == (G, len(geo)) + CANVAS and len(t["tubes"]) == G
        for f, (classes, ids, masks, boxes) in enumerate(fr):
            assert torch.equal(t["gt_classes"][f].cpu(), torch.from_numpy(classes))
            assert torch.equal(t["gt_ids"][f].cpu(), torch.from_numpy(ids))
            assert t["gt_boxes"][f].dtype == torch.float32 and torch.equal(t["gt_boxes"][f].cpu(), torch.from_numpy(boxes))
            want = np.stack([CR.pad_to(m, CANVAS) for m in masks]) if G else np.zeros((0,) + CANVAS, dtype=bool)
            assert torch.equal(t["masks"][:, f].cpu(), torch.from_numpy(want))
            assert torch.equal(t["areas"][:, f].cpu(), torch.from_numpy(masks.reshape(G, -1).sum(axis=1).astype(np.int32)))
    empty = CI.clip_targets([[], []], samples[0]["clip"], K, device=dev)     # a clip without annotations
    assert tuple(empty["masks"].shape) == (0, 2, 32, 64) and tuple(empty["gt_ids"][1].shape) == (0,)


# ---- the detectron2 level ---------------------------------------------------------------------------------------------------------------
def _stub_model(dev):
    seen = []
    model = types.SimpleNamespace(device=dev, training=True)
    model.forward = lambda batched_inputs: seen.append(batched_inputs) or "inner"
    return model, seen


def test_install_native_video_input_hands_the_reference_form_on(dev, clips):
    from mp_former_amd import d2_plugin as P
    samples, geometry, frames = clips
    model, seen = _stub_model(dev)
    batch = [dict(s, video_id=i, file_names=["f%d" % f for f in range(len(s["clip"]))]) for i, s in enumerate(samples)]
    P.install_native_video_input(model)
    assert model.forward(batch) == "inner" and len(seen) == 1
    for i, (d, s, (src, geo), fr) in enumerate(zip(seen[0], samples, geometry, frames)):
        assert d["video_id"] == i and len(d["file_names"]) == len(geo) and "image_raw" not in d and "annotations" not in d
        want_img = CR.clip_frames([im.numpy() for im in s["image_raw"]], geo, CANVAS)
        for f, ((h, w), _) in enumerate(geo):
            img, inst = d["image"][f], d["instances"][f]
            assert img.dtype == torch.uint8 and tuple(img.shape) == (3, h, w) and img.device == dev
            assert torch.equal(img.cpu(), want_img[f, :, :h, :w])
            classes, ids, masks, boxes = fr[f]
            assert tuple(inst.image_size) == (h, w) and len(inst) == len(ids)
            assert torch.equal(inst.gt_classes.cpu(), torch.from_numpy(classes)) and torch.equal(inst.gt_ids.cpu(), torch.from_numpy(ids))
            assert inst.gt_masks.tensor.dtype == torch.bool and torch.equal(inst.gt_masks.tensor.cpu(), torch.from_numpy(masks))
            assert torch.equal(inst.gt_boxes.tensor.cpu(), torch.from_numpy(boxes))
    model.training = False                                   # eval is passed through untouched
    assert model.forward(batch) == "inner" and seen[1] is batch


def test_the_hook_composes_with_install_native_video_training(dev, clips):
    from mp_former_amd import d2_plugin as P
    samples, geometry, frames = clips
    model, seen = _stub_model(dev)
    old_matcher = types.SimpleNamespace(cost_class=2.0, cost_mask=5.0, cost_dice=5.0, num_points=64)
    model.criterion = types.SimpleNamespace(num_classes=K, matcher=old_matcher, weight_dict={"loss_ce": 2.0}, eos_coef=0.1,
                                            losses=["labels", "masks"], num_points=64, oversample_ratio=3.0,
                                            importance_sample_ratio=0.75, empty_weight=torch.ones(K + 1, device=dev), training=True)
    model.prepare_targets = None
    P.install_native_video_training(model)
    P.install_native_video_input(model)
    model.forward(samples)
    got = model.prepare_targets(seen[0], types.SimpleNamespace(tensor=torch.zeros((5, 3) + CANVAS, device=dev)))
    for t, fr in zip(got, frames):
        ref = CR.prepare_targets(fr, CANVAS)
        for k in ("labels", "ids", "masks"):
            assert torch.equal(t[k].cpu(), ref[k]), k
