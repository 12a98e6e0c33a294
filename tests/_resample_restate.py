"""A numpy restatement of PIL's 8-bit bilinear resize (ImagingResample, triangle filter) and of detectron2's large-scale-jitter
geometry, written from the rules alone and independent of mp_former_amd.augment: what tests/test_lsj_cpu.py pins to PIL and to
tests/golden/lsj_pil_resize.npz, and what the GPU tests compare the kernel with by integer equality."""
import math

import numpy as np

PRECISION_BITS = 22


def axis_tables(in_size, out_size):
    """-> (coef int32 [out, ksize], bounds int32 [out, 2] = (first source index, tap count)) of one axis"""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    coef = np.zeros((out_size, ksize), dtype=np.int32)
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(xmax)]
        ww = sum(w)
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            coef[xx, x] = int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return coef, bounds


def _pass(img, coef, bounds):
    """one pass along axis 1 of uint8 [H, W, C] -> uint8 [H, out, C]"""
    out = np.zeros((img.shape[0], coef.shape[0], img.shape[2]), dtype=np.uint8)
    src = img.astype(np.int64)
    for xx in range(coef.shape[0]):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = (1 << (PRECISION_BITS - 1)) + (src[:, x0:x0 + n, :] * coef[xx, :n].astype(np.int64)[None, :, None]).sum(axis=1)
        assert np.abs(acc).max() < 2 ** 31, "the sum must fit PIL's int"
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize(img, out_h, out_w):
    """PIL's Image.fromarray(img).resize((out_w, out_h), Image.BILINEAR) for uint8 [H, W, C]: the horizontal pass first, rounded to
    uint8, then the vertical pass on those bytes; a pass whose size does not change is skipped"""
    img = np.ascontiguousarray(img)
    H, W = img.shape[:2]
    if out_w != W:
        img = _pass(img, *axis_tables(W, out_w))
    if out_h != H:
        img = _pass(img.transpose(1, 0, 2), *axis_tables(H, out_h)).transpose(1, 0, 2)
    return np.ascontiguousarray(img)


# ---- detectron2's geometry ----------------------------------------------------------------------------------------------------------
def resize_scale_size(h, w, scale, target_h, target_w):
    r = min(target_h * scale / h, target_w * scale / w)
    return int(np.round(h * r)), int(np.round(w * r))


def fixed_crop(rh, rw, sh, sw, u):
    oy, ox = int(np.round(max(rh - sh, 0) * u)), int(np.round(max(rw - sw, 0) * u))
    return (oy, ox), (min(rh - oy, sh), min(rw - ox, sw))


def shortest_edge_size(h, w, size, max_size):
    scale = size * 1.0 / min(h, w)
    newh, neww = (size, scale * w) if h < w else (scale * h, size)
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def lsj_image(img, flip, resized, offset, crop, pad_value=128):
    """flip, resize, crop at ``offset``, pad at the bottom right to ``crop`` with ``pad_value`` -> uint8 [3, Sh, Sw]"""
    if flip:
        img = img[:, ::-1]
    full = resize(img, resized[0], resized[1])
    out = np.full((crop[0], crop[1], 3), pad_value, dtype=np.uint8)
    win = full[offset[0]:offset[0] + crop[0], offset[1]:offset[1] + crop[1]]
    out[:win.shape[0], :win.shape[1]] = win
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def transform_ring(ring, flip, src, resized, offset):
    """[x0, y0, x1, y1, ...] in float64 through flip (x -> W - x), scale (x w' / W, y h' / H), crop (minus the offset)"""
    a = np.asarray(ring, dtype=np.float64).reshape(-1, 2).copy()
    if flip:
        a[:, 0] = src[1] - a[:, 0]
    a[:, 0] = a[:, 0] * (resized[1] * 1.0 / src[1])
    a[:, 1] = a[:, 1] * (resized[0] * 1.0 / src[0])
    a[:, 0] -= offset[1]
    a[:, 1] -= offset[0]
    return a.reshape(-1)


def lsj_annotations(annotations, flip, src, resized, offset):
    """the non-crowd annotations -> (labels int64 [T], polygons (list of lists of transformed rings), boxes float32 [T, 4] xyxy): the
    box is the min / max of the transformed vertices, unclipped, and an instance is kept if its box is wider and taller than 1e-5"""
    labels, polys, boxes = [], [], []
    for a in annotations:
        if a.get("iscrowd", 0) != 0:
            continue
        rings = [transform_ring(r, flip, src, resized, offset) for r in a["segmentation"]]
        xy = np.concatenate(rings).reshape(-1, 2)
        box = np.concatenate([xy.min(axis=0), xy.max(axis=0)]).astype(np.float32)
        if not (box[2] - box[0] > np.float32(1e-5) and box[3] - box[1] > np.float32(1e-5)):
            continue
        labels.append(int(a["category_id"]))
        polys.append(rings)
        boxes.append(box)
    return (np.asarray(labels, dtype=np.int64), polys,
            np.stack(boxes) if boxes else np.zeros((0, 4), dtype=np.float32))
