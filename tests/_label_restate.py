"""A numpy restatement of the reference's panoptic and semantic training mappers on label maps, written from the rules alone and
independent of mp_former_amd.label_input: the two nearest-neighbour rules (PIL's for a uint8 array, torch's for a float64 tensor),
detectron2's ``RandomCrop_CategoryAreaConstraint`` with ``np.unique``, the mappers end to end (``_resample_restate.resize`` for the
image), and ``id == k`` masks packed in the column-major layout of ``inference.pack_masks``."""
import numpy as np
import torch

import _resample_restate as R


# ---- the two nearest rules ----------------------------------------------------------------------------------------------------------
def nearest_pil(in_size, out_size):
    """ImagingScaleAffine: a double starts at 0.5 * in / out and in / out is ADDED per output; the index is its C truncation"""
    step = in_size / out_size
    acc = 0.0 + step * 0.5
    idx = np.zeros(out_size, dtype=np.int64)
    for i in range(out_size):
        idx[i] = min(int(acc), in_size - 1)
        acc += step
    return idx


def nearest_torch(in_size, out_size):
    """what F.interpolate(mode="nearest") reads on a float64 tensor, asked of torch with a column (the H axis of a 2-D map)"""
    src = torch.arange(in_size, dtype=torch.float64).view(1, 1, in_size, 1).expand(1, 1, in_size, 2).contiguous()
    return torch.nn.functional.interpolate(src, size=(out_size, 2), mode="nearest")[0, 0, :, 1].to(torch.int64).numpy()


def resize_nearest(label, out_h, out_w, rule):
    """label [H, W] or [H, W, 3] -> [out_h, out_w(, 3)]"""
    f = {"pil": nearest_pil, "torch": nearest_torch}[rule]
    return label[f(label.shape[0], out_h)][:, f(label.shape[1], out_w)]


def rgb2id(rgb):
    rgb = rgb.astype(np.int64)
    return rgb[..., 0] + 256 * rgb[..., 1] + 65536 * rgb[..., 2]


# ---- the crop rule ------------------------------------------------------------------------------------------------------------------
def category_crop(sem_seg, origins, crop, ignore_label, max_area):
    """RandomCrop_CategoryAreaConstraint.get_transform on given origins -> the index of the window taken"""
    if max_area >= 1.0:
        return 0
    for i, (y0, x0) in enumerate(origins):
        labels, cnt = np.unique(sem_seg[y0:y0 + crop[0], x0:x0 + crop[1]], return_counts=True)
        cnt = cnt[labels != ignore_label]
        if len(cnt) > 1 and np.max(cnt) < np.sum(cnt) * max_area:
            return i
    return len(origins) - 1


def choose_from_counts(counts, max_area):
    """the same rule from per-window counts [tries, K] of the non-ignored labels"""
    if max_area >= 1.0:
        return 0
    for i, c in enumerate(counts):
        cnt = c[c > 0]
        if len(cnt) > 1 and np.max(cnt) < np.sum(cnt) * max_area:
            return i
    return len(counts) - 1


# ---- packed bits --------------------------------------------------------------------------------------------------------------------
def pack(masks):
    """bool [T, H, W] -> int64 [T, nwords]: position p = x * H + y, bit b of word j = position 64 j + b"""
    T, H, W = masks.shape
    nwords = (H * W + 63) // 64
    flat = np.zeros((T, nwords * 64), dtype=np.uint8)
    flat[:, :H * W] = masks.transpose(0, 2, 1).reshape(T, H * W)
    return np.packbits(flat.reshape(T, nwords, 64), axis=2, bitorder="little").view(np.uint64).reshape(T, nwords).view(np.int64)


def id_bits(id_map, ids):
    """-> (bits int64 [T, nwords], areas int64 [T]) of ``id_map == k`` for k in ids"""
    masks = np.stack([id_map == k for k in ids]) if len(ids) else np.zeros((0,) + id_map.shape, dtype=bool)
    return pack(masks), masks.reshape(len(ids), id_map.size).sum(axis=1)


def boxes(masks):
    """BitMasks.get_bounding_boxes: float32 (x0, y0, x1 + 1, y1 + 1), zeros for an empty mask"""
    out = np.zeros((len(masks), 4), dtype=np.float32)
    for i, m in enumerate(masks):
        ys, xs = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
        if len(xs) and len(ys):
            out[i] = (xs[0], ys[0], xs[-1] + 1, ys[-1] + 1)
    return out


# ---- the mappers --------------------------------------------------------------------------------------------------------------------
def label_lsj(label, flip, resized, offset, crop, pad, rule="pil"):
    """flip, nearest resize, crop at ``offset``, pad at the bottom right to ``crop`` -> [Sh, Sw(, 3)]"""
    if flip:
        label = label[:, ::-1]
    full = resize_nearest(label, resized[0], resized[1], rule)
    out = np.full((crop[0], crop[1]) + label.shape[2:], pad, dtype=label.dtype)
    win = full[offset[0]:offset[0] + crop[0], offset[1]:offset[1] + crop[1]]
    out[:win.shape[0], :win.shape[1]] = win
    return out


def panoptic_mapper(image, pan_rgb, segments_info, flip, resized, offset, crop):
    """COCOPanopticNewBaselineDatasetMapper for fixed draws -> (image uint8 [3, S, S], classes, masks bool [T, S, S], boxes)"""
    img = R.lsj_image(image, flip, resized, offset, crop, pad_value=128)
    pan = rgb2id(label_lsj(pan_rgb, flip, resized, offset, crop, 255, "pil"))
    keep = [s for s in segments_info if not s["iscrowd"]]
    masks = np.stack([pan == s["id"] for s in keep]) if keep else np.zeros((0,) + pan.shape, dtype=bool)
    return img, np.array([s["category_id"] for s in keep], dtype=np.int64), masks, boxes(masks)


def semantic_mapper(image, sem_seg, resized, origins, crop, flip, size_divisibility, ignore_label, max_area):
    """MaskFormerSemanticDatasetMapper for fixed draws: ResizeShortestEdge (bilinear image, torch-nearest float64 labels), the
    category-area crop among ``origins``, the flip of the CROP, the pad to ``size_divisibility`` -> (image uint8 [3, Hc, Wc], sem_seg
    int64 [Hc, Wc], classes, masks, boxes, the index of the window taken)"""
    img = R.resize(image, resized[0], resized[1])
    sem = resize_nearest(sem_seg.astype(np.float64), resized[0], resized[1], "torch")
    i = category_crop(sem, origins, crop, ignore_label, max_area)
    y0, x0 = origins[i]
    img, sem = img[y0:y0 + crop[0], x0:x0 + crop[1]], sem[y0:y0 + crop[0], x0:x0 + crop[1]]
    if flip:
        img, sem = img[:, ::-1], sem[:, ::-1]
    sem = sem.astype(np.int64)
    Hc, Wc = (size_divisibility, size_divisibility) if size_divisibility > 0 else crop
    img_p = np.full((Hc, Wc, 3), 128, dtype=np.uint8)
    img_p[:crop[0], :crop[1]] = img
    sem_p = np.full((Hc, Wc), ignore_label, dtype=np.int64)
    sem_p[:crop[0], :crop[1]] = sem
    classes = np.unique(sem_p)
    classes = classes[classes != ignore_label]
    masks = np.stack([sem_p == c for c in classes]) if len(classes) else np.zeros((0, Hc, Wc), dtype=bool)
    return np.ascontiguousarray(img_p.transpose(2, 0, 1)), sem_p, classes.astype(np.int64), masks, boxes(masks), i
