"""Large-scale-jitter training input on the device: what the reference's ``COCOInstanceNewBaselineDatasetMapper``
(mask2former/data/dataset_mappers/coco_instance_new_baseline_dataset_mapper.py) does on the CPU with PIL and pycocotools — a random
horizontal flip, ``ResizeScale``, ``FixedSizeCrop`` with pad value 128, then a dense mask per polygon — from the decoded source
image, a few KB of vertices and one geometry record per image.

* ``resample_images`` is the image half (csrc/img_resample.hip): ONE launch for a batch, integer-equal to PIL's 8-bit bilinear
  resize (detectron2's ``ResizeTransform.apply_image`` for uint8) of the flipped image, cropped and padded; only the crop window is
  computed.  As uint8, or already normalised (fp32 bit-equal to ``(x - pixel_mean) / pixel_std``, or bf16) on the zero canvas of
  ``ImageList.from_tensors``.
* ``lsj_targets`` / ``lsj_batch`` are the annotation half: the polygons transformed on the host in float64 as detectron2's
  transforms do (no clipping), rasterised by ``inference.polygon_bits`` at the crop size, unpacked by ``inference.unpack_masks``.
* ``resize_scale_size`` / ``fixed_crop`` / ``shortest_edge_size`` / ``draw_lsj`` are detectron2's geometry in numpy float64.

The supported range is a source / resized ratio of at most ``MAX_RATIO`` (64) per axis: the tile height is chosen per image so that
a tile's source rows fit the kernel's LDS buffer (``SPAN_ROWS`` rows).  There is no CPU path: a CPU device raises.
"""
import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib

MAX_RATIO = 64          # mpf_img_resample_max_ratio()
SPAN_ROWS = 256         # mpf_img_resample_span_rows(): source rows of one tile held in LDS
_TILE_HS = (32, 16, 8, 4, 2, 1)
_REC_WORDS = 22         # MpfResampleRecord in int32 words: the pointer (2), then 20 fields
_PRECISION_BITS = 22


# ---- PIL's coefficient tables ---------------------------------------------------------------------------------------------------------
def resample_coeffs(in_size, out_size, first=0, count=None):
    """PIL's bilinear (triangle filter) tables of one axis for the outputs ``first .. first + count`` of ``out_size`` ->
    (coef int32 [count, ksize], bounds int32 [count, 2] = (first source index, tap count)), in double as ``precompute_coeffs`` and
    ``normalize_coeffs_8bpc`` compute them."""
    in_size, out_size, first = int(in_size), int(out_size), int(first)
    count = out_size - first if count is None else int(count)
    if in_size <= 0 or out_size <= 0 or first < 0 or count < 0 or first + count > out_size:
        raise ValueError(f"resample_coeffs: need sizes > 0 and 0 <= first <= first + count <= out_size, got {in_size}, {out_size}, {first}, {count}")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)           # (int) truncates; the operand is > -1
    xmax = np.minimum((center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.float64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((x + xmin[:, None] - center[:, None] + 0.5) / fs))
    w[np.arange(ksize)[None, :] >= xmax[:, None]] = 0.0
    ww = np.zeros(count, dtype=np.float64)
    for t in range(ksize):                                                    # PIL's left-to-right sum
        ww = ww + w[:, t]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    coef = (0.5 + w * float(1 << _PRECISION_BITS)).astype(np.int64).astype(np.int32)
    coef[np.arange(ksize)[None, :] >= xmax[:, None]] = 0
    return coef, np.stack([xmin, xmax], axis=1).astype(np.int32)


# ---- detectron2's geometry --------------------------------------------------------------------------------------------------------------
def resize_scale_size(h, w, scale, target_h, target_w):
    """``ResizeScale._get_resize``: the size (h', w') of an h x w image at ``scale`` of the target"""
    target_scale = np.multiply((target_h, target_w), scale)
    r = np.minimum(target_scale[0] / h, target_scale[1] / w)
    out = np.round(np.multiply((h, w), r)).astype(int)
    return int(out[0]), int(out[1])


def fixed_crop(rh, rw, sh, sw, u):
    """``FixedSizeCrop`` of an rh x rw image to sh x sw with the draw ``u`` in [0, 1) -> ((off_y, off_x), (valid_h, valid_w))"""
    max_offset = np.maximum(np.subtract((rh, rw), (sh, sw)), 0)
    offset = np.round(np.multiply(max_offset, u)).astype(int)
    valid = np.minimum(np.subtract((rh, rw), offset), (sh, sw))
    return (int(offset[0]), int(offset[1])), (int(valid[0]), int(valid[1]))


def shortest_edge_size(h, w, size, max_size):
    """``ResizeShortestEdge.get_output_shape``: the evaluation mappers' size"""
    scale = size * 1.0 / min(h, w)
    newh, neww = (size, scale * w) if h < w else (scale * h, size)
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


@dataclass(frozen=True)
class LSJParams:
    """The geometry of one image: all a worker has to decide, and all the device needs besides the pixels and the vertices."""
    flip: bool
    src: tuple          # (H, W) of the source
    resized: tuple      # (h', w')
    offset: tuple       # (y0, x0) of the crop inside the resized image
    crop: tuple         # (Sh, Sw)
    valid: tuple        # min(resized - offset, crop)


def lsj_params(h, w, flip, scale, u, image_size=1024):
    """The parameters of one image from the three draws"""
    sh, sw = (image_size, image_size) if np.isscalar(image_size) else (int(image_size[0]), int(image_size[1]))
    rh, rw = resize_scale_size(h, w, scale, sh, sw)
    offset, valid = fixed_crop(rh, rw, sh, sw, u)
    return LSJParams(bool(flip), (int(h), int(w)), (rh, rw), offset, (int(sh), int(sw)), valid)


def draw_lsj(h, w, image_size=1024, min_scale=0.1, max_scale=2.0, flip=True, rng=np.random):
    """Draw in the reference's order (``RandomFlip``, ``ResizeScale``, ``FixedSizeCrop``): the flip decision ``uniform() < 0.5``
    (not drawn with ``flip=False``), the scale ``uniform(min, max)``, the crop's ``uniform(0, 1)``.  ``rng``: a
    ``numpy.random.Generator``, a ``RandomState`` or the ``numpy.random`` module."""
    do_flip = bool(rng.uniform() < 0.5) if flip else False
    scale = rng.uniform(min_scale, max_scale)
    u = rng.uniform(0.0, 1.0)
    return lsj_params(h, w, do_flip, scale, u, image_size)


# ---- label maps: the nearest-neighbour rules, the semantic mapper's draws and crop rule ---------------------------------------------
def nearest_table_pil(in_size, out_size):
    """The source index PIL's ``Image.resize(..., NEAREST)`` reads for each of ``out_size`` outputs of an axis of ``in_size`` -> int32
    [out_size]: detectron2's ``ResizeTransform.apply_segmentation`` on a uint8 array (the panoptic PNG).  ``ImagingScaleAffine``
    starts a double at ``0.5 * in / out`` and ADDS ``in / out`` once per output; the index is the C truncation of the running sum
    (which differs from ``(int)((x + 0.5) * in / out)`` where the accumulated rounding crosses an integer)."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size <= 0 or out_size <= 0:
        raise ValueError(f"nearest_table_pil: sizes must be positive, got {in_size}, {out_size}")
    step = in_size / out_size
    steps = np.full(out_size, step, dtype=np.float64)
    steps[0] = 0.0 + step * 0.5
    acc = np.cumsum(steps)                                   # sequential double additions, as the C loop's ``xo += a[0]``
    # PIL leaves an output whose coordinate falls outside the source untouched; after the clamp below none does
    return np.minimum(acc.astype(np.int64), in_size - 1).astype(np.int32)


_TORCH_NEAREST = {}


def nearest_table_torch(in_size, out_size):
    """The source index ``F.interpolate(mode="nearest")`` reads on a float64 CPU tensor -> int32 [out_size]: the route detectron2's
    ``ResizeTransform`` takes for the reference's semantic mapper, which converts the label map to ``double`` first.  Taken from torch
    itself (an ``arange`` of the axis interpolated as a [1, 1, 1, in] tensor), so it is the installed torch's rule by construction;
    the rule is the same on either axis and inside a 2-D map."""
    key = (int(in_size), int(out_size))
    if key[0] <= 0 or key[1] <= 0:
        raise ValueError(f"nearest_table_torch: sizes must be positive, got {key[0]}, {key[1]}")
    t = _TORCH_NEAREST.get(key)
    if t is None:
        src = torch.arange(key[0], dtype=torch.float64).view(1, 1, 1, key[0])
        t = torch.nn.functional.interpolate(src, size=(1, key[1]), mode="nearest").view(-1).to(torch.int32).numpy()
        if len(_TORCH_NEAREST) > 4096:
            _TORCH_NEAREST.clear()
        _TORCH_NEAREST[key] = t
    return t


def draw_shortest_edge(h, w, short_edge_length, max_size, sample_style="range", rng=np.random):
    """``ResizeShortestEdge.get_transform``: the draw (``"range"``: ``rng.randint(min, max + 1)``; ``"choice"``:
    ``rng.choice(list)``), then ``shortest_edge_size`` -> (h', w').  A drawn size of 0 keeps the image, as detectron2's NoOp."""
    if isinstance(short_edge_length, int):
        short_edge_length = (short_edge_length, short_edge_length)
    if sample_style == "range":
        if len(short_edge_length) != 2:
            raise ValueError(f"draw_shortest_edge: 'range' needs (min, max), got {short_edge_length!r}")
        size = rng.randint(short_edge_length[0], short_edge_length[1] + 1)
    elif sample_style == "choice":
        size = rng.choice(list(short_edge_length))
    else:
        raise ValueError(f"draw_shortest_edge: sample_style must be 'range' or 'choice', got {sample_style!r}")
    if size == 0:
        return int(h), int(w)
    return shortest_edge_size(h, w, int(size), max_size)


def crop_size_absolute(crop_size, image_size):
    """``RandomCrop.get_crop_size`` for ``CROP.TYPE == "absolute"``: (min(ch, h), min(cw, w))"""
    return min(int(crop_size[0]), int(image_size[0])), min(int(crop_size[1]), int(image_size[1]))


def crop_size(crop_type, crop_size, image_size):
    """The crop size of ``CROP.TYPE``; only ``"absolute"`` is built, the others raise NotImplementedError naming the type"""
    if crop_type == "absolute":
        return crop_size_absolute(crop_size, image_size)
    raise NotImplementedError(f"INPUT.CROP.TYPE {crop_type!r}: only 'absolute' is implemented on the device path")


def choose_category_crop(counts, tries, single_category_max_area):
    """detectron2's ``RandomCrop_CategoryAreaConstraint`` acceptance rule on integer counts.  ``counts`` [tries, K]: per candidate
    window the pixel count of every non-ignored label.  For try i, cnt = the non-zero counts; the first i with ``len(cnt) > 1 and
    cnt.max() < cnt.sum() * single_category_max_area`` is taken, the last try if none passes.  With ``single_category_max_area >=
    1.0`` there is one draw and no test -> the index of the chosen try."""
    if single_category_max_area >= 1.0:
        return 0
    counts = np.asarray(counts)
    tries = int(tries)
    if counts.ndim != 2 or tries < 1 or counts.shape[0] < tries:
        raise ValueError(f"choose_category_crop: counts must be [tries, K] with tries >= 1, got {counts.shape} for {tries} tries")
    for i in range(tries):
        cnt = counts[i][counts[i] > 0]
        if len(cnt) > 1 and np.max(cnt) < np.sum(cnt) * single_category_max_area:
            return i
    return tries - 1


@dataclass(frozen=True)
class SemSegParams:
    """The geometry of one image of the semantic mapper, whose order is resize -> crop -> flip -> pad to ``size_divisibility``: the
    flip mirrors the CROPPED image (the valid columns), after the resize."""
    src: tuple          # (H, W) of the source
    resized: tuple      # (h', w') of ResizeShortestEdge
    offset: tuple       # (y0, x0) of the chosen crop window inside the resized image
    crop: tuple         # (ch, cw) of the window
    valid: tuple        # = crop: an absolute crop never leaves the resized image
    flip: bool
    canvas: tuple       # what the mapper pads to, at the bottom right


@dataclass(frozen=True)
class SemSegDraw:
    """All a worker draws for one image of the semantic mapper: the resized size, the window size, every candidate origin (the
    category-area rule picks one of them on the device side, from the counts) and the flip."""
    src: tuple
    resized: tuple
    crop: tuple         # (ch, cw)
    origins: tuple      # ((y0, x0), ...): ``tries`` candidates, one where the rule is off
    flip: bool
    canvas: tuple

    def params(self, i):
        return SemSegParams(self.src, self.resized, tuple(self.origins[i]), self.crop, self.crop, self.flip, self.canvas)


CROP_TRIES = 10         # RandomCrop_CategoryAreaConstraint.get_transform: ``for _ in range(10)``


def draw_semseg(h, w, short_edge_length, max_size, sample_style="range", crop=None, crop_type="absolute",
                single_category_max_area=1.0, flip=True, size_divisibility=-1, rng=np.random):
    """Draw for the reference's semantic mapper: the short edge, the crop origins (``randint(h' - ch + 1)`` then ``randint(w' - cw +
    1)`` per try), the flip ``uniform() < 0.5``.  ``crop``: (ch, cw) or None (cropping disabled: the whole resized image is the one
    window).  ALL ``CROP_TRIES`` origins are drawn up front where the category-area rule applies (``single_category_max_area < 1``):
    the windows have the reference's distribution, but the reference stops drawing at the first accepted window, so the RNG stream
    is consumed differently."""
    rh, rw = draw_shortest_edge(h, w, short_edge_length, max_size, sample_style, rng)
    if crop is None:
        ch, cw, origins = rh, rw, ((0, 0),)
    else:
        ch, cw = crop_size(crop_type, crop, (rh, rw))
        tries = 1 if single_category_max_area >= 1.0 else CROP_TRIES
        origins = tuple((int(rng.randint(rh - ch + 1)), int(rng.randint(rw - cw + 1))) for _ in range(tries))
    do_flip = bool(rng.uniform() < 0.5) if flip else False
    canvas = (int(size_divisibility), int(size_divisibility)) if size_divisibility > 0 else (ch, cw)
    return SemSegDraw((int(h), int(w)), (rh, rw), (ch, cw), origins, do_flip, canvas)


def resize_params(h, w, size):
    """No flip, no crop: the whole resized image (the evaluation route)"""
    rh, rw = int(size[0]), int(size[1])
    return LSJParams(False, (int(h), int(w)), (rh, rw), (0, 0), (rh, rw), (rh, rw))


# ---- the image ------------------------------------------------------------------------------------------------------------------------
def _tile_h(ybounds):
    """the largest tile height whose tiles tap at most SPAN_ROWS source rows each"""
    ends = ybounds[:, 0] + ybounds[:, 1]
    n = len(ybounds)
    for th in _TILE_HS:
        first = np.arange(0, n, th)
        last = np.minimum(first + th, n) - 1
        if int((ends[last] - ybounds[first, 0]).max()) <= SPAN_ROWS:
            return th
    raise ValueError("resample_images: one output row taps more than %d source rows" % SPAN_ROWS)


def _check_params(p, i):
    H, W = p.src
    for name, (a, b) in (("src", p.src), ("resized", p.resized), ("crop", p.crop), ("valid", p.valid)):
        if a <= 0 or b <= 0:
            raise ValueError(f"resample_images: image {i} has a non-positive {name} size {a} x {b}")
    if H > MAX_RATIO * p.resized[0] or W > MAX_RATIO * p.resized[1]:
        raise ValueError(f"resample_images: image {i} is reduced {H} x {W} -> {p.resized[0]} x {p.resized[1]}: the ratio per axis is "
                         f"limited to {MAX_RATIO}")
    for k in (0, 1):
        if p.offset[k] < 0 or p.valid[k] > p.crop[k] or p.offset[k] + p.valid[k] > p.resized[k]:
            raise ValueError(f"resample_images: image {i}: the valid extent {p.valid} at {p.offset} must lie inside the crop {p.crop} and "
                             f"the resized image {p.resized}")


def resample_images(images, params, dtype=torch.uint8, mean=None, std=None, canvas=None, pad_value=128, device=None):
    """``images``: a list of uint8 [H, W, 3] tensors (host tensors are uploaded, device tensors are read in place, any row stride);
    ``params``: their ``LSJParams`` (a flip mirrors the source before the resize) or ``SemSegParams`` (a flip mirrors the valid
    columns of the crop after it, and the pad value fills the record's own ``canvas``, as the semantic mapper pads to the size
    divisibility) -> [B, 3, Hc, Wc] on the device in ONE launch.  ``canvas`` (Hc, Wc) defaults to the largest crop
    (``SemSegParams``: the largest ``canvas``).
    uint8: PIL's value, ``pad_value`` in the rest of the crop rectangle.  float32 (needs ``mean`` and ``std``, three values each):
    ``(v - mean[c]) / std[c]`` bit-equal to the torch expression, 0 outside the crop rectangle; bfloat16: that rounded to nearest
    even.  ValueError before any device work for a non-uint8 or non-[H, W, 3] source, a canvas smaller than a crop, float output
    without mean / std and a ratio above ``MAX_RATIO``."""
    images, params = list(images), list(params)
    if len(images) != len(params):
        raise ValueError(f"resample_images: {len(images)} images but {len(params)} parameter records")
    if dtype not in (torch.uint8, torch.float32, torch.bfloat16):
        raise TypeError(f"resample_images: dtype must be uint8, float32 or bfloat16, got {dtype}")
    if dtype != torch.uint8 and (mean is None or std is None):
        raise ValueError("resample_images: float output needs mean and std")
    if not 0 <= int(pad_value) <= 255:
        raise ValueError(f"resample_images: pad_value must be 0 .. 255, got {pad_value}")
    for i, (im, p) in enumerate(zip(images, params)):
        if im.dtype != torch.uint8:
            raise ValueError(f"resample_images: image {i} must be uint8, got {im.dtype}")
        if im.dim() != 3 or im.shape[2] != 3:
            raise ValueError(f"resample_images: image {i} must be [H, W, 3] (3 channels), got {tuple(im.shape)}")
        if tuple(im.shape[:2]) != tuple(p.src):
            raise ValueError(f"resample_images: image {i} is {tuple(im.shape[:2])} but its parameters say {tuple(p.src)}")
        _check_params(p, i)
    if canvas is None:
        sizes = [p.canvas if isinstance(p, SemSegParams) else p.crop for p in params]
        canvas = (max([c[0] for c in sizes], default=1), max([c[1] for c in sizes], default=1))
    Hc, Wc = int(canvas[0]), int(canvas[1])
    for i, p in enumerate(params):
        if p.crop[0] > Hc or p.crop[1] > Wc:
            raise ValueError(f"resample_images: the canvas {Hc} x {Wc} is smaller than the crop {p.crop[0]} x {p.crop[1]} of image {i}")
        if isinstance(p, SemSegParams) and (p.canvas[0] > Hc or p.canvas[1] > Wc or p.crop[0] > p.canvas[0] or p.crop[1] > p.canvas[1]):
            raise ValueError(f"resample_images: image {i}: the crop {p.crop} must fit its canvas {p.canvas}, and that the batch's {Hc} x {Wc}")
    mean_c = std_c = None
    if dtype != torch.uint8:
        mean_v = [float(v) for v in torch.as_tensor(mean).reshape(-1).tolist()]
        std_v = [float(v) for v in torch.as_tensor(std).reshape(-1).tolist()]
        if len(mean_v) != 3 or len(std_v) != 3:
            raise ValueError("resample_images: mean and std must hold three values")
        mean_c, std_c = (ctypes.c_float * 3)(*mean_v), (ctypes.c_float * 3)(*std_v)
    if device is None:
        device = next((im.device for im in images if im.is_cuda), "cuda")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("resample_images: Not implemented on the CPU (device tensors only)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    B = len(images)
    out = torch.empty((B, 3, Hc, Wc), dtype=dtype, device=dev)
    if B == 0:
        return out
    srcs = []
    for im in images:
        im = im.to(dev, non_blocking=True) if not im.is_cuda or im.device != dev else im
        if im.stride(2) != 1 or im.stride(1) != 3 or im.stride(0) < 3 * im.shape[1]:
            im = im.contiguous()
        srcs.append(im)
    # the staging buffer: the records, then every image's four tables, all int32, filled in place in pinned memory (the tables by
    # the library's host code: PIL's arithmetic in C, a few microseconds per axis)
    lib = _lib.lib()
    nrec = B * _REC_WORDS
    layout, n = [], 0
    for p in params:
        kx, ky = lib.mpf_img_resample_ksize(p.src[1], p.resized[1]), lib.mpf_img_resample_ksize(p.src[0], p.resized[0])
        offs = (n, n + p.valid[1] * kx, n + p.valid[1] * (kx + 2), n + p.valid[1] * (kx + 2) + p.valid[0] * ky)
        n = offs[3] + 2 * p.valid[0]
        layout.append((kx, ky, offs))
    pinned = torch.empty(nrec + n, dtype=torch.int32, pin_memory=True)
    host, base = pinned.numpy(), pinned.data_ptr() + 4 * nrec
    recs = host[:nrec].reshape(B, _REC_WORDS)
    for b, (im, p, (kx, ky, offs)) in enumerate(zip(srcs, params, layout)):
        _lib.call("mpf_img_resample_tables", dev, p.src[1], p.resized[1], p.offset[1], p.valid[1], base + 4 * offs[0], base + 4 * offs[1])
        _lib.call("mpf_img_resample_tables", dev, p.src[0], p.resized[0], p.offset[0], p.valid[0], base + 4 * offs[2], base + 4 * offs[3])
        yb = host[nrec + offs[3]:nrec + offs[3] + 2 * p.valid[0]].reshape(-1, 2)
        addr = im.data_ptr()
        # LSJ mirrors the source, then crops; the semantic mapper mirrors the cropped result and pads it to ITS canvas with the pad
        # value: the record's pad rectangle is then that canvas
        sem = isinstance(p, SemSegParams)
        flip_in, flip_out = (0, int(p.flip)) if sem else (int(p.flip), 0)
        rect = p.canvas if sem else p.crop
        recs[b] = (_i32(addr), _i32(addr >> 32),
                   im.stride(0), p.src[0], p.src[1], flip_in, p.resized[0], p.resized[1], p.offset[0], p.offset[1],
                   rect[0], rect[1], p.valid[0], p.valid[1], _tile_h(yb), kx, ky, offs[0], offs[1], offs[2], offs[3], flip_out)
    staged = pinned.to(dev, non_blocking=True)
    _lib.call("mpf_img_resample", dev, pinned.data_ptr(), staged.data_ptr(), pinned.data_ptr() + 4 * nrec, staged.data_ptr() + 4 * nrec,
              n, B, out.data_ptr(), _lib.DTYPE[dtype], Hc, Wc, int(pad_value), mean_c, std_c, _lib.stream_ptr(dev))
    # the sources and the staging buffer are read by the launch just enqueued: the caching allocator gives their memory to later
    # work of this stream only, which runs after it
    return out


def _i32(v):
    """the low 32 bits of v as a signed int32"""
    v &= 0xffffffff
    return v - (1 << 32) if v >= 1 << 31 else v


def resize_image(image, size, dtype=torch.uint8, mean=None, std=None, canvas=None, device=None):
    """One uint8 [H, W, 3] image resized to ``size`` (h', w') as PIL does: no flip, no crop -> [3, Hc, Wc] (the evaluation route, with
    ``shortest_edge_size`` for the size)."""
    return resample_images([image], [resize_params(image.shape[0], image.shape[1], size)], dtype=dtype, mean=mean, std=std, canvas=canvas,
                           device=device)[0]


# ---- the annotations ------------------------------------------------------------------------------------------------------------------
def transform_polygons(polygons, params):
    """A list of rings [x0, y0, x1, y1, ...] through the transforms in their order, in float64 as detectron2's ``apply_coords``:
    flip ``x -> W - x``, scale ``x * (w' / W)``, ``y * (h' / H)``, crop ``- offset``.  No clipping; the pad is at the bottom right and
    shifts nothing."""
    H, W = params.src
    out = []
    for ring in polygons:
        a = np.array(ring, dtype=np.float64).reshape(-1, 2)
        if params.flip:
            a[:, 0] = W - a[:, 0]
        a[:, 0] = a[:, 0] * (params.resized[1] * 1.0 / W)
        a[:, 1] = a[:, 1] * (params.resized[0] * 1.0 / H)
        a[:, 0] -= params.offset[1]
        a[:, 1] -= params.offset[0]
        out.append(a.reshape(-1))
    return out


def _kept(annotations, params):
    """the mapper's filters on the host -> (labels, transformed polygons per instance, boxes float32 [T, 4])"""
    labels, polys, boxes = [], [], []
    for a in annotations:
        if a.get("iscrowd", 0) != 0:
            continue
        segm = a["segmentation"]
        if not isinstance(segm, (list, tuple)):
            raise ValueError("lsj_targets: only polygon segmentations are transformed (the reference's mapper asserts the same)")
        rings = transform_polygons(segm, params)
        if not rings:
            continue
        xy = np.concatenate(rings).reshape(-1, 2)
        box = np.concatenate([xy.min(axis=0), xy.max(axis=0)]).astype(np.float32)       # PolygonMasks.get_bounding_boxes (float32)
        if not (box[2] - box[0] > np.float32(1e-5) and box[3] - box[1] > np.float32(1e-5)):   # filter_empty_instances
            continue
        labels.append(int(a["category_id"]))
        polys.append(rings)
        boxes.append(box)
    return labels, polys, (np.stack(boxes) if boxes else np.zeros((0, 4), dtype=np.float32))


def _targets(labels, boxes, bits, size, dev):
    from .inference import unpack_masks
    return {"labels": torch.as_tensor(labels, dtype=torch.int64).to(dev), "bits": bits, "masks": unpack_masks(bits, size),
            "boxes": torch.from_numpy(boxes).to(dev)}


def lsj_targets(annotations, params, device="cuda"):
    """The annotations of one image -> {"labels" int64 [T], "bits" int64 [T, nwords], "masks" bool [T, Sh, Sw], "boxes" float32
    [T, 4]} on the device, as the reference's mapper leaves them: crowd annotations dropped, the polygons transformed and rasterised
    at the crop size, the boxes the min / max of the transformed vertices (xyxy, unclipped), instances whose box is not wider and
    taller than 1e-5 dropped.  An instance wholly outside the crop stays, with an all-zero mask."""
    from .inference import _codec_device, polygon_bits
    dev = _codec_device(device, "lsj_targets")
    labels, polys, boxes = _kept(annotations, params)
    return _targets(labels, boxes, polygon_bits(polys, params.crop, device=dev), params.crop, dev)


def lsj_batch(samples, dtype=torch.uint8, mean=None, std=None, canvas=None, pad_value=128, device=None):
    """B samples, each a dict with "image_raw" (uint8 [H, W, 3]), "lsj" (``LSJParams``) and optionally "annotations" ->
    (images [B, 3, Hc, Wc], a list of B target dicts as ``lsj_targets`` gives).  One resample launch, and where all images share the
    crop size (the LSJ configuration) one ``polygon_bits`` pass over the instances of the whole batch, split per image."""
    from .inference import polygon_bits
    samples = list(samples)
    params = [s["lsj"] for s in samples]
    images = resample_images([s["image_raw"] for s in samples], params, dtype=dtype, mean=mean, std=std, canvas=canvas,
                             pad_value=pad_value, device=device)
    dev = images.device
    kept = [_kept(s.get("annotations", ()), p) for s, p in zip(samples, params)]
    crops = {p.crop for p in params}
    if len(crops) != 1:
        return images, [_targets(lab, box, polygon_bits(pol, p.crop, device=dev), p.crop, dev) for (lab, pol, box), p in zip(kept, params)]
    crop = crops.pop()
    bits = polygon_bits([rings for _, pol, _ in kept for rings in pol], crop, device=dev)
    targets, t0 = [], 0
    for lab, pol, box in kept:
        targets.append(_targets(lab, box, bits[t0:t0 + len(pol)], crop, dev))
        t0 += len(pol)
    return images, targets
