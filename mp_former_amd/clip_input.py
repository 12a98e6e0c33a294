"""Video training input on the device: what the reference's ``YTVISDatasetMapper`` (mask2former_video/data_video/dataset_mapper.py:
114-269, augmentations in data_video/augmentation.py) does on the CPU per sampled frame — a PIL bilinear resize of the frame, a
``mask_util.decode`` of every instance's RLE, a PIL nearest resize and a flip of every dense mask, ``BitMasks`` and
``get_bounding_boxes`` — and the padded copy of ``VideoMaskFormer.prepare_targets`` (video_maskformer_model.py:227-253), from the
decoded frames, the annotations as the json holds them and one geometry record per frame.  Every result is an integer.

* ``sample_clip_frames`` / ``draw_clip``: the mapper's frame sampling and the two augmentations' draws, in their order.
* ``resample_mask_bits``: ONE launch (csrc/clip_input.hip) for every (tube, frame) plane of a batch: packed bits (the layout of
  ``inference.pack_masks``, as ``inference.rle_bits`` / ``polygon_bits`` leave them) -> the nearest resize by PIL's rule, the
  output-side flip and the pad, written as bool bytes straight into the [P, Hc, Wc] store, and the areas.  No dense intermediate.
* ``clip_targets``: the target half of one clip, in the mapper's tube order, with its dummy rows and ``-1`` ids.
* ``clip_batch``: a batch of clips end to end: one ``augment.resample_images`` launch for all frames, one ``rle_bits`` / one
  ``polygon_bits`` pass per distinct size, one mask launch for all planes -> the frames and the dicts of
  ``video_losses.prepare_video_targets``.  ``clip_batch_instances``: the same batch as per-frame classes, ids, boxes and views of
  the store, the form the reference's mapper leaves a clip in (``d2_plugin.native_video_inputs``).

There is no CPU path: a CPU device raises.
"""
import dataclasses
import random

import numpy as np
import torch

from . import _lib
from .augment import LSJParams, SemSegParams, _i32, nearest_table_pil, resample_images, shortest_edge_size, transform_polygons

SAMPLE_STYLES = ("range", "choice", "range_by_clip", "choice_by_clip")
FLIP_MODES = ("none", "horizontal", "flip_by_clip")
MAX_PLANES = 65535                              # planes per launch (the grid's z extent); a longer list is an error, not split
_REC_WORDS = 10                                 # MpfMaskBitsRecord in int32 words: the pointer (2), then 8 fields


# ---- the draws --------------------------------------------------------------------------------------------------------------------------
def sample_clip_frames(length, num, frame_range, shuffle, py_rng=random, np_rng=np.random):
    """The frames of one training clip (dataset_mapper.py:187-201), in the mapper's draw order: ``py_rng.randrange(length)`` is the
    reference frame, ``np_rng.choice`` draws ``num - 1`` more from the window of ``frame_range`` frames on either side of it (the
    reference frame itself excluded) WITH replacement, as ``numpy.random.choice`` defaults: a frame can repeat.  Sorted, then
    ``py_rng.shuffle`` where ``shuffle``.  A one-frame video with ``num > 1`` raises what numpy raises for an empty population."""
    length, num, frame_range = int(length), int(num), int(frame_range)
    ref = py_rng.randrange(length)
    start, end = max(0, ref - frame_range), min(length, ref + frame_range + 1)
    selected = np_rng.choice(np.array(list(range(start, ref)) + list(range(ref + 1, end))), num - 1)
    selected = sorted(selected.tolist() + [ref])
    if shuffle:
        py_rng.shuffle(selected)
    return [int(i) for i in selected]


def _draw_size(short_edge_length, is_range, rng):
    size = rng.randint(short_edge_length[0], short_edge_length[1] + 1) if is_range else rng.choice(list(short_edge_length))
    if size == 0:
        raise ValueError("draw_clip: a drawn short edge of 0 (detectron2's NoOpTransform: the frame keeps its size) is not "
                         "implemented on the device path")
    return int(size)


def _round_up(n, d):
    return (n + d - 1) // d * d if d > 1 else n


def draw_clip(h, w, num_frames, short_edge_length, max_size, sample_style="choice_by_clip", random_flip="flip_by_clip",
              size_divisibility=32, rng=np.random):
    """The geometry of the ``num_frames`` frames of one clip -> a tuple of ``augment.SemSegParams`` (the video mapper's order is the
    semantic mapper's: resize, then a flip of the RESULT; the crop is the whole resized frame).  The draws are those of
    data_video/augmentation.py in its order, per frame the size and then the flip: ``"range"`` (``rng.randint(min, max + 1)``) and
    ``"choice"`` (``rng.choice``) draw for every frame, ``"range_by_clip"`` / ``"choice_by_clip"`` once, at frame 0;
    ``random_flip``: ``"none"`` (nothing drawn), ``"horizontal"`` (``rng.uniform() < 0.5`` per frame) or ``"flip_by_clip"`` (once,
    at frame 0).  ``canvas`` is the frame's own size rounded up to ``size_divisibility``; the batch takes the maximum over its
    frames, which is ``ImageList.from_tensors``' size.  ValueError for a drawn size of 0 and for ``"vertical"``."""
    if sample_style not in SAMPLE_STYLES:
        raise ValueError(f"draw_clip: sample_style must be one of {SAMPLE_STYLES}, got {sample_style!r}")
    if random_flip == "vertical":
        raise ValueError("draw_clip: INPUT.RANDOM_FLIP 'vertical': only the horizontal flip is implemented on the device path")
    if random_flip not in FLIP_MODES:
        raise ValueError(f"draw_clip: random_flip must be one of {FLIP_MODES}, got {random_flip!r}")
    if isinstance(short_edge_length, int):
        short_edge_length = (short_edge_length, short_edge_length)
    is_range = "range" in sample_style
    if is_range and len(short_edge_length) != 2:
        raise ValueError(f"draw_clip: {sample_style!r} needs (min, max), got {short_edge_length!r}")
    h, w, d = int(h), int(w), int(size_divisibility)
    size_every = 1 if "by_clip" not in sample_style else int(num_frames)
    flip_every = 1 if random_flip == "horizontal" else int(num_frames)
    size, flip, out = None, False, []
    for f in range(int(num_frames)):
        if f % size_every == 0:
            size = _draw_size(short_edge_length, is_range, rng)
        if random_flip != "none" and f % flip_every == 0:
            flip = bool(rng.uniform() < 0.5)
        rh, rw = shortest_edge_size(h, w, size, max_size)
        out.append(SemSegParams((h, w), (rh, rw), (0, 0), (rh, rw), (rh, rw), flip, (_round_up(rh, d), _round_up(rw, d))))
    return tuple(out)


# ---- the kernel's wrapper ---------------------------------------------------------------------------------------------------------------
def _device(tensors, device, what):
    if device is None:
        device = next((t.device for t in tensors if t is not None and t.is_cuda), "cuda")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{what}: Not implemented on the CPU (device tensors only)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def resample_mask_bits(planes, canvas, device=None, dst=None, out=None):
    """``planes``: P triples ``(bits, (src_h, src_w), params)``.  ``bits``: the plane's packed words, an int64 [nwords] device row in
    the layout of ``inference.pack_masks`` at the source size (a row of ``rle_bits`` / ``polygon_bits``), or None for an empty plane;
    ``params``: the frame's ``SemSegParams`` (the mask is resized from the source size to ``params.resized`` by PIL's NEAREST rule,
    ``augment.nearest_table_pil``: detectron2's ``ResizeTransform.apply_segmentation`` on a uint8 mask, not torch's rule; then its
    columns are mirrored where ``params.flip``), or None for the identity (the plane was rasterised at its final size already).
    ``canvas`` (Hc, Wc) -> (masks bool [P, Hc, Wc], areas int32 [P]) in ONE launch: 0 outside the resized rectangle, every byte
    written.  ``dst``: a permutation, plane i is written to row dst[i] (default: in order); ``out``: a contiguous bool / uint8
    [P, Hc, Wc] device tensor to write instead of a new one."""
    planes = list(planes)
    P, Hc, Wc = len(planes), int(canvas[0]), int(canvas[1])
    if Hc <= 0 or Wc <= 0 or Hc * Wc >= 1 << 31:
        raise ValueError(f"resample_mask_bits: the canvas must be positive and below 2^31 elements, got {Hc} x {Wc}")
    if P > MAX_PLANES:
        raise ValueError(f"resample_mask_bits: at most {MAX_PLANES} planes per launch, got {P}")
    dst = list(range(P)) if dst is None else [int(i) for i in dst]
    if sorted(dst) != list(range(P)):
        raise ValueError("resample_mask_bits: dst must be a permutation of 0 .. P-1")
    tables, tab_len, rows = {}, 0, []

    def table(n_in, n_out):
        nonlocal tab_len
        if (n_in, n_out) not in tables:
            tables[(n_in, n_out)] = (tab_len, nearest_table_pil(n_in, n_out))
            tab_len += n_out
        return tables[(n_in, n_out)][0]

    for i, (bits, size, p) in enumerate(planes):
        if bits is None:
            rows.append(None)
            continue
        sh, sw = int(size[0]), int(size[1])
        if sh <= 0 or sw <= 0 or sh * sw >= 1 << 31:
            raise ValueError(f"resample_mask_bits: plane {i} has the source size {sh} x {sw}")
        if bits.dtype != torch.int64 or bits.dim() != 1 or bits.shape[0] != (sh * sw + 63) // 64:
            raise ValueError(f"resample_mask_bits: plane {i} must be int64 [{(sh * sw + 63) // 64}] for a {sh} x {sw} mask, got "
                             f"{bits.dtype} {tuple(bits.shape)}")
        if p is None:
            vh, vw, flip, xo, yo = sh, sw, 0, -1, -1
        else:
            if tuple(p.src) != (sh, sw):
                raise ValueError(f"resample_mask_bits: plane {i} is {sh} x {sw} but its parameters say {tuple(p.src)}")
            if tuple(p.offset) != (0, 0) or tuple(p.crop) != tuple(p.resized) or tuple(p.valid) != tuple(p.resized):
                raise ValueError(f"resample_mask_bits: plane {i}: a clip frame is the whole resized frame (no crop)")
            (vh, vw), flip = p.resized, int(p.flip)
            xo, yo = table(sw, vw), table(sh, vh)
        if vh <= 0 or vw <= 0 or vh > Hc or vw > Wc:
            raise ValueError(f"resample_mask_bits: the canvas {Hc} x {Wc} is smaller than the size {vh} x {vw} of plane {i}")
        rows.append((bits, sh, sw, vh, vw, flip, xo, yo))
    dev = _device([b for b, _, _ in planes] + [out], device, "resample_mask_bits")
    if out is None:
        out = torch.empty((P, Hc, Wc), dtype=torch.bool, device=dev)
    elif (out.dtype not in (torch.bool, torch.uint8) or tuple(out.shape) != (P, Hc, Wc) or not out.is_contiguous()
          or out.device != dev):
        raise ValueError(f"resample_mask_bits: out must be a contiguous bool or uint8 [{P}, {Hc}, {Wc}] tensor on {dev}")
    areas = torch.empty(P, dtype=torch.int32, device=dev)
    if P == 0:
        return out.view(torch.bool), areas
    nrec = P * _REC_WORDS
    pinned = torch.empty(nrec + tab_len, dtype=torch.int32, pin_memory=True)
    host = pinned.numpy()
    recs = host[:nrec].reshape(P, _REC_WORDS)
    keep = []                                                # the source rows stay alive until the launch is enqueued
    for i, row in enumerate(rows):
        if row is None:
            recs[i] = (0, 0, 0, 0, 0, 0, 0, -1, -1, dst[i])
            continue
        bits, sh, sw, vh, vw, flip, xo, yo = row
        if bits.device != dev or bits.stride(0) != 1:
            bits = bits.to(dev).contiguous()
        keep.append(bits)
        addr = bits.data_ptr()
        recs[i] = (_i32(addr), _i32(addr >> 32), sh, sw, vh, vw, flip, xo, yo, dst[i])
    for off, tab in tables.values():
        host[nrec + off:nrec + off + len(tab)] = tab
    staged = pinned.to(dev, non_blocking=True)
    _lib.call("mpf_mask_bits_resample", dev, pinned.data_ptr(), staged.data_ptr(), pinned.data_ptr() + 4 * nrec,
              staged.data_ptr() + 4 * nrec, tab_len, P, out.data_ptr(), areas.data_ptr(), Hc, Wc, _lib.stream_ptr(dev))
    # the source rows and the staging buffer are read by the launch just enqueued: the caching allocator gives their memory to later
    # work of this stream only, which runs after it
    return out.view(torch.bool), areas


# ---- one clip's targets -----------------------------------------------------------------------------------------------------------------
def _flip_free(p):
    return LSJParams(False, p.src, p.resized, (0, 0), p.resized, p.resized)


def _plan(frame_annotations, params, num_classes, who):
    """the host half of one clip -> (tube ids in the mapper's order, classes [F][G], ids [F][G], entries [G][F]); an entry is None
    (absent: the reference's dummy annotation, whose all-zero polygon rasterises to nothing), ("rle", dict, frame) or ("poly", the
    rings transformed to the resized frame, frame)"""
    F = len(params)
    if len(frame_annotations) != F:
        raise ValueError(f"{who}: {len(frame_annotations)} frames of annotations but {F} parameter records")
    _ids = set()                                             # dataset_mapper.py:209-214: a set, enumerated as it iterates
    for annos in frame_annotations:
        _ids.update([a["id"] for a in annos])
    index = {_id: i for i, _id in enumerate(_ids)}
    G = len(index)
    classes = [[int(num_classes)] * G for _ in range(F)]
    ids = [[-1] * G for _ in range(F)]
    entries = [[None] * F for _ in range(G)]
    for f, (annos, p) in enumerate(zip(frame_annotations, params)):
        for a in annos:
            if a.get("iscrowd", 0) != 0:
                continue
            g = index[a["id"]]
            classes[f][g], ids[f][g] = int(a["category_id"]), int(a["id"])
            segm = a["segmentation"]
            if isinstance(segm, dict):
                if tuple(int(v) for v in segm["size"]) != tuple(p.src):
                    raise ValueError(f"{who}: an RLE of size {tuple(segm['size'])} in a frame of {tuple(p.src)}")
                entries[g][f] = ("rle", segm, f)
            elif isinstance(segm, (list, tuple)):
                rings = transform_polygons(segm, _flip_free(p))       # ResizeTransform.apply_coords, then HFlipTransform's
                if p.flip:
                    for r in rings:
                        r[0::2] = p.resized[1] - r[0::2]
                entries[g][f] = ("poly", rings, f)
            else:
                raise ValueError(f"{who}: a segmentation must be an RLE dict or a list of polygons, got {type(segm).__name__}")
    return list(index), classes, ids, entries


def _boxes(masks):
    """BitMasks.get_bounding_boxes of bool [P, H, W] -> float32 [P, 4] (x0, y0, x1 + 1, y1 + 1), zeros for an empty mask"""
    P, H, W = masks.shape
    dev = masks.device
    out = torch.zeros((P, 4), dtype=torch.float32, device=dev)
    if P == 0:
        return out
    for k, (hit, n) in enumerate(((masks.any(dim=1), W), (masks.any(dim=2), H))):
        at = torch.arange(n, device=dev, dtype=torch.int32)
        out[:, k] = torch.where(hit, at, n).amin(dim=1)
        out[:, k + 2] = torch.where(hit, at, -1).amax(dim=1) + 1
    out[out[:, 2] <= 0] = 0
    return out


def _run(plans, all_params, canvas, dev):
    """every plane of a batch of planned clips -> per clip (masks [G, F, Hc, Wc], areas [G, F]): one ``rle_bits`` pass per source
    size, one ``polygon_bits`` pass per resized size, ONE resample launch"""
    from .inference import polygon_bits, rle_bits
    rle, poly, where = {}, {}, []
    for (_, _, _, entries), params in zip(plans, all_params):
        for row in entries:
            for f, e in enumerate(row):
                if e is None:
                    where.append(None)
                elif e[0] == "rle":
                    group = rle.setdefault(tuple(params[f].src), [])
                    where.append(("rle", tuple(params[f].src), len(group), params[f]))
                    group.append(e[1])
                else:
                    group = poly.setdefault(tuple(params[f].resized), [])
                    where.append(("poly", tuple(params[f].resized), len(group), None))
                    group.append(e[1])
    bits = {("rle", size): rle_bits(group, size, device=dev) for size, group in rle.items()}
    bits.update({("poly", size): polygon_bits(group, size, device=dev) for size, group in poly.items()})
    planes = [(None, None, None) if w is None else (bits[(w[0], w[1])][w[2]], w[1], w[3]) for w in where]
    masks, areas = resample_mask_bits(planes, canvas, device=dev)
    out, at = [], 0
    for (tubes, _, _, _), params in zip(plans, all_params):
        G, F = len(tubes), len(params)
        out.append((masks[at:at + G * F].view(G, F, *masks.shape[1:]), areas[at:at + G * F].view(G, F)))
        at += G * F
    return out


def _frame_fields(plan, masks, areas, dev):
    """-> (classes int64 [F, G], ids int64 [F, G] with -1 where the plane is empty: ``filter_empty_instances``, a non-empty mask
    has a non-empty box) from ONE upload"""
    _, classes, ids, _ = plan
    both = torch.tensor([classes, ids], dtype=torch.int64).to(dev, non_blocking=True)
    if both.dim() != 3:                                      # no tube at all
        both = both.reshape(2, len(classes), 0)
    return both[0], torch.where(areas.t() > 0, both[1], -1)


def _frame_targets(plan, masks, areas, dev):
    classes, ids = _frame_fields(plan, masks, areas, dev)
    G, F = masks.shape[:2]
    boxes = _boxes(masks.flatten(0, 1)).view(G, F, 4)
    return {"gt_classes": list(classes.unbind(0)), "gt_ids": list(ids.unbind(0)), "gt_boxes": list(boxes.unbind(1)), "masks": masks,
            "areas": areas, "tubes": plan[0]}


def clip_targets(frame_annotations, params, num_classes, canvas=None, device=None):
    """The target half of one clip.  ``frame_annotations``: per sampled frame the list of its annotations as the json holds them
    (``id``, ``category_id``, ``iscrowd``, ``segmentation``: an RLE dict with counts as list, str or bytes, or polygons);
    ``params``: the frames' ``SemSegParams``; ``canvas`` (default: the largest frame canvas).  Tube order is the mapper's own: the
    ids of ALL annotations of the sampled frames in a Python ``set``, enumerated; crowd annotations are dropped after that.  RLEs go
    through ``inference.rle_bits`` at the source size and the kernel, polygons through ``augment.transform_polygons`` (the flip
    applied after the scale, as the mapper's transforms do) and ``inference.polygon_bits`` at the resized size and the kernel with
    identity tables.  An instance absent from a frame is an empty plane with id -1 and class ``num_classes``.
    -> {"gt_classes": F x int64 [G], "gt_ids": F x int64 [G] (-1 where the resized mask is empty), "gt_boxes": F x float32 [G, 4]
    (x0, y0, x1 + 1, y1 + 1), "masks": bool [G, F, Hc, Wc], "areas": int32 [G, F], "tubes": the G ids}."""
    params = tuple(params)
    dev = _device([], device, "clip_targets")
    plan = _plan(frame_annotations, params, num_classes, "clip_targets")
    if canvas is None:
        canvas = (max(p.canvas[0] for p in params), max(p.canvas[1] for p in params))
    (masks, areas), = _run([plan], [params], canvas, dev)
    return _frame_targets(plan, masks, areas, dev)


# ---- a batch of clips -------------------------------------------------------------------------------------------------------------------
def _video_targets(classes, ids, masks):
    """``video_losses.prepare_video_targets`` on the store the kernel wrote: the tubes whose id is -1 in every frame are dropped;
    the count of the kept ones is the one value read back"""
    ids = ids.t().contiguous()                               # [G, F]
    valid = (ids != -1).any(dim=-1)
    if int(valid.sum()) == ids.shape[0]:                     # (G' is read back, as the boolean index of the reference does)
        return {"labels": classes[-1], "ids": ids, "masks": masks}
    return {"labels": classes[-1][valid], "ids": ids[valid], "masks": masks[valid]}


def _batch(samples, dtype, mean, std, device, who):
    """-> (frames [sum F, 3, Hc, Wc], per clip (plan, params, masks [G, F, Hc, Wc], areas [G, F]))"""
    samples = list(samples)
    all_params = [tuple(s["clip"]) for s in samples]
    for i, (s, params) in enumerate(zip(samples, all_params)):
        if len(s["image_raw"]) != len(params) or not params:
            raise ValueError(f"{who}: clip {i} has {len(s['image_raw'])} frames but {len(params)} parameter records")
    images = [im for s in samples for im in s["image_raw"]]
    dev = _device(images, device, who)
    flat = [p for params in all_params for p in params]
    plans = [_plan(s.get("annotations", [[] for _ in params]), params, s["num_classes"], who) for s, params in zip(samples, all_params)]
    if not samples:
        return resample_images([], [], dtype=dtype, mean=mean, std=std, device=dev), []
    canvas = (max(p.canvas[0] for p in flat), max(p.canvas[1] for p in flat))
    # ImageList.from_tensors pads the NORMALISED frames with 0: the record's own pad rectangle (filled with the pad value, then
    # normalised) is the frame itself, everything else on the canvas is 0
    frames = resample_images(images, [dataclasses.replace(p, canvas=p.resized) for p in flat], dtype=dtype, mean=mean, std=std,
                             canvas=canvas, pad_value=0, device=dev)
    return frames, [(plan, params, masks, areas) for plan, params, (masks, areas) in zip(plans, all_params, _run(plans, all_params, canvas, dev))]


def clip_batch(samples, dtype=torch.uint8, mean=None, std=None, device=None):
    """B samples, each a dict with "image_raw" (F uint8 [H, W, 3] frames), "clip" (F ``SemSegParams``: ``draw_clip``),
    "annotations" (per frame, as ``clip_targets`` takes them) and "num_classes" -> (frames [sum F, 3, Hc, Wc] in sample order:
    uint8, or normalised as ``augment.resample_images`` does, 0 in the pad, as ``ImageList.from_tensors`` leaves it; a list of B
    dicts in the form ``video_losses.prepare_video_targets`` returns: "labels" [G'] (the LAST frame's classes, as that function
    documents), "ids" [G', F], "masks" bool [G', F, Hc, Wc]; also "frames": the clip's (first, last + 1) rows of the frames).
    The canvas is the largest frame canvas of the batch.  One image launch for all frames, one ``rle_bits`` and one
    ``polygon_bits`` pass per distinct size, one mask launch for all planes; only G' is read back, per clip."""
    frames, clips = _batch(samples, dtype, mean, std, device, "clip_batch")
    targets, at = [], 0
    for plan, params, masks, areas in clips:
        classes, ids = _frame_fields(plan, masks, areas, frames.device)
        t = _video_targets(classes, ids, masks)
        t["frames"] = (at, at + len(params))
        at += len(params)
        targets.append(t)
    return frames, targets


def clip_batch_instances(samples, device=None):
    """The same batch in the form the reference's mapper leaves a clip in (the detectron2 route, d2_plugin.native_video_inputs) ->
    (frames uint8 [sum F, 3, Hc, Wc], per clip the dict of ``clip_targets`` plus "frames"): per-frame classes, ids and boxes, and
    the padded store, of which frame f's ``gt_masks`` is the view ``masks[:, f, :h, :w]``."""
    frames, clips = _batch(samples, torch.uint8, None, None, device, "clip_batch_instances")
    out, at = [], 0
    for plan, params, masks, areas in clips:
        out.append(dict(_frame_targets(plan, masks, areas, frames.device), frames=(at, at + len(params))))
        at += len(params)
    return frames, out
