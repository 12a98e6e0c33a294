"""Panoptic and semantic training input on the device, from label maps: what the reference's ``COCOPanopticNewBaselineDatasetMapper``
(mask2former/data/dataset_mappers/coco_panoptic_new_baseline_dataset_mapper.py) and ``MaskFormerSemanticDatasetMapper``
(mask_former_semantic_dataset_mapper.py) do on the CPU per image — nearest-neighbour resize of the label map, detectron2's
``RandomCrop_CategoryAreaConstraint`` (``np.unique`` on up to ten windows), pad, one dense ``H x W`` mask per segment or class in a
Python loop, boxes — from the decoded map and one small geometry record (csrc/label_input.hip).  Every result is an integer.

* ``resample_labels``: ONE gather launch for a batch through host-made index tables (``augment.nearest_table_pil`` for the panoptic
  PNG, which detectron2 resizes with PIL; ``augment.nearest_table_torch`` for the semantic map, which the reference converts to
  double so that detectron2 resizes it with torch) -> int32 ids [B, Hc, Wc], the pad id outside the valid extent.
* ``window_counts``: the label histogram of every candidate crop window, read from the source (the resized map is never formed),
  back in ONE device-to-host copy per batch: the only host wait of the path.  ``augment.choose_category_crop`` picks the window on
  the host; the chosen window's counts are also the classes present and their areas.
* ``label_bits``: one image's id map and T wanted ids -> packed bits [T, nwords] in the layout of ``inference.pack_masks`` and areas
  [T] from one read of the map.  Boxes are ``inference.mask_boxes`` of the bits, dense masks ``inference.unpack_masks``.
* ``panoptic_lsj_batch`` / ``semantic_batch``: the two mappers end to end for a batch of worker dicts.

There is no CPU path: a CPU device raises.
"""
import numpy as np
import torch

from . import _lib
from .augment import (LSJParams, SemSegDraw, SemSegParams, _i32, _targets, choose_category_crop, nearest_table_pil,
                      nearest_table_torch, resample_images)

KINDS = {"u8": 0, "i32": 1, "rgb": 2}          # MPF_LABEL_U8 / _I32 / _RGB
PANOPTIC_PAD_ID = 0xFFFFFF                      # FixedSizeCrop pads segmentation with 255; rgb2id((255, 255, 255))
MAX_CLASSES = 1024                              # mpf_label_counts_max_classes()
MAX_TRIES = 16                                  # mpf_label_counts_max_tries()
MAX_IDS = 255                                   # mpf_label_bits_max_ids(): wanted ids per launch
_REC_WORDS = 18                                 # MpfLabelRecord in int32 words: the pointer (2), then 16 fields
_RULES = {"pil": nearest_table_pil, "torch": nearest_table_torch}


def _device(sources, device, what):
    if device is None:
        device = next((s.device for s in sources if s.is_cuda), "cuda")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"{what}: Not implemented on the CPU (device tensors only)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _rule(rule, params):
    """the nearest rule of a batch: given, or PIL's for LSJ records (the panoptic PNG) and torch's for the semantic mapper's"""
    if rule is None:
        rule = "torch" if params and all(isinstance(p, (SemSegParams, SemSegDraw)) for p in params) else "pil"
    if rule not in _RULES:
        raise ValueError(f"rule must be 'pil' or 'torch', got {rule!r}")
    return _RULES[rule]


def _check_sources(sources, params, kind, what):
    if kind not in KINDS:
        raise ValueError(f"{what}: kind must be one of {sorted(KINDS)}, got {kind!r}")
    if len(sources) != len(params):
        raise ValueError(f"{what}: {len(sources)} sources but {len(params)} parameter records")
    want = {"u8": (torch.uint8, 2), "i32": (torch.int32, 2), "rgb": (torch.uint8, 3)}[kind]
    for i, (s, p) in enumerate(zip(sources, params)):
        if s.dtype != want[0] or s.dim() != want[1] or (kind == "rgb" and s.shape[2] != 3):
            raise ValueError(f"{what}: source {i} is {s.dtype} {tuple(s.shape)}, not a {kind!r} map (one kind per batch: "
                             f"u8 = uint8 [H, W], i32 = int32 [H, W], rgb = uint8 [H, W, 3])")
        if tuple(s.shape[:2]) != tuple(p.src):
            raise ValueError(f"{what}: source {i} is {tuple(s.shape[:2])} but its parameters say {tuple(p.src)}")


def _upload(sources, kind, dev):
    """the sources on the device with a unit element stride -> (tensors, row strides in bytes)"""
    out, strides = [], []
    esz = {"u8": 1, "i32": 4, "rgb": 3}[kind]
    for s in sources:
        s = s.to(dev, non_blocking=True) if not s.is_cuda or s.device != dev else s
        inner_ok = (s.stride(2) == 1 and s.stride(1) == 3) if kind == "rgb" else s.stride(1) == 1
        if not inner_ok or s.stride(0) < (3 if kind == "rgb" else 1) * s.shape[1]:
            s = s.contiguous()
        out.append(s)
        strides.append(s.stride(0) * (4 if kind == "i32" else 1))
        assert strides[-1] >= esz * s.shape[1]
    return out, strides


def _stage(srcs, strides, params, kind, tables, extra=None):
    """the pinned staging buffer of a launch: the records, then each image's x and y table, then ``extra`` (int32) -> (pinned,
    offset of the tables, their length, offset of extra)"""
    B = len(srcs)
    nrec = B * _REC_WORDS
    offs, n = [], 0
    for tx, ty in tables:
        offs.append((n, n + len(tx)))
        n += len(tx) + len(ty)
    ne = 0 if extra is None else extra.size
    pinned = torch.empty(nrec + n + ne, dtype=torch.int32, pin_memory=True)
    host = pinned.numpy()
    recs = host[:nrec].reshape(B, _REC_WORDS)
    for b, (s, st, p, (tx, ty), (ox, oy)) in enumerate(zip(srcs, strides, params, tables, offs)):
        host[nrec + ox:nrec + ox + len(tx)] = tx
        host[nrec + oy:nrec + oy + len(ty)] = ty
        addr = s.data_ptr()
        flip_in, flip_out = (0, int(p.flip)) if isinstance(p, (SemSegParams, SemSegDraw)) else (int(p.flip), 0)
        off, valid = (p.offset, p.valid) if not isinstance(p, SemSegDraw) else ((0, 0), p.crop)
        recs[b] = (_i32(addr), _i32(addr >> 32), st, p.src[0], p.src[1], KINDS[kind], flip_in, flip_out, p.resized[0], p.resized[1],
                   off[0], off[1], p.crop[0], p.crop[1], valid[0], valid[1], ox, oy)
    if ne:
        host[nrec + n:] = extra.reshape(-1)
    return pinned, nrec, n, nrec + n


def resample_labels(sources, params, kind, pad_id, canvas=None, device=None, rule=None):
    """``sources``: label maps of one ``kind`` ("u8": uint8 [H, W]; "i32": int32 [H, W], what a worker makes of a uint16 / tif map;
    "rgb": the panoptic PNG uint8 [H, W, 3], read as R + 256 G + 65536 B), host tensors are uploaded; ``params``: their ``LSJParams``
    (a flip mirrors the source) or ``SemSegParams`` (a flip mirrors the valid columns of the crop) -> int32 [B, Hc, Wc] on the
    device in ONE launch: the nearest-neighbour resize, cropped, ``pad_id`` everywhere outside the valid extent.  ``rule``: "pil" or
    "torch" (default: by the record type).  ``canvas`` defaults to the largest crop (``SemSegParams``: canvas).  ValueError before
    any device work for a source that is not of ``kind`` (one kind per batch) or does not fit its record."""
    sources, params = list(sources), list(params)
    _check_sources(sources, params, kind, "resample_labels")
    for i, p in enumerate(params):
        if not isinstance(p, (LSJParams, SemSegParams)):
            raise TypeError(f"resample_labels: record {i} must be LSJParams or SemSegParams, got {type(p).__name__}")
        for name, (a, b) in (("src", p.src), ("resized", p.resized), ("crop", p.crop), ("valid", p.valid)):
            if a <= 0 or b <= 0:
                raise ValueError(f"resample_labels: image {i} has a non-positive {name} size {a} x {b}")
        for k in (0, 1):
            if p.offset[k] < 0 or p.valid[k] > p.crop[k] or p.offset[k] + p.valid[k] > p.resized[k]:
                raise ValueError(f"resample_labels: image {i}: the valid extent {p.valid} at {p.offset} must lie inside the crop "
                                 f"{p.crop} and the resized map {p.resized}")
    if not -(1 << 31) <= int(pad_id) < 1 << 31:
        raise ValueError(f"resample_labels: pad_id must fit int32, got {pad_id}")
    if canvas is None:
        sizes = [p.canvas if isinstance(p, SemSegParams) else p.crop for p in params]
        canvas = (max([c[0] for c in sizes], default=1), max([c[1] for c in sizes], default=1))
    Hc, Wc = int(canvas[0]), int(canvas[1])
    for i, p in enumerate(params):
        if p.crop[0] > Hc or p.crop[1] > Wc:
            raise ValueError(f"resample_labels: the canvas {Hc} x {Wc} is smaller than the crop {p.crop[0]} x {p.crop[1]} of image {i}")
    table = _rule(rule, params)
    dev = _device(sources, device, "resample_labels")
    B = len(sources)
    out = torch.empty((B, Hc, Wc), dtype=torch.int32, device=dev)
    if B == 0:
        return out
    srcs, strides = _upload(sources, kind, dev)
    tables = [(table(p.src[1], p.resized[1])[p.offset[1]:p.offset[1] + p.valid[1]],
               table(p.src[0], p.resized[0])[p.offset[0]:p.offset[0] + p.valid[0]]) for p in params]
    pinned, t0, n, _ = _stage(srcs, strides, params, kind, tables)
    staged = pinned.to(dev, non_blocking=True)
    _lib.call("mpf_label_resample", dev, pinned.data_ptr(), staged.data_ptr(), pinned.data_ptr() + 4 * t0, staged.data_ptr() + 4 * t0,
              n, B, out.data_ptr(), Hc, Wc, int(pad_id), _lib.stream_ptr(dev))
    return out


def window_counts(sources, params, windows, num_classes, ignore_label, kind=None, device=None, rule=None):
    """The label histogram of candidate crop windows.  ``sources`` / ``params`` as ``resample_labels`` (``SemSegDraw`` records are
    taken too: only ``src``, ``resized`` and the flip side are read); ``windows``: per image a list of ``tries`` windows (y0, x0, h,
    w) in RESIZED coordinates, the same number for every image; labels ``0 .. num_classes - 1`` are counted, ``ignore_label`` is
    skipped -> int32 [B, tries, num_classes] on the HOST (pinned).  ValueError if a window holds any other label: bad data is never
    clamped.  ``kind`` defaults to the sources' dtype ("u8" / "i32").

    The counts come back in ONE device-to-host copy per batch, and waiting for it is the only host wait of the whole input path: a
    caller who prefetches batches runs the path under a side stream (``with torch.cuda.stream(s):``; every launch and the copy go to
    the current stream), so the wait overlaps the training step on the main stream."""
    sources, params = list(sources), list(params)
    if kind is None:
        kind = "i32" if sources and sources[0].dtype == torch.int32 else "u8"
    _check_sources(sources, params, kind, "window_counts")
    K = int(num_classes)
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"window_counts: num_classes must be 1 .. {MAX_CLASSES}, got {num_classes}")
    B = len(sources)
    win = np.asarray(windows, dtype=np.int64).reshape(B, -1, 4) if B else np.zeros((0, 1, 4), dtype=np.int64)
    tries = win.shape[1]
    if not 1 <= tries <= MAX_TRIES:
        raise ValueError(f"window_counts: 1 .. {MAX_TRIES} windows per image, got {tries}")
    for i, p in enumerate(params):
        for (y0, x0, h, w) in win[i]:
            if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > p.resized[0] or x0 + w > p.resized[1]:
                raise ValueError(f"window_counts: window {(int(y0), int(x0), int(h), int(w))} of image {i} leaves the resized map {p.resized}")
    table = _rule(rule, params)
    dev = _device(sources, device, "window_counts")
    host = torch.empty((B, tries, K + 1), dtype=torch.int32, pin_memory=True)
    if B == 0:
        return host[:, :, :K]
    srcs, strides = _upload(sources, kind, dev)
    tables = [(table(p.src[1], p.resized[1]), table(p.src[0], p.resized[0])) for p in params]
    pinned, t0, n, w0 = _stage(srcs, strides, params, kind, tables, extra=win.astype(np.int32))
    staged = pinned.to(dev, non_blocking=True)
    counts = torch.empty((B, tries, K + 1), dtype=torch.int32, device=dev)
    _lib.call("mpf_label_window_counts", dev, pinned.data_ptr(), staged.data_ptr(), pinned.data_ptr() + 4 * t0, staged.data_ptr() + 4 * t0,
              n, pinned.data_ptr() + 4 * w0, staged.data_ptr() + 4 * w0, B, tries, K, int(ignore_label), counts.data_ptr(),
              _lib.stream_ptr(dev))
    with torch.cuda.device(dev):
        host.copy_(counts, non_blocking=True)
        torch.cuda.current_stream().synchronize()             # the one host wait
    stray = host[:, :, K]
    if int(stray.sum()) != 0:
        b, t = (int(v) for v in torch.nonzero(stray)[0])
        raise ValueError(f"window_counts: window {t} of image {b} holds {int(stray[b, t])} pixels whose label is neither in "
                         f"0 .. {K - 1} nor the ignore label {ignore_label}")
    return host[:, :, :K]


def _id_map(id_map, size, what):
    if not id_map.is_cuda:
        raise RuntimeError(f"{what}: Not implemented on the CPU (device tensors only)")
    if id_map.dim() != 2 or id_map.dtype != torch.int32:
        raise ValueError(f"{what}: id_map must be int32 [Hc, Wc], got {id_map.dtype} {tuple(id_map.shape)}")
    H, W = (int(size[0]), int(size[1])) if size is not None else tuple(id_map.shape)
    if H <= 0 or W <= 0 or H > id_map.shape[0] or W > id_map.shape[1] or H * W >= 1 << 31:
        raise ValueError(f"{what}: size {H} x {W} must be positive and lie inside the map {tuple(id_map.shape)}")
    if id_map.stride(1) != 1 or id_map.stride(0) < id_map.shape[1]:
        id_map = id_map.contiguous()
    return id_map, H, W


def label_bits(id_map, ids, size=None):
    """``id_map``: int32 [Hc, Wc] on the device (any row stride: a plane of ``resample_labels``' result or a view of it); ``ids``: T
    wanted ids (a host sequence or tensor); ``size`` (H, W): the top-left region the masks cover (default: the whole map) ->
    (bits int64 [T, nwords] in the layout of ``inference.pack_masks``, areas int32 [T]): row t is ``id_map[:H, :W] == ids[t]``.  The
    map is read once per launch of up to ``MAX_IDS`` ids (a longer list is split), never once per id.  An id that does not occur
    gives a zero row, equal ids give equal rows."""
    id_map, H, W = _id_map(id_map, size, "label_bits")
    ids = np.ascontiguousarray(np.asarray(ids.cpu() if torch.is_tensor(ids) else ids, dtype=np.int64).reshape(-1))
    if ids.size and (ids.min() < -(1 << 31) or ids.max() >= 1 << 31):
        raise ValueError("label_bits: ids must fit int32")
    ids = ids.astype(np.int32)
    T, dev = int(ids.size), id_map.device
    nwords = (H * W + 63) // 64
    bits = torch.empty((T, nwords), dtype=torch.int64, device=dev)
    areas = torch.empty(T, dtype=torch.int32, device=dev)
    for t0 in range(0, T, MAX_IDS):
        n = min(MAX_IDS, T - t0)
        _lib.call("mpf_label_bits", dev, id_map.data_ptr(), id_map.stride(0), H, W, ids[t0:].ctypes.data, n, bits[t0:].data_ptr(),
                  areas[t0:].data_ptr(), _lib.stream_ptr(dev))
    return bits, areas


def _label_targets(labels, bits, size):
    from .inference import mask_boxes
    dev = bits.device
    boxes = mask_boxes(bits, size).to(torch.float32) if bits.shape[0] else torch.zeros((0, 4), dtype=torch.float32, device=dev)
    t = _targets(labels, np.zeros((0, 4), dtype=np.float32), bits, size, dev)
    t["boxes"] = boxes                                       # BitMasks.get_bounding_boxes: float32 (x0, y0, x1 + 1, y1 + 1)
    return t


def panoptic_targets(id_map, segments_info, size=None):
    """The panoptic ground truth of one image from its id map: the non-crowd segments of ``segments_info`` in json order, empty ones
    kept (the reference keeps a segment the crop removed, with an all-zero mask and a zero box) -> {"labels" (the category ids),
    "bits", "masks" bool [T, H, W], "boxes" float32 [T, 4]}, also "areas" int32 [T]."""
    keep = [s for s in segments_info if not s.get("iscrowd", 0)]
    bits, areas = label_bits(id_map, [int(s["id"]) for s in keep], size)
    H, W = (int(size[0]), int(size[1])) if size is not None else tuple(id_map.shape)
    t = _label_targets([int(s["category_id"]) for s in keep], bits, (H, W))
    t["areas"] = areas
    return t


def semantic_targets(id_map, classes, size=None):
    """The semantic ground truth of one image: one mask per class of ``classes`` (ascending and without the ignore label where they
    come from ``window_counts``, as ``np.unique`` orders them) -> the dict of ``panoptic_targets`` with the classes as labels."""
    classes = [int(c) for c in classes]
    bits, areas = label_bits(id_map, classes, size)
    H, W = (int(size[0]), int(size[1])) if size is not None else tuple(id_map.shape)
    t = _label_targets(classes, bits, (H, W))
    t["areas"] = areas
    return t


def panoptic_lsj_batch(samples, dtype=torch.uint8, mean=None, std=None, canvas=None, pad_value=128, device=None):
    """B samples, each a dict with "image_raw" (uint8 [H, W, 3]), "pan_raw" (the panoptic PNG, uint8 [H, W, 3]), "lsj"
    (``LSJParams``) and "segments_info" -> (images [B, 3, Hc, Wc], a list of B target dicts as ``panoptic_targets`` gives, at the
    crop size).  One image launch, one label launch, one ``label_bits`` launch per image; no host wait."""
    samples = list(samples)
    params = [s["lsj"] for s in samples]
    images = resample_images([s["image_raw"] for s in samples], params, dtype=dtype, mean=mean, std=std, canvas=canvas,
                             pad_value=pad_value, device=device)
    maps = resample_labels([s["pan_raw"] for s in samples], params, "rgb", PANOPTIC_PAD_ID, canvas=tuple(images.shape[2:]),
                           device=images.device, rule="pil")
    return images, [panoptic_targets(m, s.get("segments_info", ()), p.crop) for m, s, p in zip(maps, samples, params)]


def semantic_batch(samples, num_classes, ignore_label, single_category_max_area=1.0, dtype=torch.uint8, mean=None, std=None,
                   pad_value=128, device=None):
    """B samples, each a dict with "image_raw" (uint8 [H, W, 3]), "sem_seg_raw" (uint8 or int32 [H, W]) and "semseg"
    (``augment.SemSegDraw``) -> (images [B, 3, Hc, Wc], a list of B target dicts).  The counts of every candidate window
    (``window_counts``, the one host wait), detectron2's category-area rule on the host, then one image launch (PIL bilinear, the
    flip applied to the crop), one label launch (torch's nearest rule, ``ignore_label`` as the pad) and one ``label_bits`` launch per
    image for the classes the chosen window holds.  Each target dict also has "sem_seg" int64 [Hc', Wc'] (the padded label map at
    the image's own canvas) and "params" (the ``SemSegParams`` chosen); masks and boxes are at that canvas, as the reference's."""
    samples = list(samples)
    draws = [s["semseg"] for s in samples]
    labels = [s["sem_seg_raw"] for s in samples]
    tries = {len(d.origins) for d in draws}
    if len(tries) > 1:
        raise ValueError(f"semantic_batch: every image needs the same number of candidate windows, got {sorted(tries)}")
    kind = "i32" if labels and labels[0].dtype == torch.int32 else "u8"
    dev = _device([s["image_raw"] for s in samples] + labels, device, "semantic_batch")
    if not samples:
        return resample_images([], [], dtype=dtype, mean=mean, std=std, device=dev), []
    labels = [l.to(dev, non_blocking=True) for l in labels]  # once: the counts and the resample both read them
    windows = [[(y0, x0, d.crop[0], d.crop[1]) for (y0, x0) in d.origins] for d in draws]
    counts = window_counts(labels, draws, windows, num_classes, ignore_label, kind=kind, device=dev, rule="torch").numpy()
    chosen = [choose_category_crop(c, len(d.origins), single_category_max_area) for c, d in zip(counts, draws)]
    params = [d.params(i) for d, i in zip(draws, chosen)]
    images = resample_images([s["image_raw"] for s in samples], params, dtype=dtype, mean=mean, std=std, pad_value=pad_value, device=dev)
    maps = resample_labels(labels, params, kind, int(ignore_label), canvas=tuple(images.shape[2:]), device=dev, rule="torch")
    targets = []
    for m, p, c, i in zip(maps, params, counts, chosen):
        classes = np.nonzero(c[i])[0]
        t = semantic_targets(m, classes, p.canvas)
        t["sem_seg"] = m[:p.canvas[0], :p.canvas[1]].to(torch.int64)
        t["counts"] = torch.from_numpy(c[i][classes].astype(np.int32))
        t["params"] = p
        targets.append(t)
    return images, targets
