"""A numpy restatement of the reference's video training mapper (mask2former_video/data_video/dataset_mapper.py:176-269, the
augmentations of data_video/augmentation.py) and of ``VideoMaskFormer.prepare_targets`` (video_maskformer_model.py:227-253), written
from the rules alone and independent of mp_former_amd.clip_input: the frame sampling, the draws in their order, per instance and
frame ``decode -> PIL nearest resize -> flip`` (or polygons through the two transforms' ``apply_coords`` and ``polygons_to_bitmask``),
the ``set`` ordering of the tubes, the dummy rows, ``filter_empty_instances``' -1 ids, ``get_bounding_boxes`` and the padded copy."""
import numpy as np
import torch

import _codec_restate as C
import _label_restate as L
import _resample_restate as R


# ---- the draws --------------------------------------------------------------------------------------------------------------------------
def sample_frames(length, num, frame_range, shuffle, py_rng, np_rng):
    """dataset_mapper.py:187-201"""
    ref_frame = py_rng.randrange(length)
    start_idx = max(0, ref_frame - frame_range)
    end_idx = min(length, ref_frame + frame_range + 1)
    selected_idx = np_rng.choice(np.array(list(range(start_idx, ref_frame)) + list(range(ref_frame + 1, end_idx))), num - 1)
    selected_idx = sorted(selected_idx.tolist() + [ref_frame])
    if shuffle:
        py_rng.shuffle(selected_idx)
    return selected_idx


class _ResizeShortestEdge:
    """augmentation.py:17-73 without the transform object: the counter, the draw every ``clip_frame_cnt`` frames"""

    def __init__(self, short_edge_length, max_size, sample_style, clip_frame_cnt, rng, log):
        self.is_range = "range" in sample_style
        self.short_edge_length, self.max_size, self.clip_frame_cnt, self.rng, self.log, self._cnt = short_edge_length, max_size, clip_frame_cnt, rng, log, 0

    def get(self, h, w):
        if self._cnt % self.clip_frame_cnt == 0:
            if self.is_range:
                self.size = self.rng.randint(self.short_edge_length[0], self.short_edge_length[1] + 1)
            else:
                self.size = self.rng.choice(self.short_edge_length)
            self.log.append("size")
            assert self.size != 0
            self._cnt = 0
        self._cnt += 1
        return R.shortest_edge_size(h, w, self.size, self.max_size)


class _RandomFlip:
    """augmentation.py:76-112"""

    def __init__(self, clip_frame_cnt, rng, log):
        self.clip_frame_cnt, self.rng, self.log, self._cnt = clip_frame_cnt, rng, log, 0

    def get(self):
        if self._cnt % self.clip_frame_cnt == 0:
            self.do = bool(self.rng.uniform(0, 1.0) < 0.5)
            self.log.append("flip")
            self._cnt = 0
        self._cnt += 1
        return self.do


def draw_clip(h, w, num_frames, short_edge_length, max_size, sample_style, random_flip, rng):
    """build_augmentation + AugmentationList applied frame by frame -> ([(resized, flip)] per frame, the log of the draws)"""
    log = []
    resize = _ResizeShortestEdge(short_edge_length, max_size, sample_style, num_frames if "by_clip" in sample_style else 1, rng, log)
    flip = None if random_flip == "none" else _RandomFlip(num_frames if random_flip == "flip_by_clip" else 1, rng, log)
    out = []
    for _ in range(num_frames):
        resized = resize.get(h, w)                           # the augmentations run in list order on every frame
        out.append((resized, flip.get() if flip is not None else False))
    return out, log


# ---- one mask ---------------------------------------------------------------------------------------------------------------------------
def resize_mask(mask, resized, flip):
    """ResizeTransform.apply_segmentation on a uint8 mask (PIL NEAREST), then HFlipTransform's -> bool [h', w']"""
    m = L.resize_nearest(np.asarray(mask), resized[0], resized[1], "pil")
    return m[:, ::-1] if flip else m


def frame_mask(segm, src, resized, flip):
    """transform_instance_annotations + annotations_to_instances(mask_format="bitmask") for one annotation of one frame"""
    if isinstance(segm, dict):
        return resize_mask(C.segm_mask(segm, src[0], src[1]), resized, flip)
    rings = []
    for ring in segm:                                        # apply_coords of the resize, then of the flip, in float64
        a = np.asarray(ring, dtype=np.float64).reshape(-1, 2).copy()
        a[:, 0] = a[:, 0] * (resized[1] * 1.0 / src[1])
        a[:, 1] = a[:, 1] * (resized[0] * 1.0 / src[0])
        if flip:
            a[:, 0] = resized[1] - a[:, 0]
        rings.append(a.reshape(-1))
    return C.poly_mask(rings, resized[0], resized[1])


def pad_to(plane, canvas):
    out = np.zeros(canvas, dtype=bool)
    out[:plane.shape[0], :plane.shape[1]] = plane
    return out


# ---- the mapper's target half -----------------------------------------------------------------------------------------------------------
def clip_instances(frame_annotations, src, geometry, num_classes):
    """dataset_mapper.py:208-267 for the sampled frames -> per frame (gt_classes int64 [G], gt_ids int64 [G], masks bool [G, h', w'],
    boxes float32 [G, 4])"""
    _ids = set()
    for annos in frame_annotations:
        _ids.update([anno["id"] for anno in annos])
    ids = dict()
    for i, _id in enumerate(_ids):
        ids[_id] = i
    frames = []
    for annos, (resized, flip) in zip(frame_annotations, geometry):
        G = len(ids)
        classes = np.full(G, num_classes, dtype=np.int64)    # _get_dummy_anno: class num_classes, id -1, an all-zero polygon
        gt_ids = np.full(G, -1, dtype=np.int64)
        masks = np.zeros((G,) + tuple(resized), dtype=bool)
        for a in annos:
            if a.get("iscrowd", 0) != 0:
                continue
            g = ids[a["id"]]
            classes[g], gt_ids[g] = a["category_id"], a["id"]
            masks[g] = frame_mask(a["segmentation"], src, resized, flip)
        boxes = L.boxes(masks)
        nonempty = (boxes[:, 2] - boxes[:, 0] > 1e-5) & (boxes[:, 3] - boxes[:, 1] > 1e-5) & masks.reshape(G, -1).any(axis=1)
        gt_ids[~nonempty] = -1                               # filter_empty_instances
        frames.append((classes, gt_ids, masks, boxes))
    return frames


def prepare_targets(frames, canvas):
    """video_maskformer_model.py:227-253 -> labels [G'], ids [G', F], masks bool [G', F, Hc, Wc] (torch)"""
    G, F = len(frames[0][0]), len(frames)
    masks = np.zeros((G, F) + tuple(canvas), dtype=bool)
    for f, (_, _, m, _) in enumerate(frames):
        masks[:, f, :m.shape[1], :m.shape[2]] = m
    ids = np.stack([fr[1] for fr in frames], axis=1) if G else np.zeros((0, F), dtype=np.int64)
    valid = (ids != -1).any(axis=1)
    labels = frames[-1][0]                                   # the LAST frame's classes
    return {"labels": torch.from_numpy(labels[valid]), "ids": torch.from_numpy(ids[valid]), "masks": torch.from_numpy(masks[valid])}


def clip_frames(images, geometry, canvas, mean=None, std=None):
    """the frames: PIL bilinear resize, flip of the result, then (normalised, as the model does, and) zero-padded to the canvas ->
    uint8 or float32 [F, 3, Hc, Wc]"""
    out = []
    for img, (resized, flip) in zip(images, geometry):
        full = R.resize(img, resized[0], resized[1])
        if flip:
            full = full[:, ::-1]
        chw = torch.from_numpy(np.ascontiguousarray(full.transpose(2, 0, 1)))
        if mean is not None:
            chw = (chw - torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)) / torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
        pad = torch.zeros((3,) + tuple(canvas), dtype=chw.dtype)
        pad[:, :chw.shape[1], :chw.shape[2]] = chw
        out.append(pad)
    return torch.stack(out)
