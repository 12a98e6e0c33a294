"""CPU: the host half of the video training input without a GPU — the frame sampling and the draws of mp_former_amd.clip_input against
the restatement of the reference's mapper and augmentations (tests/_clip_restate.py) under seeded generators, PIL's nearest rule
for a binary mask against a golden recorded from PIL and against the installed PIL, the argument checks of mpf_mask_bits_resample
called without a device, and what the mapper refuses.

clip_mask_pil.npz: "sizes" int32 [N, 4] = (src_h, src_w, out_h, out_w); "src<i>" / "out<i>" = ``np.packbits`` of a random uint8 0/1
mask and of ``Image.fromarray(mask).resize((out_w, out_h), Image.NEAREST)`` (Pillow 12.2), the route detectron2's
``ResizeTransform.apply_segmentation`` takes for a decoded RLE.  The pair 14 x 2 -> 49 x 7 is one where PIL's accumulated
coordinate differs from ``(int)((x + 0.5) * in / out)``."""
import ctypes
import os
import random
import re
import types

import numpy as np
import pytest
import torch

import _clip_restate as CR
import _label_restate as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "clip_mask_pil.npz")
STYLES = ("range", "choice", "range_by_clip", "choice_by_clip")
FLIPS = ("none", "horizontal", "flip_by_clip")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib


# ---- the frame sampling -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffle", [False, True])
def test_sample_clip_frames_follows_the_mapper_on_seeded_generators(shuffle):
    from mp_former_amd import clip_input as CI
    repeats = 0
    for seed in range(60):
        length, num, rng = (3 + seed % 40, 2 + seed % 3, 1 + seed % 6)
        a = CI.sample_clip_frames(length, num, rng, shuffle, random.Random(seed), np.random.RandomState(seed))
        py, npr = random.Random(seed), np.random.RandomState(seed)
        b = CR.sample_frames(length, num, rng, shuffle, py, npr)
        assert a == b and len(a) == num and all(isinstance(i, int) and 0 <= i < length for i in a)
        assert max(a) - min(a) <= 2 * rng
        if not shuffle:
            assert a == sorted(a)
        repeats += len(set(a)) < len(a)
    assert repeats > 0                                       # np.random.choice draws WITH replacement: a frame can repeat


def test_sample_clip_frames_consumes_the_two_streams_in_the_mappers_order():
    from mp_former_amd import clip_input as CI
    py, npr, py2, np2 = random.Random(5), np.random.RandomState(5), random.Random(5), np.random.RandomState(5)
    CI.sample_clip_frames(30, 3, 4, True, py, npr)
    CR.sample_frames(30, 3, 4, True, py2, np2)
    assert py.random() == py2.random() and npr.randint(1 << 30) == np2.randint(1 << 30)
    assert CI.sample_clip_frames(1, 1, 5, False, random.Random(0), np.random.RandomState(0)) == [0]
    with pytest.raises(ValueError):                          # numpy's own error for an empty population
        CI.sample_clip_frames(1, 2, 5, False, random.Random(0), np.random.RandomState(0))


# ---- the draws --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", FLIPS)
@pytest.mark.parametrize("style", STYLES)
def test_draw_clip_follows_the_augmentations_on_a_seeded_random_state(style, flip):
    from mp_former_amd import augment as A
    from mp_former_amd import clip_input as CI
    h, w, F = 60, 83, 3
    edges = (40, 72) if "range" in style else (36, 48, 64, 80)
    differ = 0
    for seed in range(12):
        rng, ref = np.random.RandomState(seed), np.random.RandomState(seed)
        got = CI.draw_clip(h, w, F, edges, 100, style, flip, 32, rng=rng)
        want, log = CR.draw_clip(h, w, F, edges, 100, style, flip, ref)
        assert len(got) == F and all(isinstance(p, A.SemSegParams) for p in got)
        for p, (resized, do) in zip(got, want):
            assert p == A.SemSegParams((h, w), resized, (0, 0), resized, resized, do, tuple((v + 31) // 32 * 32 for v in resized))
        assert rng.randint(1 << 30) == ref.randint(1 << 30), "the two streams were consumed alike"
        # by_clip draws once per clip, the per-frame styles F times, the size before the flip
        n_size, n_flip = (1 if "by_clip" in style else F), {"none": 0, "horizontal": F, "flip_by_clip": 1}[flip]
        assert log.count("size") == n_size and log.count("flip") == n_flip
        if n_flip:
            assert log[:2] == ["size", "flip"]
        if "by_clip" in style:
            assert len({p.resized for p in got}) == 1
        if flip == "flip_by_clip":
            assert len({p.flip for p in got}) == 1
        differ += len({(p.resized, p.flip) for p in got}) > 1
    if "by_clip" not in style or flip == "horizontal":
        assert differ > 0                                    # the per-frame draws do differ between the frames of a clip


class _CountingRng:
    """a RandomState that logs the kind of every draw"""

    def __init__(self, seed):
        self.rs, self.log = np.random.RandomState(seed), []

    def randint(self, *a):
        self.log.append("size")
        return self.rs.randint(*a)

    def choice(self, a):
        self.log.append("size")
        return self.rs.choice(a)

    def uniform(self, *a):
        self.log.append("flip")
        return self.rs.uniform(*a)


def test_draw_clip_draw_counts_and_order():
    from mp_former_amd import clip_input as CI
    for style, flip, want in (("range", "horizontal", ["size", "flip"] * 4), ("choice", "flip_by_clip", ["size", "flip", "size", "size", "size"]),
                              ("range_by_clip", "horizontal", ["size", "flip", "flip", "flip", "flip"]),
                              ("choice_by_clip", "flip_by_clip", ["size", "flip"]), ("range_by_clip", "none", ["size"])):
        rng = _CountingRng(1)
        CI.draw_clip(48, 64, 4, (32, 40), 80, style, flip, 32, rng=rng)
        assert rng.log == want, (style, flip)


def test_draw_clip_refuses_what_is_not_built():
    from mp_former_amd import clip_input as CI
    with pytest.raises(ValueError, match="short edge of 0"):
        CI.draw_clip(48, 64, 2, (0, 0), 80, "range", "none", 32, rng=np.random.RandomState(0))
    with pytest.raises(ValueError, match="vertical"):
        CI.draw_clip(48, 64, 2, (32, 40), 80, "range", "vertical", 32)
    with pytest.raises(ValueError, match="sample_style"):
        CI.draw_clip(48, 64, 2, (32, 40), 80, "uniform", "none", 32)
    with pytest.raises(ValueError, match="random_flip"):
        CI.draw_clip(48, 64, 2, (32, 40), 80, "range", "both", 32)
    with pytest.raises(ValueError, match=r"\(min, max\)"):
        CI.draw_clip(48, 64, 2, (32, 40, 48), 80, "range_by_clip", "none", 32)
    p, = CI.draw_clip(48, 64, 1, 40, 80, "choice", "none", 0, rng=np.random.RandomState(0))      # an int edge, no divisibility
    assert p.resized == (40, 53) and p.canvas == (40, 53) and p.flip is False


# ---- PIL's nearest rule on a binary mask --------------------------------------------------------------------------------------------------
def _golden():
    z = np.load(GOLDEN)
    for i, (sh, sw, oh, ow) in enumerate(z["sizes"].tolist()):
        src = np.unpackbits(z[f"src{i}"])[:sh * sw].reshape(sh, sw).astype(bool)
        out = np.unpackbits(z[f"out{i}"])[:oh * ow].reshape(oh, ow).astype(bool)
        yield src, out


def test_mask_resize_equals_the_recorded_pil_masks():
    from mp_former_amd import augment as A
    n, differ = 0, 0
    for src, out in _golden():
        (sh, sw), (oh, ow) = src.shape, out.shape
        ty, tx = A.nearest_table_pil(sh, oh), A.nearest_table_pil(sw, ow)
        np.testing.assert_array_equal(src[ty][:, tx], out, err_msg=f"{src.shape} -> {out.shape}")
        np.testing.assert_array_equal(CR.resize_mask(src, out.shape, False), out)
        np.testing.assert_array_equal(CR.resize_mask(src, out.shape, True), out[:, ::-1])
        mult = lambda i, o: ((np.arange(o) + 0.5) * (i / o)).astype(np.int64)  # noqa: E731
        differ += int(not (np.array_equal(mult(sh, oh), ty) and np.array_equal(mult(sw, ow), tx)))
        n += 1
    assert n >= 4 and differ > 0                             # a pair where the accumulated rule is not the multiplied one is in


def test_mask_resize_equals_the_installed_pil():
    Image = pytest.importorskip("PIL.Image")
    from mp_former_amd import augment as A
    g = np.random.default_rng(8)
    for (sh, sw), (oh, ow) in (((37, 45), (53, 30)), ((14, 2), (49, 7)), ((64, 40), (33, 91)), ((360, 640), (288, 512))):
        m = (g.random((sh, sw)) < 0.4).astype(np.uint8)
        want = np.asarray(Image.fromarray(m).resize((ow, oh), Image.NEAREST)).astype(bool)
        np.testing.assert_array_equal(m.astype(bool)[A.nearest_table_pil(sh, oh)][:, A.nearest_table_pil(sw, ow)], want)
        np.testing.assert_array_equal(CR.resize_mask(m.astype(bool), (oh, ow), False), want)
    for src, out in _golden():                               # the golden is the installed PIL's too
        got = np.asarray(Image.fromarray(src.astype(np.uint8)).resize((out.shape[1], out.shape[0]), Image.NEAREST)).astype(bool)
        np.testing.assert_array_equal(got, out)


# ---- the entry --------------------------------------------------------------------------------------------------------------------------
def test_mask_bits_symbol_declared_exported_and_bound(built):
    from mp_former_amd import clip_input as CI
    src = open(os.path.join(ROOT, "include", "mpformer_hip.h")).read()
    assert "YTVISDatasetMapper" in src and "video_maskformer_model.py" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(built.LIB_PATH)
    assert re.search(r"\bmpf_mask_bits_resample\s*\(", code) and hasattr(raw, "mpf_mask_bits_resample")
    assert "mpf_mask_bits_resample" in built.SIGNATURES
    assert "clip_input.hip" in open(os.path.join(ROOT, "mp_former_amd", "csrc", "Makefile")).read()
    fields = re.search(r"typedef struct MpfMaskBitsRecord \{(.*?)\}", code, flags=re.S).group(1)
    assert len(re.findall(r"\b\w+\s*[,;]", fields.replace("const void* src;", ""))) == 8 and CI._REC_WORDS == 10
    assert built.lib().mpf_abi_version() == built.ABI_VERSION


def _record(**over):
    """a consistent host record for an 8 x 10 source resized to 6 x 12 at a fake pointer (never dereferenced), and its tables"""
    f = dict(src_lo=4096, src_hi=0, src_h=8, src_w=10, valid_h=6, valid_w=12, flip_out=0, xt_off=0, yt_off=12, dst=0)
    f.update(over)
    tab = np.concatenate([np.arange(12) * 10 // 12, np.arange(6) * 8 // 6]).astype(np.int32)
    return np.array(list(f.values()), dtype=np.int32), tab


def test_entry_rejects_bad_arguments_before_any_launch(built):
    lib = built.lib()
    one = ctypes.c_void_p(4096)      # never dereferenced: the checks come first
    err = lib.mpf_last_error

    def run(rec, tab, P=1, out=one, areas=one, Hc=8, Wc=16, recs_dev=one, tab_dev=one, tab_len=None):
        return lib.mpf_mask_bits_resample(rec.ctypes.data, recs_dev, tab.ctypes.data, tab_dev, len(tab) if tab_len is None else tab_len, P,
                                          out, areas, Hc, Wc, None)

    rec, tab = _record()
    assert run(rec, tab, P=0) == 0                           # nothing to do, nothing launched
    assert lib.mpf_mask_bits_resample(None, None, None, None, 0, 0, None, None, 8, 16, None) == 0
    for kw in (dict(out=None), dict(areas=None), dict(recs_dev=None), dict(tab_dev=None)):
        assert run(rec, tab, **kw) == -3 and b"NULL" in err(), kw
    assert lib.mpf_mask_bits_resample(None, one, tab.ctypes.data, one, len(tab), 1, one, one, 8, 16, None) == -3
    assert run(rec, tab, P=-1) == -2 and run(rec, tab, Hc=0) == -2 and run(rec, tab, Wc=0) == -2
    assert run(rec, tab, P=70000) == -4 and b"65535" in err()
    assert run(rec, tab, Hc=1 << 16, Wc=1 << 15) == -4 and b"2^31" in err()
    for over, code, what in ((dict(valid_h=7, yt_off=-1), -2, b"identity"),          # an identity record whose sizes differ
                             (dict(valid_w=11, xt_off=-1), -2, b"identity"),
                             (dict(src_w=9), -2, b"leaves the source"),              # a table entry out of range
                             (dict(src_h=6), -2, b"leaves the source"),
                             (dict(valid_h=9), -2, b"canvas smaller"),               # valid beyond the canvas
                             (dict(valid_w=17), -2, b"canvas smaller"),
                             (dict(yt_off=13), -2, b"outside the table"), (dict(xt_off=-2), -2, b"outside the table"),
                             (dict(flip_out=2), -2, b"flip_out"), (dict(src_h=0), -2, b"positive"), (dict(valid_w=0), -2, b"positive"),
                             (dict(dst=1), -2, b"dst"), (dict(dst=-1), -2, b"dst"), (dict(src_lo=4100), -2, b"aligned"),
                             (dict(src_h=1 << 16, src_w=1 << 15), -4, b"2^31")):
        bad, _ = _record(**over)
        assert run(bad, tab) == code and what in err(), over
    neg = tab.copy()
    neg[3] = -1
    assert run(rec, neg) == -2 and b"leaves the source" in err()
    assert run(rec, tab, tab_len=len(tab) - 1) == -2 and b"outside the table" in err()
    two = np.concatenate([_record()[0], _record()[0]])                               # the same dst twice
    assert run(two, tab, P=2) == -2 and b"dst" in err()
    # an identity record of equal sizes and an empty plane (NULL src: nothing else is read) pass the checks up to the launch, which
    # is not made here; so only their rejection by a later, bad record is seen
    ok_then_bad = np.concatenate([_record(src_h=6, src_w=12, xt_off=-1, yt_off=-1, dst=1)[0], _record(src_lo=0, valid_h=99, dst=2)[0],
                                  _record(valid_h=9)[0]])
    assert run(ok_then_bad, tab, P=3) == -2 and b"canvas smaller" in err()


# ---- the host layer and the mapper --------------------------------------------------------------------------------------------------------
def test_cpu_devices_raise():
    from mp_former_amd import clip_input as CI
    p, = CI.draw_clip(8, 10, 1, 8, 20, "choice", "none", 1, rng=np.random.RandomState(0))
    msg = r"Not implemented on the CPU \(device tensors only\)"
    with pytest.raises(RuntimeError, match=msg):
        CI.resample_mask_bits([(torch.zeros(2, dtype=torch.int64), (8, 10), p)], (8, 10), device="cpu")
    with pytest.raises(RuntimeError, match=msg):
        CI.clip_targets([[]], (p,), 40, device="cpu")
    sample = {"image_raw": [torch.zeros(8, 10, 3, dtype=torch.uint8)], "clip": (p,), "annotations": [[]], "num_classes": 40}
    with pytest.raises(RuntimeError, match=msg):
        CI.clip_batch([sample], device="cpu")
    with pytest.raises(ValueError, match="frames but"):
        CI.clip_batch([dict(sample, clip=(p, p))], device="cpu")
    with pytest.raises(ValueError, match="smaller than the size"):
        CI.resample_mask_bits([(torch.zeros(2, dtype=torch.int64), (8, 10), p)], (7, 10), device="cpu")


def _mapper_kwargs(**over):
    kw = dict(min_size=(32, 40), max_size=80, sampling="choice_by_clip", random_flip="flip_by_clip", image_format="RGB",
              sampling_frame_num=2, sampling_frame_range=3, sampling_frame_shuffle=False, num_classes=40, size_divisibility=32)
    kw.update(over)
    return kw


def test_the_mapper_refuses_what_is_not_built_naming_the_key():
    from mp_former_amd import d2_plugin as P
    with pytest.raises(NotImplementedError, match="INPUT.CROP.ENABLED"):
        P.YTVISClipDeviceMapper(True, **_mapper_kwargs(crop_enabled=True))
    for name in ("brightness", "contrast", "saturation", "rotation"):
        with pytest.raises(NotImplementedError, match=f"INPUT.AUGMENTATIONS '{name}'"):
            P.YTVISClipDeviceMapper(True, **_mapper_kwargs(augmentations=[name]))
    with pytest.raises(ValueError, match="only training"):
        P.YTVISClipDeviceMapper(False, **_mapper_kwargs())
    with pytest.raises(ValueError, match="vertical"):
        P.YTVISClipDeviceMapper(True, **_mapper_kwargs(random_flip="vertical"))
    with pytest.raises(ValueError, match="sampling"):
        P.YTVISClipDeviceMapper(True, **_mapper_kwargs(sampling="uniform"))


def _cfg(**inp):
    ns = types.SimpleNamespace
    base = dict(MIN_SIZE_TRAIN=(32, 40), MAX_SIZE_TRAIN=80, MIN_SIZE_TRAIN_SAMPLING="range_by_clip", RANDOM_FLIP="flip_by_clip", FORMAT="RGB",
                SAMPLING_FRAME_NUM=3, SAMPLING_FRAME_RANGE=2, SAMPLING_FRAME_SHUFFLE=False, CROP=ns(ENABLED=False), AUGMENTATIONS=[])
    base.update(inp)
    return ns(INPUT=ns(**base), MODEL=ns(MASK_ON=True, SEM_SEG_HEAD=ns(NUM_CLASSES=40), MASK_FORMER=ns(SIZE_DIVISIBILITY=32)))


def test_the_mapper_samples_reads_and_draws_without_resizing():
    from mp_former_amd import augment as A
    from mp_former_amd import d2_plugin as P
    with pytest.raises(NotImplementedError, match="INPUT.AUGMENTATIONS 'rotation'"):
        P.YTVISClipDeviceMapper(_cfg(AUGMENTATIONS=["rotation"]), True)
    with pytest.raises(NotImplementedError, match="INPUT.CROP.ENABLED"):
        P.YTVISClipDeviceMapper(_cfg(CROP=types.SimpleNamespace(ENABLED=True)), True)
    mapper = P.YTVISClipDeviceMapper(_cfg(), True)
    g = np.random.default_rng(4)
    stills = {f"v/{i:05d}.jpg": g.integers(0, 256, size=(48, 64, 3), dtype=np.uint8) for i in range(9)}
    reads = []
    mapper.read_image = lambda name, format=None: reads.append((name, format)) or stills[name]
    rle = {"size": [48, 64], "counts": [100, 20, 48 * 64 - 120]}
    annos = [[{"id": 4, "category_id": 2, "iscrowd": 0, "segmentation": rle, "keypoints": [1]},
              {"id": 5, "category_id": 3, "iscrowd": 1, "segmentation": rle}] for _ in range(9)]
    video = {"length": 9, "file_names": sorted(stills), "annotations": annos, "height": 48, "width": 64, "video_id": 77}
    random.seed(3)
    np.random.seed(3)
    d = mapper(video)
    random.seed(3)
    np.random.seed(3)
    selected = CR.sample_frames(9, 3, 2, False, random, np.random)
    geometry, _ = CR.draw_clip(48, 64, 3, (32, 40), 80, "range_by_clip", "flip_by_clip", np.random)
    assert d["file_names"] == [video["file_names"][i] for i in selected] and [r[0] for r in reads] == d["file_names"]
    assert all(r[1] == "RGB" for r in reads) and d["video_id"] == 77 and d["num_classes"] == 40 and d["length"] == 9
    assert len(d["image_raw"]) == 3 and all(im.dtype == torch.uint8 and tuple(im.shape) == (48, 64, 3) for im in d["image_raw"])
    assert all(np.array_equal(im.numpy(), stills[n]) for im, n in zip(d["image_raw"], d["file_names"]))     # no resize on the worker
    assert [(p.resized, p.flip) for p in d["clip"]] == geometry and all(isinstance(p, A.SemSegParams) for p in d["clip"])
    assert all(p.canvas == tuple((v + 31) // 32 * 32 for v in p.resized) for p in d["clip"])
    assert len(d["annotations"]) == 3
    for frame in d["annotations"]:                           # the non-crowd annotations as the json holds them: no decode
        assert [a["id"] for a in frame] == [4] and frame[0]["segmentation"] is rle and "keypoints" not in frame[0]
    assert video["annotations"][0][0]["keypoints"] == [1]    # the dataset's dict is not modified
    with pytest.raises(ValueError, match="the dataset says"):
        mapper(dict(video, height=50))
