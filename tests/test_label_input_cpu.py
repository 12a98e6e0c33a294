"""CPU: the host half of the label-map input path without a GPU — the two nearest-neighbour rules of mp_former_amd.augment against PIL
(live where it imports, and against tables recorded from it in tests/golden/label_nearest.npz) and against torch's float64
``F.interpolate``, detectron2's category-area crop rule against its ``np.unique`` restatement (tests/_label_restate.py), the draws
against a seeded RandomState, the argument checks of the three C entries called without a device, and what is out of scope.

label_nearest.npz: "pairs" int32 [N, 2] = (in, out) for every pair of 1 .. 40 and 3000 -> 333, 3001; "tables" int16 = the source
index PIL's ``Image.resize((out, 1), NEAREST)`` read for each output of an ``arange(in)`` row, concatenated in that order."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _label_restate as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "label_nearest.npz")
PAIRS = [(i, o) for i in range(1, 41) for o in range(1, 41)] + [(3000, 333), (3000, 3001)]
NEW_SYMBOLS = ("mpf_label_resample", "mpf_label_window_counts", "mpf_label_bits", "mpf_label_counts_max_classes",
               "mpf_label_counts_max_tries", "mpf_label_bits_max_ids")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib


# ---- the nearest rules ----------------------------------------------------------------------------------------------------------------
def test_nearest_table_pil_equals_the_recorded_pil_tables():
    from mp_former_amd import augment as A
    z = np.load(GOLDEN)
    assert [tuple(p) for p in z["pairs"].tolist()] == PAIRS
    tables, at = z["tables"], 0
    for i, o in PAIRS:
        want = tables[at:at + o].astype(np.int32)
        at += o
        got = A.nearest_table_pil(i, o)
        assert got.dtype == np.int32 and got.shape == (o,)
        np.testing.assert_array_equal(got, want, err_msg=f"{i} -> {o}")
        np.testing.assert_array_equal(L.nearest_pil(i, o), want, err_msg=f"restatement {i} -> {o}")
    assert at == len(tables)


def _pil_table(Image, i, o):
    """PIL's own choice per output: resize an int32 arange row (mode I) with NEAREST"""
    row = np.arange(i, dtype=np.int32)[None, :]
    return np.asarray(Image.fromarray(row).resize((o, 1), Image.NEAREST))[0]


def test_nearest_table_pil_equals_the_installed_pil():
    Image = pytest.importorskip("PIL.Image")
    from mp_former_amd import augment as A
    for i, o in PAIRS:
        np.testing.assert_array_equal(A.nearest_table_pil(i, o), _pil_table(Image, i, o), err_msg=f"{i} -> {o}")
    # the route the panoptic PNG takes: a uint8 RGB image, both axes at once
    g = np.random.default_rng(5)
    src = g.integers(0, 256, size=(37, 53, 3), dtype=np.uint8)
    for oh, ow in ((64, 19), (11, 200), (37, 53)):
        want = np.asarray(Image.fromarray(src).resize((ow, oh), Image.NEAREST))
        np.testing.assert_array_equal(src[A.nearest_table_pil(37, oh)][:, A.nearest_table_pil(53, ow)], want)
        np.testing.assert_array_equal(L.resize_nearest(src, oh, ow, "pil"), want)


def test_the_multiplied_form_is_not_pils_rule():
    """why the table accumulates: (int)((x + 0.5) * in / out) differs from the recorded PIL tables somewhere in the sweep"""
    z = np.load(GOLDEN)
    tables, at, differ = z["tables"], 0, 0
    for i, o in PAIRS:
        mult = ((np.arange(o) + 0.5) * (i / o)).astype(np.int64)
        differ += int(not np.array_equal(mult, tables[at:at + o]))
        at += o
    assert differ > 0


def test_nearest_table_torch_equals_interpolate_on_float64_maps():
    from mp_former_amd import augment as A
    g = np.random.default_rng(11)
    for _ in range(60):
        h, w, oh, ow = (int(v) for v in g.integers(1, 120, size=4))
        src = g.integers(0, 1000, size=(h, w)).astype(np.float64)
        want = torch.nn.functional.interpolate(torch.from_numpy(src)[None, None], size=(oh, ow), mode="nearest")[0, 0].numpy()
        ty, tx = A.nearest_table_torch(h, oh), A.nearest_table_torch(w, ow)
        assert ty.dtype == np.int32 and ty.shape == (oh,) and tx.shape == (ow,)
        np.testing.assert_array_equal(src[ty][:, tx], want)
        np.testing.assert_array_equal(L.resize_nearest(src, oh, ow, "torch"), want)
    for i, o in ((3000, 333), (3000, 3001), (512, 683), (7, 1)):
        np.testing.assert_array_equal(A.nearest_table_torch(i, o), L.nearest_torch(i, o))


def test_nearest_tables_reject_bad_sizes():
    from mp_former_amd import augment as A
    for f in (A.nearest_table_pil, A.nearest_table_torch):
        with pytest.raises(ValueError, match="positive"):
            f(0, 4)
        with pytest.raises(ValueError, match="positive"):
            f(4, 0)


# ---- the crop rule ------------------------------------------------------------------------------------------------------------------
def _counts(window, K, ignore):
    c = np.zeros(K, dtype=np.int64)
    labels, cnt = np.unique(window, return_counts=True)
    for l, n in zip(labels, cnt):
        if l != ignore:
            c[int(l)] = n
    return c


def _crop_case(maps, max_area, K=5, ignore=255):
    """the windows are whole maps of one size, one per try: the rule from counts equals the rule from np.unique"""
    from mp_former_amd import augment as A
    h, w = maps[0].shape
    stacked = np.concatenate(maps, axis=0)
    origins = [(i * h, 0) for i in range(len(maps))]
    want = L.category_crop(stacked, origins, (h, w), ignore, max_area)
    counts = np.stack([_counts(m, K, ignore) for m in maps])
    got = A.choose_category_crop(counts, len(maps), max_area)
    assert got == want == L.choose_from_counts(counts, max_area)
    return got


def test_choose_category_crop_equals_the_np_unique_rule():
    one = np.full((4, 5), 2)                                 # one label only: len(cnt) == 1
    ign = np.full((4, 5), 255)                               # ignore only: len(cnt) == 0
    at = np.zeros((4, 5), dtype=np.int64)                    # exactly at the threshold: 15 of 20 with max_area 0.75 -> 15 < 15 fails
    at[0] = 1
    below = at.copy()                                        # 14 of 20: passes
    below[1, 0] = 3
    mixed_ign = at.copy()                                    # the ignored pixels leave the sum: 15 of 15 + ... -> 10 of 15
    mixed_ign[3] = 255
    assert _crop_case([one, ign, at, below], 0.75) == 3
    assert _crop_case([one, ign, at], 0.75) == 2             # none passes: the last try
    assert _crop_case([below, one], 0.75) == 0
    assert _crop_case([at, mixed_ign, below], 0.75) == 1     # 10 < 15 * 0.75 = 11.25
    assert _crop_case([one, below], 1.0) == 0                # max_area >= 1: one draw, no test
    assert _crop_case([one, below], 1.5) == 0
    g = np.random.default_rng(3)
    for _ in range(200):
        maps = [g.choice([0, 1, 2, 3, 4, 255], size=(3, 4), p=g.dirichlet(np.ones(6) * 0.3)) for _ in range(10)]
        _crop_case(maps, float(g.choice([0.5, 0.75, 0.9, 1.0])))


def test_choose_category_crop_rejects_bad_counts():
    from mp_former_amd import augment as A
    with pytest.raises(ValueError, match="tries"):
        A.choose_category_crop(np.zeros((2, 3)), 3, 0.5)
    with pytest.raises(ValueError, match="tries"):
        A.choose_category_crop(np.zeros(3), 1, 0.5)


# ---- the draws --------------------------------------------------------------------------------------------------------------------------
def test_draws_follow_detectron2_on_a_seeded_random_state():
    from mp_former_amd import augment as A
    import _resample_restate as R
    h, w = 60, 83
    # ResizeShortestEdge "range", then ten (y, x) origins, then the flip
    rng, ref = np.random.RandomState(7), np.random.RandomState(7)
    d = A.draw_semseg(h, w, (40, 90), 120, "range", crop=(32, 48), single_category_max_area=0.75, size_divisibility=64, rng=rng)
    size = ref.randint(40, 91)
    rh, rw = R.shortest_edge_size(h, w, size, 120)
    ch, cw = min(32, rh), min(48, rw)
    origins = tuple((int(ref.randint(rh - ch + 1)), int(ref.randint(rw - cw + 1))) for _ in range(10))
    flip = bool(ref.uniform() < 0.5)
    assert d == A.SemSegDraw((h, w), (rh, rw), (ch, cw), origins, flip, (64, 64))
    assert rng.randint(1 << 30) == ref.randint(1 << 30), "the two streams were consumed alike"
    p = d.params(4)
    assert p == A.SemSegParams((h, w), (rh, rw), origins[4], (ch, cw), (ch, cw), flip, (64, 64))
    # "choice", the rule off: one origin; no crop: the whole image, no origin drawn
    rng, ref = np.random.RandomState(9), np.random.RandomState(9)
    d = A.draw_semseg(h, w, (30, 50, 70), 100, "choice", crop=(32, 32), single_category_max_area=1.0, rng=rng)
    rh, rw = R.shortest_edge_size(h, w, int(ref.choice([30, 50, 70])), 100)
    ch, cw = min(32, rh), min(32, rw)
    origins = ((int(ref.randint(rh - ch + 1)), int(ref.randint(rw - cw + 1))),)
    assert d == A.SemSegDraw((h, w), (rh, rw), (ch, cw), origins, bool(ref.uniform() < 0.5), (ch, cw))
    rng, ref = np.random.RandomState(2), np.random.RandomState(2)
    d = A.draw_semseg(h, w, (50, 50), 100, "range", crop=None, flip=False, rng=rng)
    rh, rw = R.shortest_edge_size(h, w, int(ref.randint(50, 51)), 100)
    assert d == A.SemSegDraw((h, w), (rh, rw), (rh, rw), ((0, 0),), False, (rh, rw))
    assert A.draw_shortest_edge(h, w, (0, 0), 100, "range", np.random.RandomState(0)) == (h, w)
    assert A.crop_size_absolute((512, 512), (300, 700)) == (300, 512)
    with pytest.raises(ValueError, match="sample_style"):
        A.draw_shortest_edge(h, w, (40, 50), 100, "uniform")


# ---- out of scope ---------------------------------------------------------------------------------------------------------------------
def _semantic_kwargs(**over):
    kw = dict(min_size=(40, 60), max_size=120, sampling="choice", crop_enabled=True, crop_type="absolute", crop_size=(32, 32),
              single_category_max_area=1.0, color_aug_ssd=False, image_format="RGB", ignore_label=255, size_divisibility=32, num_classes=5)
    kw.update(over)
    return kw


def test_what_is_out_of_scope_raises_naming_itself():
    from mp_former_amd import augment as A
    from mp_former_amd import d2_plugin as P
    for t in ("relative", "relative_range", "absolute_range"):
        with pytest.raises(NotImplementedError, match=t):
            A.crop_size(t, (0.5, 0.5), (100, 100))
        with pytest.raises(NotImplementedError, match=t):
            P.SemanticDeviceMapper(True, **_semantic_kwargs(crop_type=t))
    with pytest.raises(NotImplementedError, match="COLOR_AUG_SSD"):
        P.SemanticDeviceMapper(True, **_semantic_kwargs(color_aug_ssd=True))
    with pytest.raises(NotImplementedError, match="MaskFormerPanopticDatasetMapper"):
        P.MaskFormerPanopticDeviceMapper()
    with pytest.raises(NotImplementedError, match="vertical"):
        P.COCOPanopticLSJDeviceMapper(True, image_size=32, min_scale=0.5, max_scale=2.0, random_flip="vertical", image_format="RGB")
    P.SemanticDeviceMapper(True, **_semantic_kwargs())       # the supported configuration builds


def test_cpu_devices_raise():
    from mp_former_amd import augment as A
    from mp_former_amd import label_input as LI
    lab = torch.zeros(8, 10, dtype=torch.uint8)
    p = A.SemSegParams((8, 10), (8, 10), (0, 0), (8, 10), (8, 10), False, (8, 10))
    msg = r"Not implemented on the CPU \(device tensors only\)"
    with pytest.raises(RuntimeError, match=msg):
        LI.resample_labels([lab], [p], "u8", 255, device="cpu")
    with pytest.raises(RuntimeError, match=msg):
        LI.window_counts([lab], [p], [[(0, 0, 8, 10)]], 5, 255, device="cpu")
    with pytest.raises(RuntimeError, match=msg):
        LI.label_bits(torch.zeros(8, 10, dtype=torch.int32), [1, 2])
    with pytest.raises(RuntimeError, match=msg):
        LI.panoptic_targets(torch.zeros(8, 10, dtype=torch.int32), [])
    with pytest.raises(ValueError, match="one kind per batch"):
        LI.resample_labels([lab, lab.to(torch.int32)], [p, p], "u8", 255, device="cpu")
    with pytest.raises(ValueError, match="parameters say"):
        LI.resample_labels([torch.zeros(9, 10, dtype=torch.uint8)], [p], "u8", 255, device="cpu")
    with pytest.raises(ValueError, match="leaves the resized map"):
        LI.window_counts([lab], [p], [[(0, 0, 9, 10)]], 5, 255, device="cpu")
    with pytest.raises(ValueError, match="num_classes"):
        LI.window_counts([lab], [p], [[(0, 0, 8, 10)]], 5000, 255, device="cpu")


# ---- the entries ------------------------------------------------------------------------------------------------------------------------
def test_label_symbols_declared_exported_and_bound(built):
    from mp_former_amd import label_input as LI
    src = open(os.path.join(ROOT, "include", "mpformer_hip.h")).read()
    assert "coco_panoptic_new_baseline_dataset_mapper.py" in src and "mask_former_semantic_dataset_mapper.py" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(raw, name) and name in built.SIGNATURES, name
    assert "label_input.hip" in open(os.path.join(ROOT, "mp_former_amd", "csrc", "Makefile")).read()
    lib = built.lib()
    assert lib.mpf_label_counts_max_classes() == LI.MAX_CLASSES >= 847
    assert lib.mpf_label_counts_max_tries() == LI.MAX_TRIES >= 10
    assert lib.mpf_label_bits_max_ids() == LI.MAX_IDS
    fields = re.search(r"typedef struct MpfLabelRecord \{(.*?)\}", code, flags=re.S).group(1)
    assert len(re.findall(r"\b\w+\s*[,;]", fields.replace("const void* src;", ""))) == 16 and LI._REC_WORDS == 18


def _record(**over):
    """a consistent host record + identity tables for an 8 x 10 uint8 map at a fake pointer (never dereferenced)"""
    f = dict(src_lo=4096, src_hi=0, src_stride=10, src_h=8, src_w=10, kind=0, flip_in=0, flip_out=0, out_h=8, out_w=10, off_y=0, off_x=0,
             crop_h=8, crop_w=10, valid_h=8, valid_w=10, xt_off=0, yt_off=10)
    f.update(over)
    tab = np.concatenate([np.arange(10), np.arange(8)]).astype(np.int32)
    return np.array(list(f.values()), dtype=np.int32), tab


def test_entries_reject_bad_arguments_before_any_launch(built):
    lib = built.lib()
    one = ctypes.c_void_p(4096)      # never dereferenced: the checks come first
    err = lib.mpf_last_error

    def resample(rec, tab, B=1, out=one, Hc=8, Wc=10, recs_dev=one, tab_dev=one, tab_len=None):
        return lib.mpf_label_resample(rec.ctypes.data, recs_dev, tab.ctypes.data, tab_dev, len(tab) if tab_len is None else tab_len, B, out,
                                      Hc, Wc, 255, None)

    rec, tab = _record()
    assert resample(rec, tab, B=0) == 0
    assert resample(rec, tab, out=None) == -3 and resample(rec, tab, recs_dev=None) == -3 and resample(rec, tab, tab_dev=None) == -3
    assert resample(rec, tab, B=-1) == -2 and resample(rec, tab, Hc=0) == -2
    assert resample(rec, tab, Hc=7) == -2 and b"canvas smaller" in err()
    assert resample(rec, tab, B=70000) == -4
    assert resample(rec, tab, Hc=1 << 16, Wc=1 << 15) == -4
    for over, code, what in ((dict(src_lo=0), -3, b"NULL"), (dict(kind=3), -1, b"kind"), (dict(src_stride=9), -2, b"stride"),
                             (dict(kind=1, src_stride=42), -2, b"multiple of 4"), (dict(kind=2, src_stride=29), -2, b"stride"),
                             (dict(flip_out=2), -2, b"flip"), (dict(valid_h=9), -2, b"valid extent"), (dict(off_x=1), -2, b"valid extent"),
                             (dict(src_w=9), -2, b"leaves the source"), (dict(src_h=7), -2, b"leaves the source"),
                             (dict(yt_off=11), -2, b"outside the table"), (dict(xt_off=-1), -2, b"outside the table"),
                             (dict(src_stride=1 << 28), -4, b"2^31")):
        bad, _ = _record(**over)
        assert resample(bad, tab) == code and what in err(), over
    neg = tab.copy()
    neg[3] = -1
    assert resample(rec, neg) == -2 and b"leaves the source" in err()
    assert resample(rec, tab, tab_len=len(tab) - 1) == -2 and b"outside the table" in err()

    def counts(rec, tab, win, B=1, tries=1, K=5, out=one, win_dev=one):
        win = np.asarray(win, dtype=np.int32)
        return lib.mpf_label_window_counts(rec.ctypes.data, one, tab.ctypes.data, one, len(tab), win.ctypes.data, win_dev, B, tries, K, 255,
                                           out, None)

    assert counts(rec, tab, [0, 0, 8, 10], B=0) == 0
    assert counts(rec, tab, [0, 0, 8, 10], out=None) == -3 and counts(rec, tab, [0, 0, 8, 10], win_dev=None) == -3
    assert counts(rec, tab, [0, 0, 8, 10], tries=0) == -2 and counts(rec, tab, [0, 0, 8, 10], tries=17) == -2 and b"tries" in err()
    assert counts(rec, tab, [0, 0, 8, 10], K=0) == -2 and counts(rec, tab, [0, 0, 8, 10], K=1025) == -2 and b"classes" in err()
    for win in ([0, 0, 9, 10], [1, 0, 8, 10], [0, 1, 8, 10], [-1, 0, 2, 2], [0, 0, 0, 3]):
        assert counts(rec, tab, win) == -2 and b"inside the resized map" in err(), win
    bad, _ = _record(src_w=9)
    assert counts(bad, tab, [0, 0, 8, 10]) == -2 and b"leaves the source" in err()

    ids = np.arange(300, dtype=np.int32)

    def bits(T=3, H=8, W=10, stride=10, map_=one, ids_=ids.ctypes.data, out=one, areas=one):
        return lib.mpf_label_bits(map_, stride, H, W, ids_, T, out, areas, None)

    assert bits(T=0) == 0                                    # nothing to do, nothing launched
    assert bits(T=0, map_=None, out=None) == 0
    assert bits(map_=None) == -3 and bits(ids_=None) == -3 and bits(out=None) == -3 and bits(areas=None) == -3
    assert bits(H=0) == -2 and bits(W=0) == -2 and bits(T=-1) == -2
    assert bits(stride=9) == -2 and b"stride" in err()
    assert bits(H=1 << 16, W=1 << 15, stride=1 << 15) == -4
    assert bits(T=256) == -4 and b"255 ids" in err()
