"""CPU: large-scale-jitter input without a GPU — the numpy restatement of PIL's 8-bit bilinear resize (tests/_resample_restate.py)
pinned to outputs recorded from PIL (tests/golden/lsj_pil_resize.npz) and to the installed PIL where it imports, the coefficient
tables and detectron2's geometry of mp_former_amd.augment against it and against hand-derived values, the vertex transforms, and
the new C entry point's declaration, binding and argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _resample_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lsj_pil_resize.npz")
# source -> output, H x W
SHAPES = (((37, 53), (74, 106)), ((37, 53), (5, 7)), ((37, 53), (37, 53)), ((37, 53), (61, 53)), ((37, 53), (37, 20)),
          ((48, 64), (77, 102)), ((19, 23), (64, 9)), ((1, 5), (3, 11)), ((64, 960), (64, 32)))
LIVE_ONLY = ((480, 640), (77, 102))
NEW_SYMBOLS = ("mpf_img_resample", "mpf_img_resample_span_rows", "mpf_img_resample_max_ratio", "mpf_img_resample_ksize",
               "mpf_img_resample_tables")


def source(h, w, seed=0):
    """random bytes overlaid with a 0 / 255 checkerboard (3 x 3 squares on a random half of the pixels)"""
    g = np.random.default_rng(1000 * h + w + seed)
    img = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[:h, :w]
    board = ((yy // 3 + xx // 3) & 1).astype(bool)
    over = g.random((h, w)) < 0.5
    img[over & board] = 255
    img[over & ~board] = 0
    return img


def _id(s):
    return "%dx%d-%dx%d" % (s[0] + s[1])


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_restatement_equals_the_recorded_pil_outputs(shape):
    z = np.load(GOLDEN)
    (h, w), (oh, ow) = shape
    src = z["src_%dx%d" % (h, w)]
    np.testing.assert_array_equal(src, source(h, w))         # the fixture's sources are the generator's
    want = z["out_%s" % _id(shape)]
    assert want.shape == (oh, ow, 3)
    np.testing.assert_array_equal(R.resize(src, oh, ow), want)


@pytest.mark.parametrize("shape", SHAPES + (LIVE_ONLY,), ids=_id)
def test_restatement_equals_live_pil(shape):
    Image = pytest.importorskip("PIL.Image")
    (h, w), (oh, ow) = shape
    src = source(h, w)
    want = np.asarray(Image.fromarray(src).resize((ow, oh), Image.BILINEAR))
    np.testing.assert_array_equal(R.resize(src, oh, ow), want)


def test_flipped_read_with_unflipped_tables_is_pil_on_the_flipped_image():
    src = source(19, 23)
    coef, bounds = R.axis_tables(23, 9)
    out = np.zeros((19, 9, 3), dtype=np.uint8)
    for xx in range(9):
        x0, n = bounds[xx]
        cols = 23 - 1 - np.arange(x0, x0 + n)
        acc = (1 << 21) + (src[:, cols, :].astype(np.int64) * coef[xx, :n].astype(np.int64)[None, :, None]).sum(axis=1)
        out[:, xx] = np.clip(acc >> 22, 0, 255)
    np.testing.assert_array_equal(out, R.resize(src[:, ::-1], 19, 9))


# ---- the tables -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes", [(53, 106), (53, 7), (53, 53), (37, 61), (53, 20), (64, 102), (23, 9), (1, 3), (5, 11), (960, 32),
                                   (640, 2048), (640, 102), (480, 77), (1000, 16)])
def test_resample_coeffs_equal_the_restatement(sizes):
    from mp_former_amd.augment import resample_coeffs
    n_in, n_out = sizes
    coef, bounds = R.axis_tables(n_in, n_out)
    got_c, got_b = resample_coeffs(n_in, n_out)
    assert got_c.dtype == np.int32 and got_b.dtype == np.int32 and got_c.shape == coef.shape
    np.testing.assert_array_equal(got_c, coef)
    np.testing.assert_array_equal(got_b, bounds)
    first, count = n_out // 3, max(1, n_out // 2)
    count = min(count, n_out - first)
    win_c, win_b = resample_coeffs(n_in, n_out, first=first, count=count)
    np.testing.assert_array_equal(win_c, coef[first:first + count])
    np.testing.assert_array_equal(win_b, bounds[first:first + count])
    # an identity pass is the identity by the same formula: one tap of weight 2^22
    if n_in == n_out:
        assert (coef[:, 0] == 1 << 22).all() and (coef[:, 1:] == 0).all() and (bounds[:, 0] == np.arange(n_out)).all()
    with pytest.raises(ValueError, match="first"):
        resample_coeffs(n_in, n_out, first=n_out, count=1)


def test_the_library_host_tables_equal_the_restatement(built):
    """resample_images fills its staging buffer with the library's host code: the same integers as the numpy forms"""
    from mp_former_amd.augment import resample_coeffs
    lib = built.lib()
    g = np.random.default_rng(17)
    sizes = [(53, 106), (53, 7), (53, 53), (37, 61), (23, 9), (1, 3), (5, 11), (960, 32), (640, 2048), (640, 102), (480, 77), (1000, 16)]
    sizes += [(int(g.integers(1, 3000)), int(g.integers(1, 3000))) for _ in range(300)]
    done = 0
    for n_in, n_out in sizes:
        if n_in > 64 * n_out:
            assert lib.mpf_img_resample_tables(n_in, n_out, 0, n_out, None, None) == -2
            continue
        coef, bounds = R.axis_tables(n_in, n_out) if n_out <= 128 else resample_coeffs(n_in, n_out)      # (the loop form is slow when long)
        first = int(g.integers(0, n_out))
        count = int(g.integers(0, n_out - first + 1))
        assert lib.mpf_img_resample_ksize(n_in, n_out) == coef.shape[1]
        got_c = np.full((count, coef.shape[1]), -7, dtype=np.int32)
        got_b = np.full((count, 2), -7, dtype=np.int32)
        assert lib.mpf_img_resample_tables(n_in, n_out, first, count, got_c.ctypes.data, got_b.ctypes.data) == 0
        np.testing.assert_array_equal(got_c, coef[first:first + count], err_msg=str((n_in, n_out)))
        np.testing.assert_array_equal(got_b, bounds[first:first + count])
        done += 1
    assert done > 250
    assert lib.mpf_img_resample_ksize(0, 5) == 0 and lib.mpf_img_resample_tables(5, 5, 3, 3, None, None) == -2
    assert lib.mpf_img_resample_tables(5, 5, 0, 5, None, None) == -3 and lib.mpf_img_resample_tables(5, 5, 2, 0, None, None) == 0


# ---- the geometry -----------------------------------------------------------------------------------------------------------------------
def test_geometry_by_hand():
    from mp_former_amd import augment as A
    assert A.resize_scale_size(480, 640, 2.0, 1024, 1024) == (1536, 2048)
    assert A.fixed_crop(1536, 2048, 1024, 1024, 0.5) == ((256, 512), (1024, 1024))
    assert A.resize_scale_size(480, 640, 0.1, 1024, 1024) == (77, 102)
    assert A.fixed_crop(77, 102, 1024, 1024, 0.7) == ((0, 0), (77, 102))
    assert A.shortest_edge_size(480, 640, 800, 1333) == (800, 1067)
    assert A.shortest_edge_size(640, 480, 800, 1333) == (1067, 800)
    assert A.shortest_edge_size(300, 1000, 800, 1333) == (400, 1333)
    p = A.lsj_params(480, 640, True, 2.0, 0.5)
    assert p == A.LSJParams(True, (480, 640), (1536, 2048), (256, 512), (1024, 1024), (1024, 1024))
    p = A.lsj_params(480, 640, False, 0.1, 0.9)
    assert (p.resized, p.offset, p.valid, p.crop) == ((77, 102), (0, 0), (77, 102), (1024, 1024))
    g = np.random.default_rng(3)
    for _ in range(200):
        h, w, s, u = int(g.integers(1, 700)), int(g.integers(1, 700)), float(g.uniform(0.1, 2.0)), float(g.uniform())
        size = A.resize_scale_size(h, w, s, 256, 320)
        assert size == R.resize_scale_size(h, w, s, 256, 320)
        assert A.fixed_crop(size[0], size[1], 256, 320, u) == R.fixed_crop(size[0], size[1], 256, 320, u)
        assert A.shortest_edge_size(h, w, 200, 333) == R.shortest_edge_size(h, w, 200, 333)


class _Stub:
    """a generator that hands out a fixed list and records how it was asked"""

    def __init__(self, values):
        self.values, self.calls = list(values), []

    def uniform(self, *args):
        self.calls.append(args)
        return self.values.pop(0)


def test_draw_lsj_consumes_flip_scale_crop_in_that_order():
    from mp_former_amd import augment as A
    g = _Stub([0.3, 2.0, 0.5])
    p = A.draw_lsj(480, 640, rng=g)
    assert g.calls == [(), (0.1, 2.0), (0.0, 1.0)] and not g.values
    assert p == A.lsj_params(480, 640, True, 2.0, 0.5)
    g = _Stub([0.5, 0.1, 0.25])
    assert A.draw_lsj(480, 640, rng=g).flip is False                        # uniform() < 0.5
    g = _Stub([1.0, 0.75])
    p = A.draw_lsj(480, 640, image_size=512, min_scale=0.5, max_scale=1.5, flip=False, rng=g)
    assert g.calls == [(0.5, 1.5), (0.0, 1.0)] and p == A.lsj_params(480, 640, False, 1.0, 0.75, 512)
    for rng in (np.random.default_rng(5), np.random.RandomState(5)):
        p = A.draw_lsj(333, 500, image_size=64, rng=rng)
        assert p.crop == (64, 64) and p.valid[0] <= 64 and p.valid[1] <= 64


# ---- the vertices -----------------------------------------------------------------------------------------------------------------------
def test_transform_polygons_by_the_written_formulas():
    from mp_former_amd import augment as A
    tri = [3.0, 4.0, 40.5, 7.25, 11.0, 30.0]
    x, y = np.array(tri[0::2]), np.array(tri[1::2])
    H, W = 37, 53

    def run(flip, resized, offset):
        p = A.LSJParams(flip, (H, W), resized, offset, (32, 32), (min(resized[0] - offset[0], 32), min(resized[1] - offset[1], 32)))
        (out,) = A.transform_polygons([tri], p)
        assert out.dtype == np.float64
        np.testing.assert_array_equal(out, R.transform_ring(tri, flip, (H, W), resized, offset))
        return out[0::2], out[1::2]

    gx, gy = run(True, (H, W), (0, 0))
    np.testing.assert_array_equal(gx, W - x)
    np.testing.assert_array_equal(gy, y)
    gx, gy = run(False, (74, 107), (0, 0))
    np.testing.assert_array_equal(gx, x * (107 / 53))
    np.testing.assert_array_equal(gy, y * (74 / 37))
    gx, gy = run(False, (H, W), (3, 9))
    np.testing.assert_array_equal(gx, x - 9)
    np.testing.assert_array_equal(gy, y - 3)
    gx, gy = run(True, (61, 90), (5, 20))
    np.testing.assert_array_equal(gx, (W - x) * (90 / 53) - 20)
    np.testing.assert_array_equal(gy, y * (61 / 37) - 5)
    assert tri == [3.0, 4.0, 40.5, 7.25, 11.0, 30.0], "the input was modified"


# ---- the entry point ------------------------------------------------------------------------------------------------------------------
def test_resample_symbols_declared_exported_and_bound(built):
    from mp_former_amd import augment as A
    src = open(os.path.join(ROOT, "include", "mpformer_hip.h")).read()
    assert "ImagingResample" in src and "MpfResampleRecord" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(raw, name) and name in built.SIGNATURES, name
    assert "img_resample.hip" in open(os.path.join(ROOT, "mp_former_amd", "csrc", "Makefile")).read()
    assert built.lib().mpf_img_resample_span_rows() == A.SPAN_ROWS
    assert built.lib().mpf_img_resample_max_ratio() == A.MAX_RATIO >= 32
    # the record of the header is the one augment.py fills: a pointer and 20 int32
    fields = re.search(r"typedef struct MpfResampleRecord \{(.*?)\}", code, flags=re.S).group(1)
    assert len(re.findall(r"\b\w+\s*[,;]", fields.replace("const void* src;", ""))) == 20 and A._REC_WORDS == 22


def _record(lib_tab, src_hw=(8, 10), out_hw=(8, 10), **over):
    """a consistent host record + table buffer for an identity resize of a fake source pointer (never dereferenced)"""
    from mp_former_amd import augment as A
    xk, xb = A.resample_coeffs(src_hw[1], out_hw[1])
    yk, yb = A.resample_coeffs(src_hw[0], out_hw[0])
    tab = np.concatenate([a.reshape(-1) for a in (xk, xb, yk, yb)]).astype(np.int32)
    offs = np.cumsum([0, xk.size, xb.size, yk.size])
    f = dict(src_lo=4096, src_hi=0, src_stride=3 * src_hw[1], src_h=src_hw[0], src_w=src_hw[1], flip=0, out_h=out_hw[0], out_w=out_hw[1],
             off_y=0, off_x=0, crop_h=out_hw[0], crop_w=out_hw[1], valid_h=out_hw[0], valid_w=out_hw[1], tile_h=1, ksize_x=xk.shape[1],
             ksize_y=yk.shape[1], xk_off=int(offs[0]), xb_off=int(offs[1]), yk_off=int(offs[2]), yb_off=int(offs[3]), reserved=0)
    f.update(over)
    return np.array(list(f.values()), dtype=np.int32), tab


def test_entry_point_rejects_bad_arguments_before_any_launch(built):
    lib = built.lib()
    one = ctypes.c_void_p(4096)      # never dereferenced: the checks come first
    mean = (ctypes.c_float * 3)(1, 2, 3)

    def run(rec, tab, B=1, out=one, dtype=3, Hc=8, Wc=10, pad=128, mean=None, std=None, recs_dev=one, tab_dev=one, tab_len=None):
        return lib.mpf_img_resample(rec.ctypes.data, recs_dev, tab.ctypes.data, tab_dev, len(tab) if tab_len is None else tab_len, B, out,
                                    dtype, Hc, Wc, pad, mean, std, None)

    rec, tab = _record(lib)
    assert run(rec, tab, B=0) == 0                           # nothing to do, nothing launched
    assert run(rec, tab, out=None) == -3 and run(rec, tab, recs_dev=None) == -3 and run(rec, tab, tab_dev=None) == -3
    assert run(rec, tab, dtype=1) == -1
    assert run(rec, tab, dtype=0) == -3 and b"mean and std" in lib.mpf_last_error()
    assert run(rec, tab, dtype=0, mean=mean) == -3
    assert run(rec, tab, B=-1) == -2 and run(rec, tab, Hc=0) == -2 and run(rec, tab, pad=256) == -2
    assert run(rec, tab, Hc=7) == -2 and b"canvas smaller" in lib.mpf_last_error()
    assert run(rec, tab, Wc=9) == -2
    assert run(rec, tab, B=70000) == -4
    for over, what in ((dict(src_lo=0), b"NULL"), (dict(src_stride=29), b"stride"), (dict(tile_h=0), b"tile_h"), (dict(tile_h=33), b"tile_h"),
                       (dict(valid_h=9), b"valid extent"), (dict(off_x=1), b"valid extent"), (dict(src_w=9), b"leaves the source"),
                       (dict(src_h=7), b"leaves the source"), (dict(ksize_x=0), b"taps"), (dict(ksize_y=130), b"taps"),
                       (dict(yb_off=10 ** 6), b"outside the table"), (dict(xk_off=-1), b"outside the table")):
        bad, _ = _record(lib, **over)
        assert run(bad, tab) < 0 and what in lib.mpf_last_error(), over
    assert run(rec, tab, tab_len=len(tab) - 1) == -2 and b"outside the table" in lib.mpf_last_error()
    # a ratio above the limit, and a tile too tall for its ratio
    rec, tab = _record(lib, src_hw=(8, 650), out_hw=(8, 10))
    assert run(rec, tab) == -2 and b"above 64" in lib.mpf_last_error()
    rec, tab = _record(lib, src_hw=(1920, 10), out_hw=(64, 10), tile_h=32)
    assert run(rec, tab, Hc=64) == -2 and b"256 source rows" in lib.mpf_last_error()
    moved = tab.copy()
    moved[rec[20] + 2] = 99                                     # the second row's first tap before ... after the image's end
    assert run(rec, moved, Hc=64) == -2


def test_python_argument_errors_come_before_any_device_work():
    from mp_former_amd import augment as A
    img = torch.zeros(8, 10, 3, dtype=torch.uint8)
    p = A.resize_params(8, 10, (16, 20))
    with pytest.raises(RuntimeError, match=r"Not implemented on the CPU \(device tensors only\)"):
        A.resample_images([img], [p], device="cpu")
    with pytest.raises(RuntimeError, match=r"Not implemented on the CPU \(device tensors only\)"):
        A.lsj_targets([], p, device="cpu")
    with pytest.raises(ValueError, match="must be uint8"):
        A.resample_images([img.float()], [p])
    with pytest.raises(ValueError, match="3 channels"):
        A.resample_images([torch.zeros(8, 10, 4, dtype=torch.uint8)], [A.resize_params(8, 10, (16, 20))])
    with pytest.raises(ValueError, match="3 channels"):
        A.resample_images([torch.zeros(8, 10, dtype=torch.uint8)], [p])
    with pytest.raises(ValueError, match="parameters say"):
        A.resample_images([torch.zeros(9, 10, 3, dtype=torch.uint8)], [p])
    with pytest.raises(ValueError, match="smaller than the crop"):
        A.resample_images([img], [p], canvas=(16, 19))
    with pytest.raises(ValueError, match="mean and std"):
        A.resample_images([img], [p], dtype=torch.float32)
    with pytest.raises(ValueError, match="mean and std"):
        A.resample_images([img], [p], dtype=torch.bfloat16, mean=[1.0, 2.0, 3.0])
    with pytest.raises(TypeError, match="uint8, float32 or bfloat16"):
        A.resample_images([img], [p], dtype=torch.float16, mean=[1.0] * 3, std=[1.0] * 3)
    wide = torch.zeros(8, 650, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="limited to 64"):
        A.resample_images([wide], [A.resize_params(8, 650, (8, 10))])
    with pytest.raises(ValueError, match="limited to 64"):
        A.resize_image(wide.permute(1, 0, 2), (10, 8))
    with pytest.raises(ValueError, match="1 images but 2"):
        A.resample_images([img], [p, p])
    # the tile rule: the tallest tile whose source rows fit the LDS buffer; th rows at ratio r tap about (th - 1) r + 2 r + 1 rows
    # (6.25: 207 of 256 at 32; 8: 265 at 32, 137 at 16; 12: 204 at 16; 20: 180 at 8; 30: 150 at 4; 32: 160 at 4; 64: 192 at 2)
    for ratio, want in ((0.3, 32), (1, 32), (6.25, 32), (8, 16), (12, 16), (20, 8), (30, 4), (32, 4), (64, 2)):
        n_out = 64
        _, yb = A.resample_coeffs(int(n_out * ratio), n_out)
        assert A._tile_h(yb) == want, ratio


def test_mapper_returns_the_raw_image_the_draw_and_the_non_crowd_annotations():
    from mp_former_amd import augment as A
    from mp_former_amd import d2_plugin
    raw = np.arange(37 * 53 * 3, dtype=np.uint8).reshape(37, 53, 3)
    seen = []

    def read_image(name, format=None):
        seen.append((name, format))
        return raw

    mapper = d2_plugin.COCOInstanceLSJDeviceMapper(True, image_size=32, min_scale=0.5, max_scale=1.5, random_flip="horizontal",
                                                   image_format="RGB", read_image=read_image)
    tri = [1.0, 1.0, 20.0, 2.0, 5.0, 30.0]
    d = {"file_name": "a.jpg", "height": 37, "width": 53, "image_id": 7,
         "annotations": [{"category_id": 3, "iscrowd": 0, "segmentation": [tri], "keypoints": [1, 2, 3], "bbox": [1, 1, 19, 29]},
                         {"category_id": 4, "iscrowd": 1, "segmentation": [tri]}]}
    state = np.random.get_state()
    try:
        np.random.seed(11)
        out = mapper(d)
        np.random.seed(11)
        want = A.draw_lsj(37, 53, image_size=32, min_scale=0.5, max_scale=1.5, flip=True, rng=np.random)
    finally:
        np.random.set_state(state)
    assert seen == [("a.jpg", "RGB")] and out["lsj"] == want and out["image_id"] == 7
    assert out["image_raw"].dtype == torch.uint8 and tuple(out["image_raw"].shape) == (37, 53, 3)
    np.testing.assert_array_equal(out["image_raw"].numpy(), raw)
    assert "image" not in out and "instances" not in out
    assert [a["category_id"] for a in out["annotations"]] == [3] and "keypoints" not in out["annotations"][0]
    assert "keypoints" in d["annotations"][0], "the input was modified"
    none = d2_plugin.COCOInstanceLSJDeviceMapper(True, image_size=32, min_scale=0.5, max_scale=1.5, random_flip="none", image_format="RGB",
                                                 read_image=read_image)
    assert none(d)["lsj"].flip is False
    with pytest.raises(ValueError, match="horizontal"):
        d2_plugin.COCOInstanceLSJDeviceMapper(True, image_size=32, min_scale=0.5, max_scale=1.5, random_flip="vertical", image_format="RGB")

    class _Cfg:
        class INPUT:
            IMAGE_SIZE, MIN_SCALE, MAX_SCALE, RANDOM_FLIP, FORMAT = 1024, 0.1, 2.0, "horizontal", "RGB"
        MODEL = None

    m = d2_plugin.COCOInstanceLSJDeviceMapper(_Cfg, True)
    assert (m.image_size, m.min_scale, m.max_scale, m.random_flip, m.image_format, m.is_train) == (1024, 0.1, 2.0, "horizontal", "RGB", True)
