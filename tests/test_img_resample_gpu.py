"""GPU: the batched flip / resize / crop / pad kernel (csrc/img_resample.hip via mp_former_amd.augment.resample_images) against the
numpy restatement of PIL's 8-bit bilinear resize (tests/_resample_restate.py, pinned to PIL in tests/test_lsj_cpu.py).  Integer
equality everywhere; the float forms bit-equal to the torch expression on the device."""
import functools

import numpy as np
import pytest
import torch

import _resample_restate as R
from test_lsj_cpu import LIVE_ONLY, SHAPES, _id, source

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# the COCO statistics of the reference's configuration (MODEL.PIXEL_MEAN / PIXEL_STD)
MEAN, STD = [123.675, 116.280, 103.530], [58.395, 57.120, 57.375]
# crop windows of the 37 x 53 -> 74 x 106 result: (crop size, origin); sizes that are no multiple of a tile (32 rows, 64 columns)
WINDOWS = (((32, 40), (17, 29)), ((1, 1), (73, 105)), ((33, 65), (0, 0)))


def _np(t):
    return t.detach().cpu().numpy()


def _params(src, resized, flip=False, offset=(0, 0), crop=None):
    from mp_former_amd.augment import LSJParams
    crop = tuple(crop or resized)
    valid = (min(resized[0] - offset[0], crop[0]), min(resized[1] - offset[1], crop[1]))
    return LSJParams(bool(flip), tuple(src), tuple(resized), tuple(offset), crop, valid)


@functools.lru_cache(maxsize=None)
def _want(src_hw, resized, flip, offset, crop):
    """the restatement's uint8 [3, Sh, Sw], made once per case and left unchanged"""
    out = R.lsj_image(source(*src_hw), flip, resized, offset, crop)
    out.setflags(write=False)
    return out


def _run(p, **kw):
    from mp_former_amd.augment import resample_images
    return resample_images([torch.from_numpy(source(*p.src))], [p], **kw)[0]


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("shape", SHAPES + (LIVE_ONLY,), ids=_id)
def test_whole_image_equals_the_restatement(shape, flip):
    src_hw, resized = shape
    p = _params(src_hw, resized, flip)
    got = _run(p)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (3,) + resized and got.device == DEV
    np.testing.assert_array_equal(_np(got), _want(src_hw, resized, flip, (0, 0), resized))


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("window", WINDOWS, ids=["32x40@17,29", "1x1@last", "33x65@0,0"])
def test_crop_windows_equal_the_restatement(window, flip):
    crop, offset = window
    p = _params((37, 53), (74, 106), flip, offset, crop)
    assert p.valid == crop
    np.testing.assert_array_equal(_np(_run(p)), _want((37, 53), (74, 106), flip, offset, crop))


def test_padding_right_and_bottom():
    p = _params((37, 53), (5, 7), crop=(16, 16))
    got = _np(_run(p))
    np.testing.assert_array_equal(got, _want((37, 53), (5, 7), False, (0, 0), (16, 16)))
    assert (got[:, 5:, :] == 128).all() and (got[:, :, 7:] == 128).all()
    got = _np(_run(p, pad_value=7))
    assert (got[:, 5:, :] == 7).all() and (got[:, :, 7:] == 7).all()
    np.testing.assert_array_equal(got[:, :5, :7], _want((37, 53), (5, 7), False, (0, 0), (5, 7)))


BATCH = ((((37, 53), (74, 106)), True, (17, 29), (32, 40)), (((48, 64), (77, 102)), False, (40, 60), (32, 40)),
         (((19, 23), (5, 9)), False, (0, 0), (32, 40)))


def test_batch_of_three_in_one_launch_equals_the_single_calls():
    from mp_former_amd import _lib
    from mp_former_amd.augment import resample_images
    ps = [_params(s[0], s[1], flip, off, crop) for s, flip, off, crop in BATCH]
    imgs = [torch.from_numpy(source(*p.src)).to(DEV) for p in ps]
    _lib.profile_enable(True)
    try:
        got = resample_images(imgs, ps)
        torch.cuda.synchronize()
        launches = _lib.profile_get("img_resample_kernel")[0]
    finally:
        _lib.profile_enable(False)
    assert launches == 1 and tuple(got.shape) == (3, 3, 32, 40)
    for b, (p, (s, flip, off, crop)) in enumerate(zip(ps, BATCH)):
        np.testing.assert_array_equal(_np(got[b]), _want(s[0], s[1], flip, off, crop), err_msg=str(b))
        np.testing.assert_array_equal(_np(got[b]), _np(resample_images([imgs[b]], [p])[0]), err_msg=str(b))
    assert (_np(got[2])[:, 5:, :] == 128).all()


def test_tile_heights_mixed_in_one_batch():
    """a vertical ratio of 30 takes tiles of 4 rows, 12 of 16, the upscale of 32: the grid is sized for the smallest, and the workgroups
    an image with taller tiles does not need leave"""
    from mp_former_amd import augment as A
    cases = (((960, 16), (32, 16)), ((37, 53), (74, 106)), ((384, 9), (32, 9)))
    ps = [_params(s, r) for s, r in cases]
    assert [A._tile_h(A.resample_coeffs(p.src[0], p.resized[0])[1]) for p in ps] == [4, 32, 16]
    got = A.resample_images([torch.from_numpy(source(*p.src)) for p in ps], ps)
    assert tuple(got.shape) == (3, 3, 74, 106)
    for b, (s, r) in enumerate(cases):
        np.testing.assert_array_equal(_np(got[b, :, :r[0], :r[1]]), _want(s, r, False, (0, 0), r), err_msg=str(b))
        assert (_np(got[b, :, r[0]:, :]) == 0).all() and (_np(got[b, :, :, r[1]:]) == 0).all()


def test_every_output_byte_is_written_and_the_guard_bytes_stay():
    """the launch writes into a buffer prefilled with 0xA5 through the C entry point: the raw form of resample_images"""
    from mp_former_amd import _lib
    from mp_former_amd import augment as A
    p = _params((37, 53), (5, 7), crop=(16, 16))             # padding: the valid extent, the pad region and a 20 x 70 canvas
    for dtype, esz in ((torch.uint8, 1), (torch.float32, 4), (torch.bfloat16, 2)):
        Hc, Wc, guard = 20, 70, 4096
        buf = torch.full((3 * Hc * Wc * esz + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        src = torch.from_numpy(source(37, 53)).to(DEV)
        xk, xb = A.resample_coeffs(53, 7)
        yk, yb = A.resample_coeffs(37, 5)
        tab = np.concatenate([a.reshape(-1) for a in (xk, xb, yk, yb)]).astype(np.int32)
        offs = np.cumsum([0, xk.size, xb.size, yk.size])
        rec = np.array([A._i32(src.data_ptr()), A._i32(src.data_ptr() >> 32), 3 * 53, 37, 53, 0, 5, 7, 0, 0, 16, 16, 5, 7, A._tile_h(yb),
                        xk.shape[1], yk.shape[1], offs[0], offs[1], offs[2], offs[3], 0], dtype=np.int32)
        host = torch.from_numpy(np.concatenate([rec, tab]))
        dev = host.to(DEV)
        import ctypes
        mean, std = (ctypes.c_float * 3)(*MEAN), (ctypes.c_float * 3)(*STD)
        _lib.call("mpf_img_resample", DEV, host.data_ptr(), dev.data_ptr(), host.data_ptr() + 4 * 22, dev.data_ptr() + 4 * 22, int(tab.size),
                  1, buf.data_ptr(), _lib.DTYPE[dtype], Hc, Wc, 128, mean, std, _lib.stream_ptr(DEV))
        torch.cuda.synchronize()
        assert (_np(buf[-guard:]) == 0xA5).all(), dtype
        body = buf[:-guard].view(dtype).view(3, Hc, Wc)
        want = A.resample_images([src], [p], dtype=dtype, mean=MEAN, std=STD, canvas=(Hc, Wc))[0]
        assert torch.equal(body.view(torch.uint8), want.view(torch.uint8)), dtype
        if dtype == torch.uint8:
            u8 = _np(body)
            np.testing.assert_array_equal(u8[:, :16, :16], _want((37, 53), (5, 7), False, (0, 0), (16, 16)))
            assert (u8[:, 16:, :] == 0).all() and (u8[:, :, 16:] == 0).all()


def test_row_stride_larger_than_three_w():
    from mp_former_amd.augment import resample_images
    wide = torch.from_numpy(source(37, 70)).to(DEV)
    view = wide[:, 5:58]                                     # 37 x 53 with rows 210 bytes apart, starting 15 bytes in
    assert view.stride(0) == 210 and not view.is_contiguous()
    p = _params((37, 53), (74, 106), True, (17, 29), (32, 40))
    got = resample_images([view], [p])[0]
    want = R.lsj_image(source(37, 70)[:, 5:58], True, (74, 106), (17, 29), (32, 40))
    np.testing.assert_array_equal(_np(got), want)


@pytest.mark.parametrize("case", [((37, 53), (74, 106), True, (17, 29), (32, 40), (32, 64)), ((37, 53), (5, 7), False, (0, 0), (16, 16), (32, 96)),
                                  ((64, 960), (64, 32), False, (0, 0), (64, 32), (64, 32))], ids=["window", "padded", "ratio30"])
def test_float_forms_are_bit_equal_to_the_torch_expression(case):
    src_hw, resized, flip, offset, crop, canvas = case
    p = _params(src_hw, resized, flip, offset, crop)
    u8 = torch.from_numpy(_want(src_hw, resized, flip, offset, crop).copy()).to(DEV)
    mean, std = torch.tensor(MEAN, device=DEV), torch.tensor(STD, device=DEV)
    want = torch.zeros((3,) + canvas, dtype=torch.float32, device=DEV)
    want[:, :crop[0], :crop[1]] = (u8.float() - mean[:, None, None]) / std[:, None, None]
    got = _run(p, dtype=torch.float32, mean=MEAN, std=STD, canvas=canvas)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3,) + canvas
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    got16 = _run(p, dtype=torch.bfloat16, mean=mean, std=std, canvas=canvas)
    assert got16.dtype == torch.bfloat16 and torch.equal(got16.view(torch.int16), want.to(torch.bfloat16).view(torch.int16))
    # the pad region holds (128 - mean) / std, the canvas beyond the crop exactly 0 (+0.0)
    pad = ((torch.full((3,), 128.0, device=DEV) - mean) / std)
    vh, vw = p.valid
    if vh < crop[0]:
        assert torch.equal(got[:, vh:crop[0], :crop[1]], pad[:, None, None].expand(3, crop[0] - vh, crop[1]))
    if vw < crop[1]:
        assert torch.equal(got[:, :crop[0], vw:crop[1]], pad[:, None, None].expand(3, crop[0], crop[1] - vw))
    assert (got[:, crop[0]:, :].view(torch.int32) == 0).all() and (got[:, :, crop[1]:].view(torch.int32) == 0).all()


def test_resize_image_is_the_single_image_case():
    from mp_former_amd.augment import resize_image, shortest_edge_size
    size = shortest_edge_size(48, 64, 77, 200)
    assert size == (77, 103)
    got = resize_image(torch.from_numpy(source(48, 64)), size)
    np.testing.assert_array_equal(_np(got), R.resize(source(48, 64), *size).transpose(2, 0, 1))
