"""CPU: the COCO mask codec without a GPU — the restatement of pycocotools' rleFrPoly / rleToString / rleFrString
(tests/_codec_restate.py) pinned to hand-computed tables, the host-side string codec of mp_former_amd.inference against it, the
host-side argument checks of ``polygon_bits`` / ``rle_bits`` / ``segmentation_bits`` / ``unpack_masks``, and the new C entry points'
declarations and argument checks.

The rectangle's last run: the ring covers pixels 10..19 of both axes of a 30 x 30 image, so the last set position is 19 * 30 + 19 =
589 and 900 - 590 = 310 zeros follow (the counts must sum to H * W = 900: 310 + 10 * 10 + 9 * 20 + 310)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _ap_restate as R
import _codec_restate as C
from test_ap_cpu import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mpf_seg_poly_stage_edges", "mpf_seg_poly_toggles", "mpf_seg_rle_toggles", "mpf_seg_toggles_fill", "mpf_seg_unpack_masks")
STRINGS = (([0, 1], "01"), ([15], "?"), ([16], "`0"), ([31, 32, 1, 1024, 0, 7], "o0P11Po0OWPO"),
           ([9, 4, 4, 3, 5, 2, 6, 1, 30], "944O1O1Oh0"))
# (ring, H, W, counts)
RINGS = (([10, 10, 20, 10, 20, 20, 10, 20], 30, 30, [310] + [10, 20] * 9 + [10, 310]),
         ([1, 1, 6, 1, 1, 6], 8, 8, [9, 4, 4, 3, 5, 2, 6, 1, 30]),
         ([.5, .5, 3.5, .5, 3.5, 2.5, .5, 2.5], 4, 5, [5, 2, 2, 2, 2, 2, 5]),
         ([0, 0, 4, 4, 4, 0, 0, 4], 5, 5, [0, 3, 3, 1, 4, 1, 3, 3, 7]),
         ([0, 0, 7, 0, 7, 3, 0, 3], 3, 7, [0, 21]),
         ([2, 1, 2, 1, 2, 1], 4, 4, [16]))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ring,H,W,want", RINGS, ids=["rectangle", "triangle", "half-integer", "bow-tie", "full", "empty"])
def test_fr_poly_agrees_with_the_hand_computed_tables(ring, H, W, want):
    got = C.fr_poly(ring, H, W)
    assert got == want and sum(got) == H * W
    dense = C.decode(got, H, W)
    assert C.encode(dense) == want
    # the parity form the kernels use: a toggle per boundary position, then a running XOR
    flat = np.zeros(H * W + 1, dtype=np.int64)
    for p in C.boundary_positions(ring, H, W):
        flat[p] ^= 1
    np.testing.assert_array_equal((np.cumsum(flat[:-1]) & 1).astype(bool).reshape(W, H).T, dense)


def test_rectangle_covers_pixels_10_to_19():
    dense = C.decode(C.fr_poly(RINGS[0][0], 30, 30), 30, 30)
    want = np.zeros((30, 30), dtype=bool)
    want[10:20, 10:20] = True
    np.testing.assert_array_equal(dense, want)
    assert dense.sum() == 100


def test_sort_merge_form_and_parity_form_agree_on_random_rings():
    g = np.random.default_rng(7)
    for n in range(300):
        H, W = int(g.integers(1, 40)), int(g.integers(1, 40))
        k = int(g.integers(3, 9))
        kind = n % 3
        xy = g.uniform(-3, [W + 3, H + 3], size=(k, 2))
        if kind == 1:
            xy = np.round(xy)
        elif kind == 2:
            xy = np.round(xy * 2) / 2
        ring = xy.reshape(-1).tolist()
        dense = C.decode(C.fr_poly(ring, H, W), H, W)
        flat = np.zeros(H * W + 1, dtype=np.int64)
        for p in C.boundary_positions(ring, H, W):
            flat[p] ^= 1
        np.testing.assert_array_equal((np.cumsum(flat[:-1]) & 1).astype(bool).reshape(W, H).T, dense, err_msg=str((H, W, ring)))


def test_union_of_rings_and_the_mixed_forms():
    H, W = 8, 8
    a, b = [1, 1, 6, 1, 1, 6], [2, 2, 7, 2, 7, 7, 2, 7]
    ma, mb = C.decode(C.fr_poly(a, H, W), H, W), C.decode(C.fr_poly(b, H, W), H, W)
    assert (ma & mb).any(), "the two rings overlap: a union is not their XOR"
    np.testing.assert_array_equal(C.poly_mask([a, b], H, W), ma | mb)
    np.testing.assert_array_equal(C.poly_mask([b, a], H, W), ma | mb)
    assert not C.poly_mask([], H, W).any()
    counts = C.encode(ma)
    for segm in ([a], {"size": [H, W], "counts": counts}, {"size": [H, W], "counts": C.to_string(counts)},
                 {"size": [H, W], "counts": C.to_string(counts).encode()}):
        np.testing.assert_array_equal(C.segm_mask(segm, H, W), ma)
    assert not C.segm_mask(None, H, W).any()
    assert R.pack_columns(ma[None]).shape == (1, 1)


# ---- the string codec ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts,text", STRINGS)
def test_pinned_strings(counts, text):
    from mp_former_amd.inference import rle_compress, rle_from_string, rle_to_string
    assert C.to_string(counts) == text and C.from_string(text) == counts
    assert rle_to_string(counts) == text and rle_from_string(text) == counts and rle_from_string(text.encode()) == counts
    assert rle_compress({"size": (3, 4), "counts": counts}) == {"size": [3, 4], "counts": text}


def test_string_round_trips_of_random_counts():
    from mp_former_amd.inference import rle_from_string, rle_to_string
    g = np.random.default_rng(11)
    for n in range(400):
        k = int(g.integers(0, 40))
        hi = (2, 40, 1 << 12, 1 << 31)[n % 4]                # the large ones give negative differences of many groups
        counts = g.integers(0, hi, size=k).tolist()
        for i in g.integers(0, max(k, 1), size=k // 4).tolist():
            if k:
                counts[i] = 0                                 # zero-length runs anywhere
        text = rle_to_string(counts)
        assert text == C.to_string(counts), counts
        assert all(48 <= ord(ch) < 112 for ch in text)
        assert rle_from_string(text) == counts and C.from_string(text) == counts
    assert rle_to_string([]) == "" and rle_from_string("") == []
    assert rle_from_string(rle_to_string([1, 2, 9, 1000, 3, 2])) == [1, 2, 9, 1000, 3, 2]      # 3 - 9 and 2 - 1000: negative differences


def test_bad_strings_and_counts_raise():
    from mp_former_amd.inference import rle_from_string, rle_to_string
    with pytest.raises(ValueError, match="ends inside"):
        rle_from_string("o")                                 # bit 0x20 set and nothing follows
    with pytest.raises(ValueError, match="COCO encoding"):
        rle_from_string("0 1")
    with pytest.raises(ValueError, match="non-negative"):
        rle_to_string([3, -1])


# ---- the host-side checks -----------------------------------------------------------------------------------------------------------
def test_host_side_value_errors_come_before_any_device_work():
    from mp_former_amd.inference import polygon_bits, polygon_masks, rle_bits, segmentation_bits
    ok = [0, 0, 4, 0, 4, 4]
    for bad, what in (([0, 0, 4, 0, 4], "odd length"), ([0, 0, 4, 4], "at least 6"), ([0, 0, float("nan"), 0, 4, 4], "non-finite"),
                      ([0, 0, float("inf"), 0, 4, 4], "non-finite"), ([0, 0, 2.0 ** 31 / 5, 0, 4, 4], "2\\^31"),
                      ([0, 0, -2.0 ** 31 / 5 - 1, 0, 4, 4], "2\\^31")):
        with pytest.raises(ValueError, match=what):
            polygon_bits([[ok], [ok, bad]], (9, 9))
        with pytest.raises(ValueError, match=what):
            polygon_masks([[bad]], (9, 9))
        with pytest.raises(ValueError, match=what):
            segmentation_bits([None, [bad]], (9, 9))
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        polygon_bits([[ok]], None)
    with pytest.raises(ValueError, match="H, W > 0"):
        polygon_bits([[ok]], (0, 9))
    with pytest.raises(ValueError, match="list of rings"):
        polygon_bits([7], (9, 9))
    good = {"size": [3, 4], "counts": [5, 2, 5]}
    with pytest.raises(ValueError, match="sum to 11"):
        rle_bits([good, {"size": [3, 4], "counts": [5, 2, 4]}])
    with pytest.raises(ValueError, match="sum to 13"):
        rle_bits([{"size": [3, 4], "counts": C.to_string([5, 2, 6])}])
    with pytest.raises(ValueError, match="expected 3 x 4"):
        rle_bits([good, {"size": [4, 3], "counts": [12]}])
    with pytest.raises(ValueError, match="expected 4 x 3"):
        rle_bits([good], size=(4, 3))
    with pytest.raises(ValueError, match="negative"):
        rle_bits([{"size": [3, 4], "counts": [13, -1]}])
    with pytest.raises(ValueError, match="size must be given"):
        rle_bits([])
    with pytest.raises(ValueError, match="\"size\" and \"counts\""):
        rle_bits([{"counts": [12]}])
    with pytest.raises(ValueError, match="expected polygons"):
        segmentation_bits([good, 5], (3, 4))
    with pytest.raises(ValueError, match="expected 5 x 4"):
        segmentation_bits([[ok], good], (5, 4))


def test_cpu_devices_and_tensors_raise():
    from mp_former_amd.inference import polygon_bits, polygon_masks, rle_bits, segmentation_bits, unpack_masks
    ok = [0, 0, 4, 0, 4, 4]
    good = {"size": [3, 4], "counts": [5, 2, 5]}
    for call in (lambda: polygon_bits([[ok]], (9, 9), device="cpu"), lambda: polygon_masks([[ok]], (9, 9), device="cpu"),
                 lambda: rle_bits([good], device="cpu"), lambda: segmentation_bits([[ok], None], (9, 9), device="cpu"),
                 lambda: unpack_masks(torch.zeros(2, 1, dtype=torch.int64), (7, 9))):
        with pytest.raises(RuntimeError, match=r"Not implemented on the CPU \(device tensors only\)"):
            call()
    w = lambda *s, dt=torch.int64: _FakeCuda(torch.zeros(*s, dtype=dt))        # noqa: E731
    with pytest.raises(ValueError, match="int64"):
        unpack_masks(w(2, 1, dt=torch.int32), (7, 9))
    with pytest.raises(ValueError, match="does not fit"):
        unpack_masks(w(2, 1), (9, 9))
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        unpack_masks(w(2, 1), None)
    with pytest.raises(TypeError, match="bool, uint8 or float32"):
        unpack_masks(w(2, 1), (7, 9), dtype=torch.float16)


def test_evaluators_take_the_new_options():
    import inspect
    from mp_former_amd import d2_plugin
    ev = d2_plugin.InstanceAPEvaluator(3, dataset_id_to_contiguous={1: 0, 18: 1, 44: 2})
    assert ev.dataset_id_to_contiguous == {1: 0, 18: 1, 44: 2} and d2_plugin.InstanceAPEvaluator(3).dataset_id_to_contiguous is None
    assert inspect.signature(d2_plugin.YTVISEvaluatorHIP.results_json).parameters["compressed"].default is False
    rle = {"size": [8, 8], "counts": [9, 4, 4, 3, 5, 2, 6, 1, 30]}
    out = {"pred_scores": [0.9], "pred_labels": [2], "pred_masks_rle": [[rle, rle]]}
    plain = d2_plugin.YTVISEvaluatorHIP.results_json(5, out)
    assert plain == [{"video_id": 5, "score": 0.9, "category_id": 2, "segmentations": [rle, rle]}]
    packed = d2_plugin.YTVISEvaluatorHIP.results_json(5, out, compressed=True)
    assert packed[0]["segmentations"] == [{"size": [8, 8], "counts": "944O1O1Oh0"}] * 2 and packed[0]["score"] == 0.9
    assert d2_plugin.compress_rles([rle, None]) == [{"size": [8, 8], "counts": "944O1O1Oh0"}, None]
    assert rle["counts"] == [9, 4, 4, 3, 5, 2, 6, 1, 30], "the input was modified"


# ---- the C entry points -------------------------------------------------------------------------------------------------------------
def test_codec_symbols_declared_exported_and_bound(built):
    src = open(os.path.join(ROOT, "include", "mpformer_hip.h")).read()
    assert "rleFrPoly" in src and "rleMerge" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(raw, name) and name in built.SIGNATURES, name
    assert os.path.exists(os.path.join(ROOT, "mp_former_amd", "csrc", "seg_codec.hip"))
    assert "seg_codec.hip" in open(os.path.join(ROOT, "mp_former_amd", "csrc", "Makefile")).read()
    assert built.lib().mpf_abi_version() == 1
    assert built.lib().mpf_seg_poly_stage_edges() >= 64


def test_codec_entry_points_reject_bad_arguments(built):
    lib = built.lib()
    one = ctypes.c_void_p(16)       # never dereferenced: the checks come first

    def poly(xy=one, off=one, R=2, H=7, W=9, planes=one):
        return lib.mpf_seg_poly_toggles(xy, off, R, H, W, planes, None)

    def rle(counts=one, off=one, M=2, H=7, W=9, planes=one):
        return lib.mpf_seg_rle_toggles(counts, off, M, H, W, planes, None)

    def fill(planes=one, obj=one, R=3, M=2, H=7, W=9, bits=one):
        return lib.mpf_seg_toggles_fill(planes, obj, R, M, H, W, bits, None)

    def unpack(bits=one, M=2, H=7, W=9, masks=one):
        return lib.mpf_seg_unpack_masks(bits, M, H, W, masks, None)
    for f, ptrs, n in ((poly, ("xy", "off", "planes"), "R"), (rle, ("counts", "off", "planes"), "M"), (fill, ("planes", "obj", "bits"), "M"),
                       (unpack, ("bits", "masks"), "M")):
        for k in ptrs:
            assert f(**{k: None}) == -3 and b"NULL" in lib.mpf_last_error(), (f.__name__, k)
        assert f(**{n: -1}) == -2 and f(H=0) == -2 and f(W=-3) == -2, f.__name__
        assert f(H=1 << 16, W=1 << 15) == -4, f.__name__
        assert f(**{n: 0}, **{k: None for k in ptrs}) == 0, f.__name__                # nothing to do, nothing launched
    assert poly(R=1 << 24) == -4 and rle(M=1 << 24) == -4 and fill(R=1 << 24) == -4
    assert fill(M=70000) == -4 and unpack(M=70000) == -4 and fill(R=-1) == -2
    assert b"seg_unpack_masks" in lib.mpf_last_error() or b"seg_toggles_fill" in lib.mpf_last_error()
