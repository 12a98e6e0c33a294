"""CPU: Boundary AP without a GPU — the numpy restatement of boundary-iou-api (tests/_boundary_restate.py) against
scipy.ndimage.binary_erosion as an independent second formulation, the dilation distance, the difference Boundary IoU makes on the
golden scenes of instance mask AP, the new C entry points' declarations and argument checks, and the host-side checks of
``mask_boundaries``, ``InstanceAP(iou_type="boundary")`` and ``d2_plugin.InstanceAPEvaluator(iou_types=...)``.

boundary_iou, cv2 and pycocotools are not installed where this suite runs, so no golden was made by running the package: the
restatement is the specification and scipy its check."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _ap_restate as R
import _boundary_restate as B
from test_ap_cpu import _FakeCuda, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mpf_seg_mask_boundary", "mpf_seg_ap_match_boundary")
SHAPES = [(1, 1), (1, 64), (7, 9), (64, 1), (37, 50), (65, 63), (64, 64), (33, 56), (61, 83), (130, 70)]
DS = (1, 2, 3, 7, 40, 70)
KINDS = ("half", "dense", "blobs", "ones")
# (H, W, ratio) -> d; the halves: 75 x 100 has diagonal 125 (2.5 -> 2), 225 x 300 has 375 (7.5 -> 8)
DILATIONS = [(37, 50, 0.02, 1), (61, 83, 0.02, 2), (480, 640, 0.02, 16), (1024, 1024, 0.02, 29), (2000, 3000, 0.02, 72),
             (75, 100, 0.02, 2), (225, 300, 0.02, 8), (37, 50, 0.001, 1)]


def make_mask(kind, H, W, seed):
    """the four mask kinds of the erosion tests: density 0.5, density 0.9, blobs (sparse seeds dilated 4 times), all ones"""
    g = np.random.default_rng(seed)
    if kind == "half":
        return g.random((H, W)) < 0.5
    if kind == "dense":
        return g.random((H, W)) < 0.9
    if kind == "ones":
        return np.ones((H, W), dtype=bool)
    m = g.random((H, W)) < 0.02
    m[g.integers(0, H), g.integers(0, W)] = True
    for _ in range(4):
        p = np.zeros((H + 2, W + 2), dtype=bool)
        p[1:-1, 1:-1] = m
        m = (p[:-2, :-2] | p[:-2, 1:-1] | p[:-2, 2:] | p[1:-1, :-2] | p[1:-1, 1:-1] | p[1:-1, 2:] | p[2:, :-2] | p[2:, 1:-1] | p[2:, 2:])
    return m


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", SHAPES, ids=lambda o: f"{o[0]}x{o[1]}")
def test_restated_erosion_equals_scipy(hw):
    from scipy import ndimage
    H, W = hw
    n_changed = 0
    for d in DS:
        for k, kind in enumerate(KINDS):
            m = make_mask(kind, H, W, seed=H * 1000 + W * 10 + k)
            want = ndimage.binary_erosion(m, np.ones((3, 3), dtype=bool), iterations=d, border_value=0)
            got = B.erode(m, d)
            np.testing.assert_array_equal(got, want, err_msg=f"{H}x{W} d={d} {kind}")
            # the separable box form: a window AND along y, then along x, outside unset
            p = np.zeros((H + 2 * d, W + 2 * d), dtype=bool)
            p[d:d + H, d:d + W] = m
            ty = np.logical_and.reduce([p[k2:k2 + H, :] for k2 in range(2 * d + 1)])
            box = np.logical_and.reduce([ty[:, k2:k2 + W] for k2 in range(2 * d + 1)])
            np.testing.assert_array_equal(got, box, err_msg=f"{H}x{W} d={d} {kind} (box)")
            bd = B.mask_to_boundary(m, d)
            np.testing.assert_array_equal(bd, m & ~want)
            if 2 * d + 1 > min(H, W):
                assert not got.any() and np.array_equal(bd, m)
            n_changed += int(got.any())
    if min(H, W) >= 33:
        assert n_changed > 0, "no case of this shape kept an eroded pixel"


@pytest.mark.parametrize("H,W,ratio,want", DILATIONS)
def test_boundary_dilation(H, W, ratio, want):
    from mp_former_amd.inference import boundary_dilation
    assert B.boundary_dilation(H, W, ratio) == want
    got = boundary_dilation(H, W, ratio)
    assert got == want and isinstance(got, int)
    assert boundary_dilation(H, W) == B.boundary_dilation(H, W)          # the default ratio is the tool's 0.020


def test_boundary_dilation_rejects_an_empty_image():
    from mp_former_amd.inference import boundary_dilation
    with pytest.raises(ValueError):
        boundary_dilation(0, 5)


@pytest.mark.parametrize("rule", ["coco", "union"])
def test_boundary_evaluation_differs_from_the_mask_evaluation_on_the_golden_scenes(rule):
    g = load_golden()
    s = g["coco"]
    assert [B.boundary_dilation(H, W) for H, W in g["sizes"]] == [1, 1, 2]
    mask_ev = R.evaluate(g["images"], g["K"], s["area_rngs"], s["max_dets"], g["iou_thrs"], rule)
    with B.patched(0.02):
        bnd_ev = R.evaluate(g["images"], g["K"], s["area_rngs"], s["max_dets"], g["iou_thrs"], rule)
    assert R.compute_iou is B._MASK_IOU, "the patch must not outlive its block"
    differ = 0
    for a, b in zip(mask_ev, bnd_ev):
        assert (a is None) == (b is None)
        if a is not None:
            assert a["dtIds"] == b["dtIds"]
            differ += int(np.count_nonzero((a["dtMatches"] != 0) != (b["dtMatches"] != 0)))
    n = len(g["images"])
    ap_mask = R.summarize(R.accumulate(mask_ev, g["K"], n, s["area_rngs"], s["max_dets"], g["iou_thrs"]), s["max_dets"], g["iou_thrs"])[0]
    ap_bnd = R.summarize(R.accumulate(bnd_ev, g["K"], n, s["area_rngs"], s["max_dets"], g["iou_thrs"]), s["max_dets"], g["iou_thrs"])[0]
    print(f"{rule}: {differ} dtMatches bits differ, AP {ap_mask:.4f} (mask) -> {ap_bnd:.4f} (boundary)")
    assert differ > 0 and ap_bnd < ap_mask, "a mask-only implementation would pass the device comparison"
    # the figures this restatement gave when the feature was specified
    assert differ == {"coco": 292, "union": 168}[rule]
    assert round(float(ap_bnd), 4) == 0.1522 and round(float(ap_mask), 4) == {"coco": 0.4817, "union": 0.4773}[rule]
    # a boundary IoU never raises a pair's IoU
    dts, gts = g["images"][2]
    k = gts[0]["category"]
    dk, gk = [x for x in dts if x["category"] == k], [x for x in gts if x["category"] == k]
    assert (B.compute_iou(0.02)(dk, gk, 100, rule) <= R.compute_iou(dk, gk, 100, rule)).all()


# ---- the C entry points -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib


def test_boundary_symbols_declared_exported_and_bound(built):
    src = open(os.path.join(ROOT, "include", "mpformer_hip.h")).read()
    assert "boundary-iou-api" in src and "tools/evaluate_coco_boundary_ap.py" in src
    assert re.search(r"out MUST NOT alias", src)
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(raw, name) and name in built.SIGNATURES, name
    assert os.path.exists(os.path.join(ROOT, "mp_former_amd", "csrc", "seg_boundary.hip"))
    assert "seg_boundary.hip" in open(os.path.join(ROOT, "mp_former_amd", "csrc", "Makefile")).read()
    assert built.lib().mpf_abi_version() == 1


def test_boundary_entry_points_reject_bad_arguments(built):
    lib = built.lib()
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20)       # never dereferenced: the checks come first

    def bnd(bits=one, M=2, H=7, W=9, d=1, out=two):
        return lib.mpf_seg_mask_boundary(bits, M, H, W, d, out, None)
    assert bnd(bits=None) == -3 and bnd(out=None) == -3 and b"NULL" in lib.mpf_last_error()
    assert bnd(M=-1) == -2 and bnd(H=0) == -2 and bnd(W=-3) == -2 and bnd(d=0) == -2 and bnd(d=-5) == -2
    assert bnd(H=1 << 16, W=1 << 15) == -4 and bnd(M=70000) == -4
    assert bnd(M=0, bits=None, out=None) == 0                                      # nothing to do, nothing launched

    def match(inter=one, ad=one, ag=one, ib=one, adb=one, agb=one, D=3, G=2, sc=one, dc=one, gc=one, gcr=one, ga=one, thr=one, Tn=10,
              rng=one, A=4, K=5, md=100, rule=0, image=0, rec=one, npig=one, ws=one, nbytes=1 << 20):
        return lib.mpf_seg_ap_match_boundary(inter, ad, ag, ib, adb, agb, D, G, sc, dc, gc, gcr, ga, thr, Tn, rng, A, K, md, rule, image,
                                             rec, npig, ws, nbytes, None)
    for k in ("inter", "ad", "ag", "ib", "adb", "agb", "sc", "dc", "gc", "gcr", "ga", "thr", "rng", "rec", "npig", "ws"):
        assert match(**{k: None}) == -3, k
    assert match(ib=None) == -3 and b"boundary" in lib.mpf_last_error()
    assert match(D=-1) == -2 and match(G=-1) == -2 and match(K=0) == -2 and match(A=0) == -2 and match(Tn=0) == -2 and match(md=0) == -2
    assert match(image=-1) == -2 and match(rule=2) == -2 and match(rule=-1) == -2
    assert match(A=7, Tn=10) == -2 and b"64" in lib.mpf_last_error()
    assert match(A=65, Tn=1) == -2 and match(nbytes=79) == -2 and b"workspace" in lib.mpf_last_error()
    assert match(D=1 << 16, G=1 << 16) == -4
    assert match(D=0, G=0, inter=None, ad=None, ag=None, ib=None, adb=None, agb=None, sc=None, dc=None, gc=None, gcr=None, ga=None,
                 rec=None, ws=None, nbytes=0) == 0


# ---- the python side ----------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise():
    from mp_former_amd.inference import InstanceAP, mask_boundaries
    words = torch.zeros(2, 1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        mask_boundaries(words, (7, 9))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        InstanceAP(3, iou_type="boundary").update(words, [0.5, 0.4], [0, 1], words, [0, 1], [0, 0], size=(7, 9))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        InstanceAP(3, iou_type="boundary", device="cpu").update(words, [0.5, 0.4], [0, 1], words, [0, 1], [0, 0], size=(7, 9))


def test_option_and_shape_checks_come_before_any_launch():
    from mp_former_amd.inference import InstanceAP, mask_boundaries
    with pytest.raises(ValueError, match="iou_type"):
        InstanceAP(3, iou_type="dice")
    ap = InstanceAP(3, iou_type="boundary", dilation_ratio=0.05)
    assert ap.iou_type == "boundary" and ap.dilation_ratio == 0.05 and InstanceAP(3).iou_type == "segm"
    w = lambda *s, dt=torch.int64: _FakeCuda(torch.zeros(*s, dtype=dt))        # noqa: E731
    with pytest.raises(ValueError, match="size"):
        ap.update(w(2, 1), [0.5, 0.4], [0, 1], w(1, 1), [0], [0])               # boundary without size
    with pytest.raises(ValueError, match="does not fit"):
        ap.update(w(2, 1), [0.5, 0.4], [0, 1], w(1, 1), [0], [0], size=(9, 9))  # 81 pixels are two words
    with pytest.raises(ValueError, match="not one image"):
        ap.update(w(2, 3), [0.5, 0.4], [0, 1], w(1, 4), [0], [0], size=(7, 9))
    assert ap._npig is None and ap._images == 0, "nothing was launched or recorded"
    with pytest.raises(ValueError, match="int64"):
        mask_boundaries(w(2, 1, dt=torch.int32), (7, 9))
    with pytest.raises(ValueError, match="int64"):
        mask_boundaries(w(6), (7, 9))
    with pytest.raises(ValueError, match="does not fit"):
        mask_boundaries(w(2, 1), (9, 9))
    with pytest.raises(ValueError, match="does not fit"):
        mask_boundaries(w(2, 1), (0, 9))
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        mask_boundaries(w(2, 1), None)
    with pytest.raises(ValueError, match="at least 1"):
        mask_boundaries(w(2, 1), (7, 9), d=0)


def test_evaluator_with_both_types():
    from mp_former_amd import d2_plugin
    keys = {"AP", "AP50", "AP75", "APs", "APm", "APl", "AP-a", "AP-b", "AP-c"}
    default = d2_plugin.InstanceAPEvaluator(3, class_names=["a", "b", "c"])
    out = default.evaluate()
    assert set(out) == {"segm"} and set(out["segm"]) == keys and default.ap.iou_type == "segm" and list(default.aps) == ["segm"]
    ev = d2_plugin.InstanceAPEvaluator(3, class_names=["a", "b", "c"], iou_types=("segm", "boundary"), dilation_ratio=0.1, crowd_rule="union")
    assert ev.aps["boundary"].iou_type == "boundary" and ev.aps["boundary"].dilation_ratio == 0.1 and ev.aps["segm"].crowd_rule == "union"
    ev.reset()
    out = ev.evaluate()                                          # before any image
    assert list(out) == ["segm", "boundary"]
    for t in out:
        assert set(out[t]) == keys and all(np.isnan(v) for v in out[t].values())
    only = d2_plugin.InstanceAPEvaluator(3, iou_types=("boundary",))
    assert set(only.evaluate()) == {"boundary"} and only.ap is only.aps["boundary"]
    for bad in ((), ("segm", "segm"), ("dice",)):
        with pytest.raises(ValueError):
            d2_plugin.InstanceAPEvaluator(3, iou_types=bad)
