"""CPU: instance boxes and box AP without a GPU — the two new C entry points' declarations and argument checks, the restatement of
pycocotools' bbIou (tests/_box_restate.py) against a hand-computed table, ``boxes_of`` on hand-made masks, and the host-side checks
of ``mask_boxes``, ``InstanceAP(iou_type="bbox")``, ``InferenceConfig.instance_boxes`` and ``d2_plugin``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _box_restate as X
from test_ap_cpu import _FakeCuda

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mpf_seg_bits_boxes", "mpf_seg_ap_match_box")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib


# ---- the C entry points -------------------------------------------------------------------------------------------------------------
def test_box_symbols_declared_exported_and_bound(built):
    src = open(os.path.join(ROOT, "include", "mpformer_hip.h")).read()
    assert "maskformer_model.py:393-395" in src and "bbIou" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(raw, name) and name in built.SIGNATURES, name
    assert os.path.exists(os.path.join(ROOT, "mp_former_amd", "csrc", "seg_box.hip"))
    assert "seg_box.hip" in open(os.path.join(ROOT, "mp_former_amd", "csrc", "Makefile")).read()
    assert built.lib().mpf_abi_version() == 1


def test_box_entry_points_reject_bad_arguments(built):
    lib = built.lib()
    one = ctypes.c_void_p(16)       # never dereferenced: the checks come first

    def boxes(bits=one, M=2, H=7, W=9, out=one):
        return lib.mpf_seg_bits_boxes(bits, M, H, W, out, None)
    assert boxes(bits=None) == -3 and b"NULL" in lib.mpf_last_error() and boxes(out=None) == -3
    assert boxes(M=-1) == -2 and boxes(H=0) == -2 and boxes(H=-7) == -2 and boxes(W=0) == -2
    assert boxes(H=1 << 16, W=1 << 15) == -4 and boxes(M=70000) == -4
    assert boxes(M=0, bits=None, out=None) == 0                                    # nothing to do, nothing launched

    def match(db=one, gb=one, D=3, G=2, sc=one, dc=one, gc=one, gcr=one, ga=one, thr=one, Tn=10, rng=one, A=4, K=5, md=100, rule=0,
              image=0, rec=one, npig=one, ws=one, nbytes=1 << 20):
        return lib.mpf_seg_ap_match_box(db, gb, D, G, sc, dc, gc, gcr, ga, thr, Tn, rng, A, K, md, rule, image, rec, npig, ws, nbytes, None)
    for k in ("db", "gb", "sc", "dc", "gc", "gcr", "ga", "thr", "rng", "rec", "npig", "ws"):
        assert match(**{k: None}) == -3, k
    assert match(D=-1) == -2 and match(G=-1) == -2 and match(K=0) == -2 and match(A=0) == -2 and match(Tn=0) == -2 and match(md=0) == -2
    assert match(image=-1) == -2 and match(rule=2) == -2 and match(rule=-1) == -2
    assert match(A=7, Tn=10) == -2 and b"64" in lib.mpf_last_error()               # A * Tn > 64: the record format holds 64 settings
    assert match(A=65, Tn=1) == -2
    assert match(nbytes=79) == -2 and b"workspace" in lib.mpf_last_error()         # 4 * 10 * 2 = 80 bytes are needed
    assert match(D=1 << 16, G=1 << 16) == -4
    # one side empty: its box pointer may be NULL; both empty: nothing launched
    assert match(D=0, db=None, sc=None, dc=None, rec=None, G=0, gb=None, gc=None, gcr=None, ga=None, ws=None, nbytes=0) == 0


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def test_bb_iou_agrees_with_a_hand_computed_table():
    dt = [[0, 0, 4, 4], [2, 0, 2, 4], [10, 10, 1, 1], [1.5, 2.25, 2.0, 0.5]]
    gt = [[0, 0, 2, 4], [2, 0, 2, 4], [4, 0, 3, 3], [1.0, 2.0, 4.0, 1.0]]
    # rows: detections; plain union.  (0,0): 8 / (16 + 8 - 8); (0,2): touching edges, w = 0; (3,3): 1 / (1 + 4 - 1), the detection
    # inside; (3,0): w = 2 - 1.5 = .5, h = .5 -> .25 / (1 + 8 - .25); (3,1): w = 3.5 - 2 = 1.5 -> .75 / (1 + 8 - .75);
    # (0,3): w = 3, h = 1 -> 3 / (16 + 4 - 3); (1,3): w = 2, h = 1 -> 2 / (8 + 4 - 2)
    union = [[8 / 16, 8 / 16, 0.0, 3 / 17],
             [0.0, 1.0, 0.0, 2 / 10],
             [0.0, 0.0, 0.0, 0.0],
             [0.25 / 8.75, 0.75 / 8.25, 0.0, 1 / 4]]
    np.testing.assert_array_equal(X.bb_iou(dt, gt, [0, 0, 0, 0], "union"), np.array(union))
    np.testing.assert_array_equal(X.bb_iou(dt, gt, [0, 0, 0, 0], "coco"), np.array(union))
    np.testing.assert_array_equal(X.bb_iou(dt, gt, [1, 1, 1, 1], "union"), np.array(union))     # "union": a crowd changes nothing
    # "coco": a crowd ground truth divides by the detection's own area
    crowd = X.bb_iou(dt, gt, [1, 0, 0, 1], "coco")
    np.testing.assert_array_equal(crowd[:, 0], [8 / 16, 0.0, 0.0, 0.25 / 1.0])
    np.testing.assert_array_equal(crowd[:, 3], [3 / 16, 2 / 8, 0.0, 1.0])
    np.testing.assert_array_equal(crowd[:, 1:3], np.array(union)[:, 1:3])
    assert X.bb_iou(np.zeros((0, 4)), gt, [0] * 4, "coco").shape == (0, 4) and X.bb_iou(dt, np.zeros((0, 4)), [], "coco").shape == (4, 0)
    with pytest.raises(ValueError):
        X.bb_iou(dt, gt, [0] * 4, "dice")


def test_contraction_pairs_tell_fused_arithmetic_from_the_restatement():
    """the scene of tests/test_box_ap_gpu.py: at (pair k, threshold k) exactly one of the two arithmetics reaches the threshold"""
    dts, gts, thrs = X.contraction_scene()
    assert len(thrs) == 10 and ((thrs > 0.3) & (thrs < 1 - 1e-10)).all()
    lower = 0
    for k, (d, g) in enumerate(X.CONTRACTION_PAIRS):
        a, b = float(X.bb_iou([d], [g], [0], "union")[0, 0]), X.bb_iou_contracted(d, g)
        assert a != b and abs(a - b) <= 2 * np.spacing(a), k
        assert (a >= thrs[k]) != (b >= thrs[k]), k
        lower += int(a < b)
    assert 0 < lower < 10, "both directions: a match the contracted code misses, and one it makes wrongly"
    # on exact inputs the two agree
    assert X.bb_iou_contracted([0, 0, 4, 4], [0, 0, 2, 4]) == 0.5 and X.bb_iou_contracted([0, 0, 1, 1], [1, 0, 1, 1]) == 0.0


def test_boxes_of_hand_made_masks():
    m = np.zeros((4, 5, 7), dtype=bool)
    m[1, 2, 3] = True                                    # one pixel at y = 2, x = 3
    m[2, 1:4, 0] = True
    m[2, 4, 6] = True
    m[3] = True
    assert X.boxes_of(m).tolist() == [[0, 0, 0, 0], [3, 2, 4, 3], [0, 1, 7, 5], [0, 0, 7, 5]]
    assert X.boxes_of(m).dtype == np.int32
    assert X.xyxy_to_xywh([[3, 2, 4, 3], [0, 1, 7, 5]]).tolist() == [[3.0, 2.0, 1.0, 1.0], [0.0, 1.0, 7.0, 4.0]]


# ---- the python side ----------------------------------------------------------------------------------------------------------------
def test_cpu_tensors_raise():
    from mp_former_amd.inference import InstanceAP, mask_boxes
    words = torch.zeros(2, 1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        mask_boxes(words, (7, 9))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        mask_boxes(words.view(1, 2, 1), (7, 9))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        InstanceAP(3, iou_type="bbox").update(words, [0.5, 0.4], [0, 1], words, [0, 1], [0, 0], size=(7, 9))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        InstanceAP(3, iou_type="bbox", device="cpu").update(None, [0.5], [0], None, [0], [0], dt_boxes=[[0, 0, 1, 1]], gt_boxes=[[0, 0, 1, 1]])


def test_option_and_shape_checks_come_before_any_launch():
    from mp_former_amd.inference import AP_IOU_TYPES, InferenceConfig, InstanceAP, TubeAP, boxes_xyxy_to_xywh, mask_boxes
    assert AP_IOU_TYPES == ("segm", "boundary", "bbox")
    assert InferenceConfig(num_classes=3).instance_boxes is False and InferenceConfig(num_classes=3, instance_boxes=True).instance_boxes
    with pytest.raises(ValueError, match="tubes"):
        InstanceAP(3, iou_type="bbox", tubes=True)
    with pytest.raises(ValueError, match="tubes"):
        TubeAP(3, iou_type="bbox")
    ap = InstanceAP(3, iou_type="bbox")
    assert ap.iou_type == "bbox" and ap.crowd_rule == "coco"
    w = lambda *s, dt=torch.int64: _FakeCuda(torch.zeros(*s, dtype=dt))        # noqa: E731
    with pytest.raises(ValueError, match="size"):
        ap.update(w(2, 1), [0.5, 0.4], [0, 1], w(1, 1), [0], [0])               # boxes from bits need the size
    with pytest.raises(ValueError, match="does not fit"):
        ap.update(w(2, 1), [0.5, 0.4], [0, 1], w(1, 1), [0], [0], size=(9, 9))
    with pytest.raises(ValueError, match="gt_boxes or gt_bits"):
        ap.update(None, [0.5], [0], None, [0], [0], dt_boxes=[[0, 0, 1, 1]])
    with pytest.raises(ValueError, match="frame areas"):
        ap.update(None, [0.5], [0], None, [0], [0], dt_boxes=[[0, 0, 1, 1]], gt_boxes=[[0, 0, 1, 1]], dt_frame_area=w(1, 1))
    with pytest.raises(ValueError, match="bbox"):
        InstanceAP(3).update(w(2, 1), [0.5, 0.4], [0, 1], w(1, 1), [0], [0], gt_boxes=[[0, 0, 1, 1]])
    assert ap._npig is None and ap._images == 0, "nothing was launched or recorded"
    with pytest.raises(ValueError, match="int64"):
        mask_boxes(w(2, 1, dt=torch.int32), (7, 9))
    with pytest.raises(ValueError, match="int64"):
        mask_boxes(w(6), (7, 9))
    with pytest.raises(ValueError, match="does not fit"):
        mask_boxes(w(2, 1), (9, 9))
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        mask_boxes(w(2, 1), None)
    got = boxes_xyxy_to_xywh(torch.tensor([[3, 2, 4, 3], [0, 1, 7, 5]], dtype=torch.int32))
    assert got.dtype == torch.float64 and got.tolist() == [[3.0, 2.0, 1.0, 1.0], [0.0, 1.0, 7.0, 4.0]]
    assert boxes_xyxy_to_xywh(torch.tensor([[0.5, 0.25, 2.0, 1.0]])).tolist() == [[0.5, 0.25, 1.5, 0.75]]
    assert tuple(boxes_xyxy_to_xywh(torch.zeros(0, 4)).shape) == (0, 4)


def test_evaluator_and_install_take_the_new_type_and_option():
    import inspect
    from mp_former_amd import d2_plugin
    keys = {"AP", "AP50", "AP75", "APs", "APm", "APl", "AP-a", "AP-b", "AP-c"}
    ev = d2_plugin.InstanceAPEvaluator(3, class_names=["a", "b", "c"], iou_types=("bbox", "segm"), crowd_rule="union")
    assert list(ev.aps) == ["bbox", "segm"] and ev.ap is ev.aps["bbox"] and ev.aps["bbox"].iou_type == "bbox"
    assert ev.aps["bbox"].crowd_rule == "union"
    ev.reset()
    out = ev.evaluate()                                          # before any image
    assert list(out) == ["bbox", "segm"]
    for t in out:
        assert set(out[t]) == keys and all(np.isnan(v) for v in out[t].values())
    assert set(d2_plugin.InstanceAPEvaluator(3).evaluate()) == {"segm"}, "the default is unchanged"
    sig = inspect.signature(d2_plugin.install_native_inference)
    assert sig.parameters["instance_boxes"].default is False
    assert "detectron2" not in inspect.getsource(d2_plugin.InstanceAPEvaluator.process)
