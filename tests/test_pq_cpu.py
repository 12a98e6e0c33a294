"""CPU: panoptic quality without a GPU — the numpy restatement (tests/_pq_restate.py) against the golden made by the reference's
own ``pq_compute_single_image`` (tests/golden/make_golden_pq.py), the host arithmetic of ``pq_results`` / ``combine``, the C
entry points' argument checks and the host-side checks of ``PanopticQuality`` and ``d2_plugin.PanopticQualityEvaluator``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _pq_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pq_semantic.npz")
NEW_SYMBOLS = ("mpf_seg_pq_workspace_bytes", "mpf_seg_pq_pairs", "mpf_seg_pq_match")


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


def assert_stats_equal(got, want, tag=""):
    for k in ("tp", "fp", "fn"):
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(want[k]), err_msg=f"{tag} {k}")
    assert bits(got["iou"]) == bits(want["iou"]), f"{tag} iou {got['iou']} != {want['iou']}"


def load_golden():
    z = np.load(GOLDEN)
    K, ignore, n = int(z["num_classes"]), int(z["ignore_label"]), int(z["num_images"])
    images = []
    for i in range(n):
        images.append({"gt": z[f"gt_{i}"], "pred": z[f"pred_{i}"],
                       "single": {k: z[f"{k}_{i}"] for k in ("tp", "fp", "fn", "iou")},
                       "sum": {k: z[f"sum_{k}_{i}"] for k in ("tp", "fp", "fn", "iou")}})
    return K, ignore, images


# ---- the restatement against the reference's own function -------------------------------------------------------------------------
def test_restatement_reproduces_the_golden_bit_for_bit():
    K, ignore, images = load_golden()
    assert [im["gt"].shape for im in images] == [(37, 50), (33, 56), (61, 83)] and K == 6 and ignore == 255
    total = R.zero_stats(K)
    for n, im in enumerate(images):
        single = R.pq_single_semantic(im["gt"], im["pred"], K, ignore)
        total = R.add_stats(total, single)
        assert_stats_equal(single, im["single"], f"image {n}")
        assert_stats_equal(total, im["sum"], f"sum to {n}")
        assert im["single"]["tp"].dtype == np.int64 and im["single"]["iou"].dtype == np.float64
    last = images[-1]["sum"]
    assert last["tp"].sum() > 0 and last["fp"].sum() > 0 and last["fn"].sum() > 0
    assert 0.1 < np.mean([(im["gt"] == ignore).mean() for im in images]) < 0.2


def test_restatement_general_form_equals_the_semantic_form():
    """listed segments with ids that are not the categories, RGB round trip: the same counts as the semantic form"""
    K, ignore, images = load_golden()
    im = images[0]
    gt_ids = np.where(im["gt"] == ignore, 0, im["gt"] * 70000 + 5)          # ids above 65536, VOID = 0
    pred_ids = im["pred"] + 1
    gts = [{"id": int(c) * 70000 + 5, "category_id": int(c), "iscrowd": 0} for c in np.unique(im["gt"]) if c != ignore]
    preds = [{"id": int(c) + 1, "category_id": int(c)} for c in np.unique(im["pred"])]
    assert_stats_equal(R.pq_single(gt_ids, pred_ids, gts, preds, K, 0), im["single"])
    np.testing.assert_array_equal(R.rgb2id(R.id2rgb(gt_ids)), gt_ids)
    with pytest.raises(ValueError, match="not in segments_info"):
        R.pq_single(gt_ids, pred_ids, gts, preds[1:], K, 0)
    with pytest.raises(ValueError, match="not in the map"):
        R.pq_single(gt_ids, pred_ids, gts, preds + [{"id": 99, "category_id": 0}], K, 0)


# ---- pq_results / combine ---------------------------------------------------------------------------------------------------------
def test_pq_results_hand_computed():
    from mp_former_amd.inference import PanopticQuality, pq_results
    # K = 5, things = {0, 1, 4}.  class 0: plain; class 1: tp == 0 (sq = 0, still counted); class 2: no entries (left out of n);
    # class 3: stuff with all three; class 4: thing without entries
    stats = {"tp": np.array([2, 0, 0, 1, 0]), "fp": np.array([1, 2, 0, 0, 0]), "fn": np.array([1, 0, 0, 1, 0]),
             "iou": np.array([1.5, 0.0, 0.0, 0.75, 0.0])}
    r = pq_results(stats, {0, 1, 4})
    pc = r["per_class"]
    assert pc[0] == {"pq": 1.5 / 3.0, "sq": 0.75, "rq": 2 / 3.0}
    assert pc[1] == {"pq": 0.0, "sq": 0.0, "rq": 0.0}
    assert pc[2] == {"pq": 0.0, "sq": 0.0, "rq": 0.0} and pc[4] == pc[2]
    assert pc[3] == {"pq": 0.75 / 1.5, "sq": 0.75, "rq": 1 / 1.5}
    assert r["All"]["n"] == 3 and r["Things"]["n"] == 2 and r["Stuff"]["n"] == 1
    assert r["All"]["pq"] == (0.5 + 0.0 + 0.5) / 3 and r["All"]["sq"] == (0.75 + 0.0 + 0.75) / 3
    assert r["All"]["rq"] == (2 / 3.0 + 0.0 + 1 / 1.5) / 3
    assert r["Things"] == {"pq": 0.25, "sq": 0.375, "rq": (2 / 3.0) / 2, "n": 2}
    assert r["Stuff"] == {"pq": 0.5, "sq": 0.75, "rq": 1 / 1.5, "n": 1}
    # a group without any entry
    empty = pq_results({k: np.zeros(2, dtype=np.float64 if k == "iou" else np.int64) for k in ("tp", "fp", "fn", "iou")}, {0})
    assert empty["All"]["n"] == 0 and np.isnan(empty["All"]["pq"]) and np.isnan(empty["Things"]["rq"])
    # the nine keys, x 100, from an object that never saw an image only through pq_results
    q = PanopticQuality(5, {0, 1, 4})
    assert not any(q.stats()[k].any() for k in ("tp", "fp", "fn", "iou")) and q.stats()["iou"].dtype == np.float64
    assert set(q.results()) == {"PQ", "SQ", "RQ", "PQ_th", "SQ_th", "RQ_th", "PQ_st", "SQ_st", "RQ_st"}
    q.reset()


def test_combine_is_the_sum_in_list_order():
    from mp_former_amd.inference import PanopticQuality
    a = {"tp": np.array([1, 2]), "fp": np.array([0, 1]), "fn": np.array([3, 0]), "iou": np.array([0.1, 0.7])}
    b = {"tp": np.array([4, 0]), "fp": np.array([1, 1]), "fn": np.array([0, 0]), "iou": np.array([0.2, 0.6])}
    c = {"tp": np.array([0, 1]), "fp": np.array([0, 0]), "fn": np.array([1, 1]), "iou": np.array([0.3, 0.9])}
    s = PanopticQuality.combine([a, b, c])
    np.testing.assert_array_equal(s["tp"], [5, 3])
    np.testing.assert_array_equal(s["fp"], [1, 2])
    np.testing.assert_array_equal(s["fn"], [4, 1])
    assert s["tp"].dtype == np.int64 and s["iou"].dtype == np.float64
    assert bits(s["iou"]) == bits((a["iou"] + b["iou"]) + c["iou"])
    assert a["tp"].tolist() == [1, 2], "combine must not change its inputs"
    assert_stats_equal(PanopticQuality.combine([a]), a)
    with pytest.raises(ValueError):
        PanopticQuality.combine([])


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib


def test_pq_symbols_declared_exported_and_bound(built):
    src = open(os.path.join(ROOT, "include", "mpformer_hip.h")).read()
    assert "pq_compute_single_image" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(raw, name) and name in built.SIGNATURES, name
    assert os.path.exists(os.path.join(ROOT, "mp_former_amd", "csrc", "seg_pq.hip"))
    assert built.lib().mpf_abi_version() == 1


def test_pq_entry_points_reject_bad_arguments(built):
    lib = built.lib()
    one = ctypes.c_void_p(16)       # never dereferenced: the checks come first
    assert lib.mpf_seg_pq_workspace_bytes(3, 4) == 5 * 6 * 4 and lib.mpf_seg_pq_workspace_bytes(0, 0) == 16
    assert lib.mpf_seg_pq_workspace_bytes(-1, 4) == 0
    big = 1 << 20

    def pairs(pred=one, gt=one, fmt=0, n=100, gt_ids=None, G=3, gbase=1, pred_ids=None, S=4, pbase=1, table=one, nbytes=big):
        return lib.mpf_seg_pq_pairs(pred, gt, fmt, n, gt_ids, G, gbase, pred_ids, S, pbase, 0, table, nbytes, None)
    assert pairs(pred=None) == -3 and pairs(gt=None) == -3 and pairs(table=None) == -3
    assert pairs(n=0) == -2 and pairs(n=-5) == -2
    assert pairs(n=1 << 31) == -4
    assert pairs(G=-1) == -2 and pairs(S=-1) == -2
    assert pairs(fmt=2) == -1 and b"format" in lib.mpf_last_error()
    assert pairs(fmt=-1) == -1
    assert pairs(nbytes=5 * 6 * 4 - 1) == -2 and b"seg_pq_pairs" in lib.mpf_last_error()
    assert pairs(gt_ids=one, G=20000) == -4                     # the id table no longer fits beside nothing

    def match(table=one, nbytes=big, G=3, S=4, K=5, gt_cat=one, flags=one, pred_cat=one, implicit=0, tp=one, fp=one, fn=one, iou=one,
              err=one):
        return lib.mpf_seg_pq_match(table, nbytes, G, S, K, gt_cat, flags, pred_cat, implicit, tp, fp, fn, iou, err, None)
    for k in ("table", "tp", "fp", "fn", "iou", "err", "gt_cat", "pred_cat"):
        assert match(**{k: None}) == -3, k
    assert match(G=-1) == -2 and match(S=-1) == -2 and match(K=0) == -2 and match(K=-3) == -2
    assert match(implicit=2) == -2
    assert match(implicit=1) == -2 and b"implicit" in lib.mpf_last_error()         # G == S == K and no tables
    assert match(nbytes=8) == -2
    assert match(K=1 << 20) == -4


# ---- host-side checks of the class and the evaluator -----------------------------------------------------------------------------
def test_panoptic_quality_rejects_cpu_tensors_and_bad_segments():
    from mp_former_amd.inference import PanopticQuality, _pq_side
    q = PanopticQuality(4, {0, 1}, device="cuda:0")
    ids = torch.zeros(4, 5, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        q.update(ids, [], ids, [])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        q.update_semantic(ids, ids)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        PanopticQuality(4, {0}, device="cpu").update(ids, [], ids, [])
    with pytest.raises(ValueError):
        PanopticQuality(0, ())
    with pytest.raises(ValueError, match="outside"):
        _pq_side([{"id": 1, "category_id": 4}], 4, 0, "segments_info")
    with pytest.raises(ValueError, match="outside"):
        _pq_side([{"id": 1, "category_id": -1}], 4, 0, "segments_info")
    with pytest.raises(ValueError, match="duplicate"):
        _pq_side([{"id": 7, "category_id": 1}, {"id": 7, "category_id": 2}], 4, 0, "gt_segments")
    with pytest.raises(ValueError, match="void"):
        _pq_side([{"id": 0, "category_id": 1}], 4, 0, "gt_segments")
    # sorted by id; the LAST crowd segment of a category in the annotation's order wins, whatever its id
    segs = [{"id": 90, "category_id": 2, "iscrowd": 1}, {"id": 5, "category_id": 1, "iscrowd": 0},
            {"id": 40, "category_id": 2, "iscrowd": 1}, {"id": 70000, "category_id": 3, "iscrowd": 1}]
    i, c, f = _pq_side(segs, 4, 0, "gt_segments", crowd=True)
    assert i.tolist() == [5, 40, 90, 70000] and c.tolist() == [1, 2, 2, 3] and f.tolist() == [0, 3, 1, 3]
    assert i.dtype == c.dtype == f.dtype == np.int32
    assert _pq_side(segs, 4, 0, "segments_info")[2].tolist() == [0, 0, 0, 0]


class _FakeCuda:
    """a tensor stand-in that passes for a device tensor up to the shape checks"""

    def __init__(self, t):
        self.t, self.is_cuda, self.dtype, self.shape, self.device = t, True, t.dtype, t.shape, torch.device("cuda:0")

    def dim(self):
        return self.t.dim()

    def numel(self):
        return self.t.numel()


def test_panoptic_quality_shape_checks_come_before_any_launch():
    from mp_former_amd.inference import PanopticQuality
    q = PanopticQuality(4, {0, 1}, device="cuda:0")
    i32 = lambda *s: _FakeCuda(torch.zeros(*s, dtype=torch.int32))     # noqa: E731
    with pytest.raises(ValueError, match="same"):
        q.update(i32(4, 5), [], i32(4, 6), [])
    with pytest.raises(ValueError, match="same"):
        q.update(i32(4, 5), [], _FakeCuda(torch.zeros(5, 4, 3, dtype=torch.uint8)), [])
    with pytest.raises(ValueError, match="RGB"):
        q.update(i32(4, 5), [], _FakeCuda(torch.zeros(4, 5, 4, dtype=torch.uint8)), [])
    with pytest.raises(ValueError, match="int32"):
        q.update(_FakeCuda(torch.zeros(4, 5, dtype=torch.int64)), [], i32(4, 5), [])
    with pytest.raises(ValueError, match="int32"):
        q.update(i32(4, 5), [], _FakeCuda(torch.zeros(4, 5, dtype=torch.int64)), [])
    with pytest.raises(ValueError, match="outside"):
        q.update(i32(4, 5), [{"id": 1, "category_id": 9}], i32(4, 5), [])
    with pytest.raises(ValueError, match="duplicate"):
        q.update(i32(4, 5), [], i32(4, 5), [{"id": 3, "category_id": 1, "iscrowd": 0}, {"id": 3, "category_id": 1, "iscrowd": 0}])
    with pytest.raises(ValueError, match="same"):
        q.update_semantic(i32(4, 5), i32(5, 4))
    with pytest.raises(ValueError, match="integer"):
        q.update_semantic(i32(4, 5), _FakeCuda(torch.zeros(4, 5)))


def test_evaluator_construction_and_id_mapping():
    from mp_former_amd import d2_plugin
    calls = []

    def read_png(path):
        calls.append(path)
        return np.zeros((4, 5, 3), dtype=np.uint8)
    ev = d2_plugin.PanopticQualityEvaluator(3, {0}, {1: 0, 7: 1, 92: 2}, read_png=read_png)
    assert ev.pq.num_classes == 3 and ev.pq.thing_ids == frozenset({0}) and ev.read_png is read_png
    ev.reset()
    got = ev.gt_segments([{"id": 300, "category_id": 92, "iscrowd": 1, "area": 10}, {"id": 8, "category_id": 1}])
    assert got == [{"id": 300, "category_id": 2, "iscrowd": 1}, {"id": 8, "category_id": 0, "iscrowd": 0}]
    with pytest.raises(ValueError, match="mapping"):
        ev.gt_segments([{"id": 1, "category_id": 5}])
    out = ev.evaluate()                                          # before any image: every group is empty
    assert set(out) == {"panoptic_seg"} and len(out["panoptic_seg"]) == 9 and np.isnan(out["panoptic_seg"]["PQ"])
    assert d2_plugin.PanopticQualityEvaluator(3, {0}, {}).read_png is d2_plugin._read_png_rgb
    assert not calls
    for name in ("reset", "process", "evaluate"):
        assert callable(getattr(ev, name))


def test_default_png_reader_returns_rgb_bytes(tmp_path):
    from PIL import Image
    from mp_former_amd import d2_plugin
    ids = np.array([[0, 5, 70000], [255, 256, 16777215]], dtype=np.int64)
    path = str(tmp_path / "pan.png")
    Image.fromarray(R.id2rgb(ids)).save(path)
    rgb = d2_plugin._read_png_rgb(path)
    assert rgb.dtype == np.uint8 and rgb.shape == (2, 3, 3)
    np.testing.assert_array_equal(R.rgb2id(rgb), ids)
