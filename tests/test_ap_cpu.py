"""CPU: instance mask AP without a GPU — the numpy restatement (tests/_ap_restate.py) against the golden made by the reference's own
``evaluate`` / ``accumulate`` / ``summarize`` (tests/golden/make_golden_ap.py), the host arithmetic of ``InstanceAP`` (accumulate,
summarize, results, combine) on the golden's records, the C entry points' argument checks and the host-side checks of the module
and of ``d2_plugin.InstanceAPEvaluator``."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _ap_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ap_instances.npz")
NEW_SYMBOLS = ("mpf_seg_instance_bits", "mpf_seg_pack_masks", "mpf_seg_mask_pairs", "mpf_seg_ap_workspace_bytes", "mpf_seg_ap_match")
RULES = ("union", "coco")
SETTINGS = ("coco", "small")


def bits(a):
    return np.asarray(a, dtype=np.float64).tobytes()


_golden = None


def load_golden():
    """-> {"K", "sizes", "images": [(dts, gts)], "iou_thrs", "rec_thrs", settings and results by name}; read once, never changed"""
    global _golden
    if _golden is not None:
        return _golden
    z = np.load(GOLDEN)
    sizes = [tuple(int(v) for v in s) for s in z["sizes"]]

    def masks(packed, image):
        flat = np.unpackbits(packed)
        out, at = [], 0
        for i in image:
            H, W = sizes[int(i)]
            out.append(flat[at:at + H * W].reshape(H, W).astype(bool))
            at += H * W
        return out
    gm, dm = masks(z["gt_masks"], z["gt_image"]), masks(z["dt_masks"], z["dt_image"])
    images = [([], []) for _ in sizes]
    for n, m in enumerate(dm):
        images[int(z["dt_image"][n])][0].append({"id": int(z["dt_id"][n]), "category": int(z["dt_category"][n]), "mask": m,
                                                 "score": float(z["dt_score"][n]), "area": float(z["dt_area"][n])})
    for n, m in enumerate(gm):
        images[int(z["gt_image"][n])][1].append({"id": int(z["gt_id"][n]), "category": int(z["gt_category"][n]), "mask": m,
                                                 "area": float(z["gt_area"][n]), "iscrowd": int(z["gt_crowd"][n])})
    g = {"K": int(z["num_classes"]), "sizes": sizes, "images": images, "iou_thrs": z["iou_thrs"], "rec_thrs": z["rec_thrs"]}
    for name in SETTINGS:
        g[name] = {"area_rngs": z[f"{name}_area_rngs"].tolist(), "max_dets": [int(m) for m in z[f"{name}_max_dets"]]}
        for rule in RULES:
            g[rule, name] = {k: z[f"{rule}_{name}_{k}"] for k in ("table", "dtm", "dtig", "gtig", "dtids", "gtids", "precision", "recall",
                                                                   "scores", "stats")}
    _golden = g
    return g


def golden_eval_imgs(g, rule, name):
    """the golden's flat arrays back as the evalImgs list (dtMatches as booleans)"""
    z, T = g[rule, name], len(g["iou_thrs"])
    out, d_at, g_at, m_at = [], 0, 0, 0
    for D, G, exists in z["table"]:
        if not exists:
            out.append(None)
            continue
        D, G = int(D), int(G)
        out.append({"dtIds": z["dtids"][d_at:d_at + D].tolist(), "gtIds": z["gtids"][g_at:g_at + G].tolist(),
                    "dtMatches": z["dtm"][m_at:m_at + T * D].reshape(T, D), "dtIgnore": z["dtig"][m_at:m_at + T * D].reshape(T, D),
                    "gtIgnore": z["gtig"][g_at:g_at + G].astype(np.int64)})
        d_at, g_at, m_at = d_at + D, g_at + G, m_at + T * D
    assert d_at == len(z["dtids"]) and g_at == len(z["gtids"]) and m_at == len(z["dtm"])
    return out


def golden_stats(g, rule, name, images=None):
    """the golden's records in the form ``InstanceAP.stats`` returns (through the restatement's bookkeeping only)"""
    s = g[name]
    sel = list(range(len(g["images"]))) if images is None else list(images)
    ev = golden_eval_imgs(g, rule, name)
    n, A = len(g["images"]), len(s["area_rngs"])
    ev = [ev[(k * A + a) * n + i] for k in range(g["K"]) for a in range(A) for i in sel]
    return R.expected_stats([g["images"][i] for i in sel], g["K"], s["area_rngs"], s["max_dets"], g["iou_thrs"], rule, eval_imgs=ev)


def assert_stats_equal(got, want, tag=""):
    assert np.asarray(got["scores"], dtype=np.float32).tobytes() == np.asarray(want["scores"], dtype=np.float32).tobytes(), f"{tag} scores"
    for k in ("category", "rank", "image", "matched", "ignored", "npig"):
        np.testing.assert_array_equal(np.asarray(got[k]), np.asarray(want[k]), err_msg=f"{tag} {k}")
    assert np.asarray(got["matched"]).dtype == bool and np.asarray(got["npig"]).dtype == np.int64


# ---- the restatement against the reference's own code --------------------------------------------------------------------------------
def test_golden_is_what_the_issue_asks_for():
    g = load_golden()
    assert g["sizes"] == [(37, 50), (33, 56), (61, 83)] and g["K"] == 4
    assert all(H % 2 == 1 and (H * W) % 64 for H, W in g["sizes"])
    assert g["iou_thrs"].tobytes() == np.linspace(.5, .95, 10).tobytes() and g["rec_thrs"].tobytes() == np.linspace(0, 1, 101).tobytes()
    assert g["coco"]["area_rngs"] == [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]] and g["coco"]["max_dets"] == [1, 10, 100]
    assert g["small"]["max_dets"] == [1, 3, 5]
    cats_gt = {x["category"] for _, gts in g["images"] for x in gts}
    cats_dt = {x["category"] for dts, _ in g["images"] for x in dts}
    assert cats_gt == {0, 1, 3} and cats_dt == {0, 1, 2}
    assert os.path.getsize(GOLDEN) < 64 * 1024


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", SETTINGS)
def test_restatement_reproduces_the_golden_bit_for_bit(rule, name):
    g = load_golden()
    s, want = g[name], golden_eval_imgs(g, rule, name)
    got = R.evaluate(g["images"], g["K"], s["area_rngs"], s["max_dets"], g["iou_thrs"], rule)
    assert len(got) == len(want) == g["K"] * 4 * 3
    for n, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), n
        if a is None:
            continue
        assert a["dtIds"] == b["dtIds"] and a["gtIds"] == b["gtIds"], n
        np.testing.assert_array_equal(a["dtMatches"] != 0, b["dtMatches"], err_msg=f"entry {n} dtMatches")
        np.testing.assert_array_equal(np.asarray(a["dtIgnore"]).astype(bool), b["dtIgnore"], err_msg=f"entry {n} dtIgnore")
        np.testing.assert_array_equal(a["gtIgnore"], b["gtIgnore"], err_msg=f"entry {n} gtIgnore")
    acc = R.accumulate(got, g["K"], len(g["images"]), s["area_rngs"], s["max_dets"], g["iou_thrs"], g["rec_thrs"])
    z = g[rule, name]
    for k in ("precision", "recall", "scores"):
        assert acc[k].shape == z[k].shape and bits(acc[k]) == bits(z[k]), k
    assert (z["precision"] == -1).any() and (z["precision"] > 0).any()
    assert bits(R.summarize(acc, s["max_dets"], g["iou_thrs"])) == bits(z["stats"])


def test_the_two_crowd_rules_differ_in_the_golden():
    g = load_golden()
    assert not np.array_equal(g["union", "coco"]["dtm"], g["coco", "coco"]["dtm"])
    assert bits(g["union", "coco"]["stats"]) != bits(g["coco", "coco"]["stats"])


def test_each_fraction_matches_at_its_own_threshold():
    """1/2, 11/20, ..., 19/20 as mask IoUs match at the threshold of the same index: this pins the threshold bits (np.linspace, not
    0.5 + 0.05 i) and the correctly rounded quotient"""
    rebuilt_fails = 0
    for i in range(10):
        num = 10 + i
        gt = np.zeros((4, 5), dtype=bool)
        gt.reshape(-1)[:20] = True
        dt = np.zeros((4, 5), dtype=bool)
        dt.reshape(-1)[:num] = True
        dts = [{"id": 1, "category": 0, "score": 0.5, "mask": dt, "area": float(num)}]
        gts = [{"id": 1, "category": 0, "mask": gt, "area": 20.0, "iscrowd": 0}]
        for rule in RULES:
            e = R.evaluate_image(dts, gts, [0, 1e10], 100, R.IOU_THRS, rule)
            m = e["dtMatches"][:, 0] != 0
            assert m[:i + 1].all() and not m[i + 1:].any(), (i, rule, m)
        rebuilt_fails += not (num / 20 >= 0.5 + 0.05 * i)
    assert rebuilt_fails >= 1, "thresholds rebuilt as 0.5 + 0.05 i would have lost a match: the test pins something"


# ---- InstanceAP's host arithmetic on the golden's records -----------------------------------------------------------------------------
def _ap(g, rule, name):
    from mp_former_amd.inference import InstanceAP
    s = g[name]
    return InstanceAP(g["K"], area_rngs=s["area_rngs"], max_dets=s["max_dets"], crowd_rule=rule)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("name", SETTINGS)
def test_accumulate_summarize_results_equal_the_golden(rule, name):
    g = load_golden()
    ap, z = _ap(g, rule, name), g[rule, name]
    stats = golden_stats(g, rule, name)
    assert len(stats["scores"]) == sum(len(d) for d, _ in g["images"])
    acc = ap.accumulate(stats)
    for k in ("precision", "recall", "scores"):
        assert acc[k].dtype == np.float64 and acc[k].shape == z[k].shape and bits(acc[k]) == bits(z[k]), k
    assert bits(ap.summarize(stats)) == bits(z["stats"])
    res = ap.results(stats=stats)
    st = z["stats"]
    for i, key in enumerate(("AP", "AP50", "AP75", "APs", "APm", "APl")):
        if st[i] == -1:
            assert np.isnan(res[key]), key
        else:
            assert res[key] == float(st[i] * 100), key
    assert set(res) == {"AP", "AP50", "AP75", "APs", "APm", "APl", "AP-0", "AP-1", "AP-2", "AP-3"}
    p = z["precision"]
    for k in range(4):
        v = p[:, :, k, 0, -1]
        v = v[v > -1]
        if v.size:
            assert res[f"AP-{k}"] == float(np.mean(v) * 100)
        else:
            assert np.isnan(res[f"AP-{k}"])
    assert np.isnan(res["AP-2"]) and not np.isnan(res["AP-3"])          # no ground truth: absent; no detection: AP 0
    named = ap.results(["a", "b", "c", "d"], stats=stats)
    assert named["AP-d"] == res["AP-3"] and "AP-0" not in named
    with pytest.raises(ValueError):
        ap.results(["a"], stats=stats)


@pytest.mark.parametrize("rule", RULES)
def test_combine_of_per_image_stats_equals_the_single_run(rule):
    from mp_former_amd.inference import InstanceAP
    g = load_golden()
    whole = golden_stats(g, rule, "small")
    parts = [golden_stats(g, rule, "small", images=[i]) for i in range(3)]
    for i, p in enumerate(parts):
        p["image"] = p["image"] + i                     # a shard numbers its own images from 0
    both = InstanceAP.combine(parts)
    assert_stats_equal(both, whole)
    ap = _ap(g, rule, "small")
    for k in ("precision", "recall", "scores"):
        assert bits(ap.accumulate(both)[k]) == bits(g[rule, "small"][k])
    assert parts[0]["npig"].sum() < whole["npig"].sum(), "combine must not change its inputs"
    with pytest.raises(ValueError):
        InstanceAP.combine([])


def test_stats_of_a_fresh_object_and_config_errors():
    from mp_former_amd.inference import InferenceConfig, InstanceAP
    ap = InstanceAP(3)
    assert ap.iou_thrs.tobytes() == np.linspace(.5, .95, 10).tobytes() and ap.max_dets == (1, 10, 100)
    assert ap.area_rngs.tolist() == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]
    s = ap.stats()
    assert s["scores"].shape == (0,) and s["matched"].shape == (0, 4, 10) and s["npig"].shape == (3, 4) and not s["npig"].any()
    assert (ap.accumulate()["precision"] == -1).all() and (ap.summarize() == -1).all()
    assert all(np.isnan(v) for v in ap.results().values())
    ap.reset()
    assert InstanceAP(3, max_dets=(100, 1, 10)).max_dets == (1, 10, 100)
    for bad in (dict(num_classes=0), dict(num_classes=3, crowd_rule="pixel"), dict(num_classes=3, iou_thrs=[]),
                dict(num_classes=3, area_rngs=[[0, 1, 2]]), dict(num_classes=3, max_dets=()), dict(num_classes=3, max_dets=(0, 5)),
                dict(num_classes=3, iou_thrs=np.linspace(.5, .95, 10), area_rngs=[[0, 1]] * 7)):
        with pytest.raises(ValueError):
            InstanceAP(**bad)
    InstanceAP(3, iou_thrs=np.linspace(.5, .95, 16), area_rngs=[[0, 1]] * 4)           # 64 settings fit
    with pytest.raises(ValueError):
        InstanceAP(3, area_rngs=[[0, 1e10]]).summarize()                               # the 12 statistics need four ranges
    with pytest.raises(ValueError):
        ap.accumulate({**s, "npig": np.zeros((2, 4), dtype=np.int64)})
    with pytest.raises(ValueError, match="instance_masks"):
        InferenceConfig(num_classes=3, instance_masks="bits")                          # the config is not touched
    with pytest.raises(ValueError, match="instance_on"):
        from mp_former_amd.inference import instance_bits
        instance_bits(None, None, None, None, None, InferenceConfig(num_classes=3, instance_on=False, semantic_on=True))


def test_cpu_tensors_raise():
    from mp_former_amd.inference import InferenceConfig, InstanceAP, instance_bits, mask_pair_counts, pack_masks
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        pack_masks(torch.zeros(2, 4, 5, dtype=torch.uint8))
    words = torch.zeros(2, 1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        mask_pair_counts(words, words)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        InstanceAP(3).update(words, [0.5, 0.4], [0, 1], words, [0, 1], [0, 0])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        InstanceAP(3, device="cpu").update(words, [0.5, 0.4], [0, 1], words, [0, 1], [0, 0])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        instance_bits(torch.zeros(1, 5, 4), torch.zeros(1, 5, 8, 8), [(32, 32)], (32, 32), [(32, 32)], InferenceConfig(num_classes=3))


class _FakeCuda:
    """a tensor stand-in that passes for a device tensor up to the shape checks"""

    def __init__(self, t):
        self.t, self.is_cuda, self.dtype, self.shape, self.device = t, True, t.dtype, t.shape, torch.device("cuda:0")

    def dim(self):
        return self.t.dim()

    def contiguous(self):
        return self


def test_shape_and_dtype_checks_come_before_any_launch():
    from mp_former_amd.inference import InstanceAP, mask_pair_counts, pack_masks
    with pytest.raises(ValueError, match=r"\[M, H, W\]"):
        pack_masks(_FakeCuda(torch.zeros(4, 5, dtype=torch.uint8)))
    with pytest.raises(ValueError, match=r"\[M, H, W\]"):
        pack_masks(_FakeCuda(torch.zeros(2, 0, 5, dtype=torch.uint8)))
    with pytest.raises(TypeError, match="uint8, bool or float32"):
        pack_masks(_FakeCuda(torch.zeros(2, 4, 5, dtype=torch.int32)))
    w = lambda *s, dt=torch.int64: _FakeCuda(torch.zeros(*s, dtype=dt))        # noqa: E731
    with pytest.raises(ValueError, match="int64"):
        mask_pair_counts(w(2, 3, dt=torch.int32), w(2, 3))
    with pytest.raises(ValueError, match="int64"):
        mask_pair_counts(w(6), w(2, 3))
    with pytest.raises(ValueError, match="nwords"):
        mask_pair_counts(w(2, 3), w(2, 4))
    with pytest.raises(ValueError, match="not one image"):
        InstanceAP(3).update(w(2, 3), [0.5, 0.4], [0, 1], w(1, 4), [0], [0])


# ---- the C entry points -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib


def test_ap_symbols_declared_exported_and_bound(built):
    src = open(os.path.join(ROOT, "include", "mpformer_hip.h")).read()
    assert "ytvoseval.py" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(raw, name) and name in built.SIGNATURES, name
    assert os.path.exists(os.path.join(ROOT, "mp_former_amd", "csrc", "seg_ap.hip"))
    assert "seg_ap.hip" in open(os.path.join(ROOT, "mp_former_amd", "csrc", "Makefile")).read()
    assert built.lib().mpf_abi_version() == 1


def test_ap_entry_points_reject_bad_arguments(built):
    lib = built.lib()
    one = ctypes.c_void_p(16)       # never dereferenced: the checks come first

    def ibits(masks=one, sq=64, dt=0, Q=5, h=8, w=8, Hp=32, Wp=32, hi=30, wi=31, H=37, W=50, sel=one, T=3, out=one):
        return lib.mpf_seg_instance_bits(masks, sq, dt, Q, h, w, Hp, Wp, hi, wi, H, W, sel, T, out, None)
    assert ibits(masks=None) == -3 and ibits(sel=None) == -3 and ibits(out=None) == -3
    assert ibits(dt=3) == -1 and ibits(T=0) == -2 and ibits(T=70000) == -2 and ibits(h=0) == -2 and ibits(hi=33) == -2
    assert ibits(out=ctypes.c_void_p(12)) == -2 and b"aligned" in lib.mpf_last_error()
    assert ibits(H=1 << 16, W=1 << 15) == -4

    def pack(masks=one, dt=3, M=2, H=7, W=9, out=one):
        return lib.mpf_seg_pack_masks(masks, dt, M, H, W, out, None)
    assert pack(masks=None) == -3 and pack(out=None) == -3
    assert pack(dt=2) == -1 and pack(dt=1) == -1 and b"dtype" in lib.mpf_last_error()
    assert pack(M=-1) == -2 and pack(H=0) == -2 and pack(W=-4) == -2
    assert pack(H=1 << 16, W=1 << 15) == -4 and pack(M=70000) == -4
    assert pack(M=0, masks=None, out=None) == 0                                    # nothing to do, nothing launched

    def pairs(a=one, T=3, b=one, G=2, nwords=5, inter=one, aa=one, ab=one):
        return lib.mpf_seg_mask_pairs(a, T, b, G, nwords, inter, aa, ab, None)
    for k in ("a", "b", "inter", "aa", "ab"):
        assert pairs(**{k: None}) == -3, k
    assert pairs(T=-1) == -2 and pairs(G=-1) == -2 and pairs(nwords=0) == -2
    assert pairs(T=1 << 16, G=1 << 16) == -4 and pairs(nwords=1 << 25) == -4
    assert pairs(T=0, G=0, a=None, b=None, inter=None, aa=None, ab=None) == 0      # nothing to do, nothing launched

    assert lib.mpf_seg_ap_workspace_bytes(20, 4, 10) == 800 and lib.mpf_seg_ap_workspace_bytes(0, 4, 10) == 0
    assert lib.mpf_seg_ap_workspace_bytes(-1, 4, 10) == 0

    def match(inter=one, ad=one, ag=one, D=3, G=2, sc=one, dc=one, gc=one, gcr=one, ga=one, thr=one, Tn=10, rng=one, A=4, K=5, md=100, rule=0,
              image=0, rec=one, npig=one, ws=one, nbytes=1 << 20):
        return lib.mpf_seg_ap_match(inter, ad, ag, D, G, sc, dc, gc, gcr, ga, thr, Tn, rng, A, K, md, rule, image, rec, npig, ws, nbytes, None)
    for k in ("inter", "ad", "ag", "sc", "dc", "gc", "gcr", "ga", "thr", "rng", "rec", "npig", "ws"):
        assert match(**{k: None}) == -3, k
    assert match(D=-1) == -2 and match(G=-1) == -2 and match(K=0) == -2 and match(A=0) == -2 and match(Tn=0) == -2 and match(md=0) == -2
    assert match(image=-1) == -2 and match(rule=2) == -2 and match(rule=-1) == -2
    assert match(A=7, Tn=10) == -2 and b"64" in lib.mpf_last_error()               # the record format holds 64 settings
    assert match(A=65, Tn=1) == -2 and match(A=1 << 20, Tn=1 << 20) == -2
    assert match(nbytes=79) == -2 and b"workspace" in lib.mpf_last_error()
    assert match(D=1 << 16, G=1 << 16) == -4
    assert match(D=0, G=0, inter=None, ad=None, ag=None, sc=None, dc=None, gc=None, gcr=None, ga=None, rec=None, ws=None, nbytes=0) == 0


# ---- the evaluator's host side ----------------------------------------------------------------------------------------------------
def test_evaluator_construction():
    from mp_former_amd import d2_plugin
    ev = d2_plugin.InstanceAPEvaluator(3, class_names=["a", "b", "c"], crowd_rule="union", max_dets=(1, 3, 5))
    assert ev.ap.num_classes == 3 and ev.ap.crowd_rule == "union" and ev.ap.max_dets == (1, 3, 5)
    ev.reset()
    out = ev.evaluate()                                          # before any image
    assert set(out) == {"segm"} and set(out["segm"]) == {"AP", "AP50", "AP75", "APs", "APm", "APl", "AP-a", "AP-b", "AP-c"}
    assert all(np.isnan(v) for v in out["segm"].values())
    with pytest.raises(ValueError):
        d2_plugin.InstanceAPEvaluator(3, class_names=["a"])
    for name in ("reset", "process", "evaluate"):
        assert callable(getattr(ev, name))
    import inspect
    sig = inspect.signature(d2_plugin.install_native_inference)
    assert sig.parameters["instance_bits"].default is False
    assert "detectron2" not in inspect.getsource(d2_plugin.InstanceAPEvaluator.process)
