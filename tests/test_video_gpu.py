"""GPU: the video eval branch on the device (csrc/seg_video.hip via mp_former_amd.inference.postprocess_video, the tube form of
InstanceAP, d2_plugin's video entry points) against the reference's own results (tests/golden/vinfer_small.npz, vap_small.npz)
and the restatements of tests/_video_restate.py.

Mask pixels may differ from the reference only inside the tie band: where the restatement's resampled logit is within 2e-5 of 0
(the "> 0" decision), and such pixels may be at most 0.1 % of the clip."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _ap_restate as A
import _video_restate as V
from test_ap_cpu import assert_stats_equal
from test_video_cpu import BAND, SETTINGS, VARIANTS, golden_tube_stats, load_vap, load_vinfer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FORMS = ("dense", "bits", "rle")


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _cfg(K, Q, masks="dense", topk=10):
    from mp_former_amd.inference import VideoInferenceConfig
    return VideoInferenceConfig(num_classes=K, num_queries=Q, topk=topk, masks=masks)


def _unpack(bits, H, W):
    """int64 [T, F, nwords] -> (bool [T, F, H, W], the bits at and past H * W)"""
    T, F, nwords = bits.shape
    dense, tail = A.unpack_columns(_np(bits).reshape(T * F, nwords), H, W)
    return dense.reshape(T, F, H, W), tail


def _clip(g, variant):
    m = g[variant + "_in"].to(DEV)
    return g["pred_logits"].to(DEV), m if variant == "f32" else m.to(torch.bfloat16)


def _run(g, variant, form, **kw):
    from mp_former_amd.inference import postprocess_video
    lg, mk = _clip(g, variant)
    return postprocess_video(lg, mk, g["image_size"], g["padded"], g["output_size"], _cfg(g["K"], g["Q"], form, **kw))


# ---- 1. fixture parity -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_fixture_parity_in_all_three_forms(variant):
    g = load_vinfer()
    want = g[variant]
    sc = want["scores"].astype(np.float64)
    assert (sc[:-1] - sc[1:]).min() > 1e-6, "the fixture's top-10 scores must be distinct: tie order may not decide the test"
    H, W = g["output_size"]
    r = V.inference_video(g["pred_logits"], g[variant + "_in"], g["image_size"], g["padded"], H, W)
    np.testing.assert_array_equal(r["masks"].numpy(), want["masks"])            # the restatement is the reference (test_video_cpu)
    band = np.abs(r["logits"].numpy()) <= BAND
    out = {form: _run(g, variant, form) for form in FORMS}
    for form, o in out.items():
        assert tuple(o["image_size"]) == (H, W), form
        np.testing.assert_array_equal(_np(o["pred_labels"]), want["labels"], err_msg=form)
        np.testing.assert_array_equal(_np(o["pred_queries"]), r["query"].numpy(), err_msg=form)
        np.testing.assert_allclose(_np(o["pred_scores"]), want["scores"], rtol=1e-5, atol=0, err_msg=form)
    for form in ("dense", "rle"):
        assert isinstance(out[form]["pred_scores"], list) and isinstance(out[form]["pred_labels"], list)
    b = out["bits"]
    assert b["pred_scores"].is_cuda and b["pred_labels"].is_cuda and b["bits"].dtype == torch.int64 and b["frame_area"].dtype == torch.int32
    dense = _np(out["dense"]["pred_masks"])
    assert dense.dtype == bool and dense.shape == want["masks"].shape and out["dense"]["pred_masks"].is_cuda
    diff = dense != want["masks"]
    print(f"{variant}: {int(diff.sum())} pixels differ, {int(band.sum())} of {band.size} inside the band")
    assert not (diff & ~band).any(), f"{int((diff & ~band).sum())} mask pixels differ outside the tie band"
    assert diff.sum() <= 1e-3 * diff.size, "more than 0.1 % of the clip's pixels were excused by the band"
    # the three forms agree with each other exactly
    unpacked, tail = _unpack(b["bits"], H, W)
    np.testing.assert_array_equal(unpacked, dense)
    assert not tail.any(), "bits at or past H * W must be zero"
    np.testing.assert_array_equal(_np(b["frame_area"]), dense.sum((2, 3)))
    rle = out["rle"]["pred_masks_rle"]
    assert len(rle) == dense.shape[0] and all(len(x) == dense.shape[1] for x in rle)
    for t in range(dense.shape[0]):
        for f in range(dense.shape[1]):
            assert rle[t][f] == {"size": [H, W], "counts": V.rle_counts(dense[t, f])}, (t, f)


def test_empty_clip_gives_the_reference_empty_result():
    from mp_former_amd.inference import postprocess_video
    for form in FORMS:
        o = postprocess_video(torch.zeros(0, 6, device=DEV), torch.zeros(0, 3, 9, 13, device=DEV), (33, 50), (36, 52), (47, 71), _cfg(5, 12, form))
        assert o["image_size"] == (47, 71) and len(o["pred_scores"]) == 0 and len(o["pred_labels"]) == 0
        if form == "dense":
            assert tuple(o["pred_masks"].shape) == (0, 3, 47, 71)
        elif form == "rle":
            assert o["pred_masks_rle"] == []
        else:
            assert tuple(o["bits"].shape) == (0, 3, 53) and tuple(o["frame_area"].shape) == (0, 3)


# ---- 2. F = 1 is the image route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_one_frame_is_the_image_route_bit_for_bit(variant):
    from mp_former_amd import _lib
    g = load_vinfer()
    lg, mk = _clip(g, variant)
    Q, F, h, w = mk.shape
    H, W = g["output_size"]
    nwords = (H * W + 63) // 64
    sel = torch.tensor([7, 0, 11, 3, 3], dtype=torch.int64, device=DEV)
    T = sel.numel()
    stream = _lib.stream_ptr(DEV)
    geo = (h, w, *g["padded"], *g["image_size"], H, W)
    for f in range(F):
        frame = mk[:, f]                                     # [Q, h, w], stride_q = F * h * w: the view the image route takes
        img = torch.full((T, nwords), -1, dtype=torch.int64, device=DEV)
        _lib.call("mpf_seg_instance_bits", DEV, frame.data_ptr(), frame.stride(0), _lib.DTYPE[mk.dtype], Q, *geo, sel.data_ptr(), T,
                  img.data_ptr(), stream)
        vid = torch.full((T, 1, nwords), -1, dtype=torch.int64, device=DEV)
        area = torch.full((T, 1), -1, dtype=torch.int32, device=DEV)
        _lib.call("mpf_seg_video_bits", DEV, frame.data_ptr(), frame.stride(0), 0, _lib.DTYPE[mk.dtype], Q, 1, *geo, sel.data_ptr(), T,
                  vid.data_ptr(), area.data_ptr(), None, stream)
        assert torch.equal(vid[:, 0], img), f
        # run lengths: bits the caller holds against the image route's own count + write
        ws = _lib.scratch("test.rle_img", DEV, stream, _lib.lib().mpf_seg_instance_rle_workspace_bytes(T, H, W))
        off_i = torch.empty(T + 1, dtype=torch.int64, device=DEV)
        _lib.call("mpf_seg_instance_rle_count", DEV, frame.data_ptr(), frame.stride(0), _lib.DTYPE[mk.dtype], Q, *geo, sel.data_ptr(), T,
                  off_i.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        total = int(off_i[T])
        pos, cnt_i = torch.empty(total, dtype=torch.int32, device=DEV), torch.empty(total, dtype=torch.int32, device=DEV)
        _lib.call("mpf_seg_instance_rle_write", DEV, ws.data_ptr(), ws.numel(), T, H, W, off_i.data_ptr(), total, pos.data_ptr(),
                  cnt_i.data_ptr(), stream)
        ws2 = _lib.scratch("test.rle_bits", DEV, stream, _lib.lib().mpf_seg_bits_rle_workspace_bytes(T, H, W))
        off_b = torch.empty(T + 1, dtype=torch.int64, device=DEV)
        _lib.call("mpf_seg_bits_rle_count", DEV, img.data_ptr(), T, H, W, off_b.data_ptr(), ws2.data_ptr(), ws2.numel(), stream)
        assert torch.equal(off_b, off_i)
        cnt_b = torch.empty(total, dtype=torch.int32, device=DEV)
        _lib.call("mpf_seg_bits_rle_write", DEV, img.data_ptr(), ws2.data_ptr(), ws2.numel(), T, H, W, off_b.data_ptr(), total, pos.data_ptr(),
                  cnt_b.data_ptr(), stream)
        assert torch.equal(cnt_b, cnt_i) and total > T


def test_rle_of_many_tiles_and_edge_masks():
    """bits_rle where a mask spans several count tiles (256 words each) and for all-zero / all-one / single-pixel masks"""
    from mp_former_amd.inference import bits_rle, pack_masks
    H, W = 211, 397                                          # 83767 positions: 1309 words, 6 tiles, a 55-bit tail
    gen = torch.Generator().manual_seed(5)
    m = torch.rand(6, H, W, generator=gen) > 0.5
    m[1] = False
    m[2] = True
    m[3] = False
    m[3, H - 1, W - 1] = True
    m[4] = torch.rand(H, W, generator=gen) > 0.999
    m[5, :, : W // 2] = True
    m[5, :, W // 2:] = False
    got = bits_rle(pack_masks(m.to(DEV)), (H, W))
    for i in range(m.shape[0]):
        assert got[i] == {"size": [H, W], "counts": V.rle_counts(m[i].numpy())}, i


# ---- 3. strides and entry counts -------------------------------------------------------------------------------------------------------
def test_strided_slice_equals_the_contiguous_copy():
    from mp_former_amd.inference import postprocess_video
    g = load_vinfer()
    lg, mk = _clip(g, "f32")
    Q, F, h, w = mk.shape
    big = torch.randn(2, 3 * Q, F + 1, h, w, device=DEV)
    big[1, Q:2 * Q, :F] = mk
    view = big[1, Q:2 * Q, :F]
    assert not view.is_contiguous() and view.stride(0) == (F + 1) * h * w and view.stride(1) == h * w
    ptr = view.data_ptr()
    for topk in (1, 10):
        cfg = _cfg(g["K"], Q, "bits", topk=topk)
        a = postprocess_video(lg, view, g["image_size"], g["padded"], g["output_size"], cfg)
        b = postprocess_video(lg, mk.contiguous(), g["image_size"], g["padded"], g["output_size"], cfg)
        assert a["bits"].shape[0] == topk == min(topk, Q * g["K"])
        for k in ("bits", "frame_area", "pred_scores", "pred_labels", "pred_queries"):
            assert torch.equal(a[k], b[k]), (topk, k)
        d = postprocess_video(lg, view, g["image_size"], g["padded"], g["output_size"], _cfg(g["K"], Q, "dense", topk=topk))
        np.testing.assert_array_equal(_np(d["pred_masks"]), _unpack(a["bits"], *g["output_size"])[0])
    assert view.data_ptr() == ptr and torch.equal(big[1, Q:2 * Q, :F], mk), "the slice is read in place and left alone"


def test_fewer_entries_than_topk():
    from mp_former_amd.inference import postprocess_video
    g = load_vinfer()
    lg, mk = _clip(g, "f32")
    o = postprocess_video(lg[:2, [0, 1, 2, 5]].contiguous(), mk[:2], g["image_size"], g["padded"], g["output_size"], _cfg(3, 2, "bits"))
    assert o["bits"].shape[0] == 6 and sorted(zip(_np(o["pred_queries"]).tolist(), _np(o["pred_labels"]).tolist())) == [
        (q, c) for q in range(2) for c in range(3)]
    sc = _np(o["pred_scores"])
    assert (sc[:-1] >= sc[1:]).all()


# ---- 4. tube AP -------------------------------------------------------------------------------------------------------------------------
def _pack_tubes(tubes, F, H, W):
    """tubes of tests/_video_restate.py -> int64 [M, F, nwords] on the device, through pack_masks"""
    from mp_former_amd.inference import pack_masks
    nwords = (H * W + 63) // 64
    if not tubes:
        return torch.empty((0, F, nwords), dtype=torch.int64, device=DEV)
    dense = np.stack([V.stack_frames(t["frames"], H, W) for t in tubes])
    return pack_masks(torch.from_numpy(dense.reshape(-1, H, W)).to(DEV)).view(len(tubes), F, nwords)


_packed = None


def _packed_videos():
    """the fixture's videos packed once, shared by the tests below and left unchanged"""
    global _packed
    if _packed is None:
        g = load_vap()
        H, W = g["size"]
        _packed = [(_pack_tubes(dts, F, H, W), _pack_tubes(gts, F, H, W)) for (dts, gts, _), F in zip(g["videos"], g["frames"])]
    return _packed


def _update(ap, g, v):
    dts, gts, _ = g["videos"][v]
    db, gb = _packed_videos()[v]
    ap.update(db, [d["score"] for d in dts], [d["category"] for d in dts], gb, [t["category"] for t in gts], [t["iscrowd"] for t in gts])


def _tube_ap(g, name, **kw):
    from mp_former_amd.inference import InstanceAP
    s = g[name]
    return InstanceAP(g["K"], area_rngs=s["area_rngs"], max_dets=s["max_dets"], tubes=True, device=DEV, **kw)


@pytest.mark.parametrize("name", SETTINGS)
def test_tube_ap_equals_the_reference(name):
    g = load_vap()
    ap = _tube_ap(g, name)
    for v in range(len(g["videos"])):
        _update(ap, g, v)
    stats = ap.stats()
    assert_stats_equal(stats, golden_tube_stats(g, name), name)
    z = g["union", name]
    np.testing.assert_allclose(ap.summarize(stats), z["stats"], rtol=0, atol=1e-12)
    res = ap.results(stats=stats)
    for i, key in enumerate(("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10")):
        want = z["stats"][i] * 100 if z["stats"][i] >= 0 else float("nan")
        assert (np.isnan(res[key]) and np.isnan(want)) or abs(res[key] - want) <= 1e-10, key
    # two shards combined equal one run
    a, b = _tube_ap(g, name), _tube_ap(g, name)
    for v in (0, 1):
        _update(a, g, v)
    for v in (2, 3):
        _update(b, g, v)
    sb = b.stats()
    sb["image"] = sb["image"] + 2
    assert_stats_equal(type(ap).combine([a.stats(), sb]), stats, name + " combined")


def test_tube_areas_on_the_device():
    from mp_former_amd.inference import tube_avg_areas, tube_frame_areas
    g = load_vap()
    H, W = g["size"]
    for (dts, gts, _), (db, gb) in zip(g["videos"], _packed_videos()):
        for tubes, packed, key in ((dts, db, "dt_avg_area"), (gts, gb, "gt_avg_area")):
            if not tubes:
                continue
            fa = tube_frame_areas(packed)
            want = np.asarray([[0 if a is None else a for a in V.frame_areas(t["frames"])] for t in tubes])
            np.testing.assert_array_equal(_np(fa), want)
            ids = [t["id"] - 1 for t in tubes]
            assert _np(tube_avg_areas(fa)).tobytes() == np.asarray(g[key][ids], dtype=np.float64).tobytes()


@pytest.mark.parametrize("rule", ["union", "coco"])
def test_one_frame_tubes_give_the_records_of_the_image_form(rule):
    from mp_former_amd.inference import InstanceAP, pack_masks
    from test_ap_cpu import load_golden
    g = load_golden()
    s = g["small"]
    kw = dict(area_rngs=s["area_rngs"], max_dets=s["max_dets"], crowd_rule=rule, device=DEV)
    img, tube = InstanceAP(g["K"], **kw), InstanceAP(g["K"], tubes=True, **kw)
    for dts, gts in g["images"]:
        dm = pack_masks(torch.from_numpy(np.stack([d["mask"] for d in dts])).to(DEV))
        gm = pack_masks(torch.from_numpy(np.stack([t["mask"] for t in gts])).to(DEV))
        args = ([d["score"] for d in dts], [d["category"] for d in dts]), ([t["category"] for t in gts], [t["iscrowd"] for t in gts])
        img.update(dm, *args[0], gm, *args[1])
        tube.update(dm[:, None], *args[0], gm[:, None], *args[1])
    assert_stats_equal(tube.stats(), img.stats(), rule)


# ---- 5. end to end ------------------------------------------------------------------------------------------------------------------------
class ImageList:
    """detectron2.structures.ImageList.from_tensors: pad to the largest image, rounded up to size_divisibility."""

    def __init__(self, tensor, image_sizes):
        self.tensor, self.image_sizes = tensor, image_sizes

    @staticmethod
    def from_tensors(tensors, size_divisibility=0, pad_value=0.0):
        sizes = [(int(t.shape[-2]), int(t.shape[-1])) for t in tensors]
        d = max(int(size_divisibility), 1)
        hmax, wmax = ((max(s[i] for s in sizes) + d - 1) // d * d for i in (0, 1))
        out = tensors[0].new_full((len(tensors), tensors[0].shape[0], hmax, wmax), pad_value)
        for i, t in enumerate(tensors):
            out[i, :, :t.shape[-2], :t.shape[-1]].copy_(t)
        return ImageList(out, sizes)


class _StubVideoHead:
    """Fixed random predictions sized from the input frames [F, 3, Hp, Wp]: [1, Q, K+1] logits, [1, Q, F, Hp / 4, Wp / 4] mask logits."""

    def __init__(self, K, Q):
        self.num_classes, self.Q = K, Q

    def __call__(self, x):
        F, hp, wp = int(x.shape[0]), int(x.shape[-2]), int(x.shape[-1])
        gen = torch.Generator().manual_seed(hp * 7 + wp + F)
        logits = torch.randn(1, self.Q, self.num_classes + 1, generator=gen) * 2
        masks = torch.randn(1, self.Q, F, hp // 4, wp // 4, generator=gen) * 4
        return {"pred_logits": logits.to(DEV), "pred_masks": masks.to(DEV)}


def _stub_video_model(K, Q):
    m = SimpleNamespace(device=DEV, pixel_mean=torch.tensor([120.0, 115.0, 100.0], device=DEV).view(3, 1, 1),
                        pixel_std=torch.tensor([58.0, 57.0, 57.0], device=DEV).view(3, 1, 1), size_divisibility=32,
                        backbone=lambda x: x, sem_seg_head=_StubVideoHead(K, Q), num_queries=Q, training=False)
    m.forward = lambda batched_inputs: (_ for _ in ()).throw(AssertionError("the reference's forward ran in eval mode"))
    return m


def test_installed_video_inference_feeds_the_evaluator():
    from mp_former_amd import d2_plugin
    from mp_former_amd.inference import postprocess_video
    K, Q, F = 4, 9, 3
    inp = {"image": [torch.rand(3, 50, 70) * 255 for _ in range(F)], "height": 61, "width": 83, "video_id": 17, "length": F}
    outs = {}
    for form in FORMS:
        model = _stub_video_model(K, Q)
        cfg = d2_plugin.install_native_video_inference(model, masks=form, image_list_cls=ImageList)
        assert (cfg.num_classes, cfg.num_queries, cfg.topk, cfg.masks) == (K, Q, 10, form)
        outs[form] = model.forward([inp])
    head = _StubVideoHead(K, Q)(torch.zeros(F, 3, 64, 96))
    want = postprocess_video(head["pred_logits"][0], head["pred_masks"][0], (50, 70), (64, 96), (61, 83), _cfg(K, Q, "dense"))
    dense = _np(outs["dense"]["pred_masks"])
    assert dense.shape == (10, F, 61, 83) and dense.any()
    np.testing.assert_array_equal(dense, _np(want["pred_masks"]))
    assert outs["dense"]["pred_scores"] == want["pred_scores"] and outs["dense"]["pred_labels"] == want["pred_labels"]
    # the submission entries decode back to the dense masks
    res = d2_plugin.YTVISEvaluatorHIP.results_json(inp["video_id"], outs["rle"])
    assert len(res) == 10
    for t, r in enumerate(res):
        assert r["video_id"] == 17 and r["score"] == want["pred_scores"][t] and r["category_id"] == want["pred_labels"][t]
        assert len(r["segmentations"]) == F
        for f, seg in enumerate(r["segmentations"]):
            np.testing.assert_array_equal(V.rle_decode(seg), dense[t, f])
    # the evaluator on the bits form: ground truth = the masks of three predicted entries, one of them with a frame left out
    gt_masks = torch.from_numpy(dense[[0, 3, 5]].copy())
    gt_masks[1, 1] = False
    gt_classes = [want["pred_labels"][i] for i in (0, 3, 5)]
    ev = d2_plugin.YTVISEvaluatorHIP(K, device=DEV)
    ev.process([{"instances": {"gt_masks": gt_masks, "gt_classes": gt_classes}}], outs["bits"])
    res = ev.evaluate()["segm"]
    assert {"AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10"} <= set(res)
    # the same numbers from the restatement
    dts = [{"id": t + 1, "category": want["pred_labels"][t], "score": float(np.float32(want["pred_scores"][t])), "frames": list(dense[t])}
           for t in range(10)]
    gts = [{"id": i + 1, "category": gt_classes[i], "iscrowd": 0, "frames": [m if m.any() else None for m in gt_masks[i].numpy()]}
           for i in range(3)]
    ev_imgs = V.evaluate_tubes([(dts, gts, (61, 83))], K, V.YTVIS_AREA_RNGS, [1, 10, 100])
    st = A.summarize(A.accumulate(ev_imgs, K, 1, V.YTVIS_AREA_RNGS, [1, 10, 100]), [1, 10, 100])
    for i, key in enumerate(("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10")):
        w = st[i] * 100 if st[i] >= 0 else float("nan")
        assert (np.isnan(res[key]) and np.isnan(w)) or abs(res[key] - w) <= 1e-10, key
    assert res["AP50"] > 0
    # packed ground truth gives the same
    from mp_former_amd.inference import pack_masks
    ev2 = d2_plugin.YTVISEvaluatorHIP(K, device=DEV)
    packed = pack_masks(gt_masks.reshape(-1, 61, 83).to(DEV)).view(3, F, -1)
    ev2.process([{"instances": {"gt_masks": packed, "gt_classes": gt_classes}}], outs["bits"])
    np.testing.assert_equal(ev2.evaluate(), {"segm": res})        # (nan where a range holds no ground truth: equal as nan)


# ---- 6. no host sync, memory, reproducibility -------------------------------------------------------------------------------------------
def test_bits_route_and_update_make_no_host_sync():
    from mp_former_amd.inference import TubeAP, postprocess_video
    g = load_vinfer()
    lg, mk = _clip(g, "f32")
    cfg = _cfg(g["K"], g["Q"], "bits")
    args = (lg, mk, g["image_size"], g["padded"], g["output_size"], cfg)
    ap = TubeAP(g["K"], device=DEV)
    o = postprocess_video(*args)
    gt = o["bits"][[0, 4]].clone()
    upd = lambda o: ap.update(o["bits"], o["pred_scores"], o["pred_labels"], gt, [1, 2], [0, 0], dt_frame_area=o["frame_area"])     # noqa: E731
    upd(o)                                                   # warm: scratch and record buffers allocated
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        o2 = postprocess_video(*args)
        upd(o2)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert len(ap.stats()["scores"]) == 20
    for k in ("bits", "frame_area", "pred_scores", "pred_labels"):
        assert torch.equal(o[k], o2[k]), k


def test_memory_and_kernels_of_the_bits_route():
    from mp_former_amd import _lib
    from mp_former_amd.inference import postprocess_video
    Q, K, F, H, W, T = 100, 40, 8, 360, 640, 10
    gen = torch.Generator().manual_seed(3)
    lg = torch.randn(Q, K + 1, generator=gen).to(DEV)
    mk = (torch.randn(Q, F, 96, 168, generator=gen) * 4).to(DEV)
    cfg = _cfg(K, Q, "bits")
    run = lambda: postprocess_video(lg, mk, (360, 640), (384, 672), (H, W), cfg)     # noqa: E731
    a = run()                                                # warm: the scratch buffers are allocated
    assert _lib.last_kernel() == "seg_video_bits_kernel"
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    b = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak increase of the bits route {peak / 2**20:.2f} MiB, the dense bool masks alone {T * F * H * W / 2**20:.2f} MiB")
    assert peak < T * F * H * W, (peak, T * F * H * W)
    for k in ("bits", "frame_area", "pred_scores", "pred_labels", "pred_queries"):
        assert torch.equal(a[k], b[k]), k                    # integer atomics: reproducible bit for bit
    assert int(a["frame_area"].sum()) > 0 and a["bits"].shape == (T, F, (H * W + 63) // 64)
    del a, b
    d = postprocess_video(lg, mk, (360, 640), (384, 672), (H, W), _cfg(K, Q, "dense"))
    assert _lib.last_kernel() == "seg_video_bits_kernel<dense>"
    # many workgroups per frame: the selection against torch's, the masks against the reference's two resizes of the selected planes
    sc, idx = lg.cpu().softmax(-1)[:, :-1].flatten().topk(T, sorted=True)
    assert (sc[:-1] - sc[1:]).min() > 1e-6 and d["pred_queries"] == (idx // K).tolist() and d["pred_labels"] == (idx % K).tolist()
    up = torch.nn.functional.interpolate(mk.cpu()[idx // K], size=(384, 672), mode="bilinear", align_corners=False)
    logit = torch.nn.functional.interpolate(up[:, :, :360, :640], size=(H, W), mode="bilinear", align_corners=False).numpy()
    diff = _np(d["pred_masks"]) != (logit > 0)
    assert not (diff & (np.abs(logit) > BAND)).any() and diff.sum() <= 1e-3 * diff.size


# ---- 7. argument errors -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    from mp_former_amd import _lib
    from mp_former_amd.inference import TubeAP, postprocess_video, tube_avg_areas
    g = load_vinfer()
    lg, mk = _clip(g, "f32")
    lib = _lib.lib()
    _lib.call("mpf_seg_tube_areas", DEV, torch.zeros(3, dtype=torch.int32, device=DEV).data_ptr(), 1, 3,
              torch.zeros(1, dtype=torch.float64, device=DEV).data_ptr(), _lib.stream_ptr(DEV))
    before = _lib.last_kernel()
    assert before == "seg_tube_areas_kernel"
    one = ctypes.c_void_p(64)
    geo = (12, 3, 9, 13, 36, 52, 33, 50, 47, 71)
    assert lib.mpf_seg_video_bits(None, 351, 117, 0, *geo, one, 2, one, one, None, None) == -3
    assert lib.mpf_seg_video_bits(one, 351, 117, 0, *geo, one, 2, None, one, None, None) == -3
    assert lib.mpf_seg_video_bits(one, 468, 117, 0, 12, 4, 9, 13, 36, 52, 33, 50, 23171, 23171, one, 2, one, one, None, None) == -4
    assert lib.mpf_seg_ap_match_tube(one, one, one, 2, 2, one, one, one, one, one, None, one, 10, one, 4, 3, 100, 1, 0, one, one, one, 80,
                                     None) == -3
    assert _lib.last_kernel() == before, "an argument error must not launch"
    ap = TubeAP(3, device=DEV)
    a = torch.zeros((2, 3, 14), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="not one video"):
        ap.update(a, [1., 1.], [0, 0], torch.zeros((2, 3, 15), dtype=torch.int64, device=DEV), [0, 0], [0, 0])
    with pytest.raises(ValueError, match="not one video"):
        ap.update(a, [1., 1.], [0, 0], torch.zeros((2, 4, 14), dtype=torch.int64, device=DEV), [0, 0], [0, 0])
    with pytest.raises(ValueError, match="packed tubes"):
        ap.update(a[:, 0], [1., 1.], [0, 0], a, [0, 0], [0, 0])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        ap.update(a.cpu(), [1., 1.], [0, 0], a, [0, 0], [0, 0])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        postprocess_video(lg.cpu(), mk, g["image_size"], g["padded"], g["output_size"], _cfg(g["K"], g["Q"]))
    with pytest.raises(ValueError, match="frame areas"):
        tube_avg_areas(torch.zeros((2, 3), dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="classes"):
        postprocess_video(lg, mk, g["image_size"], g["padded"], g["output_size"], _cfg(g["K"] + 1, g["Q"]))
    assert _lib.last_kernel() == before and ap.stats()["scores"].size == 0
