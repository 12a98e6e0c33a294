"""CPU: semantic test-time augmentation without a GPU — the argument rules of ``inference.SemanticTTA``, the argument checks of
the three ``mpf_seg_tta_*`` entry points (never-dereferenced pointers, as tests/test_abi_cpu.py), and the host side of
``d2_plugin.SemanticSegmentorWithTTAHIP`` (flip detection, the default mapper's ImportError)."""
import ctypes
import importlib.util
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TTA_SYMBOLS = ("mpf_seg_tta_accumulate", "mpf_seg_tta_resize_add", "mpf_seg_tta_finish")


def _cfg(**kw):
    from mp_former_amd.inference import InferenceConfig
    return InferenceConfig(num_classes=5, num_queries=3, **kw)


def test_semantic_tta_argument_rules():
    from mp_former_amd.inference import SemanticTTA
    with pytest.raises(ValueError, match="semantic_on"):
        SemanticTTA(_cfg())
    tta = SemanticTTA(_cfg(semantic_on=True, instance_on=False, sem_seg_postprocess_before_inference=False))
    with pytest.raises(RuntimeError, match="no view"):
        tta.result()
    lg, mk = torch.zeros(3, 6), torch.zeros(3, 8, 12)
    with pytest.raises(RuntimeError, match="CPU"):
        tta.add(lg, mk, (30, 45), (32, 48), (29, 41), False)
    with pytest.raises(RuntimeError, match="CPU"):
        tta.add(lg[None], mk[None], (30, 45), (32, 48), (29, 41), True)           # the batched form of one view
    with pytest.raises(ValueError, match="classes"):
        tta.add(torch.zeros(3, 8), mk, (30, 45), (32, 48), (29, 41), False)       # K = 7 against the config's 5
    with pytest.raises(ValueError, match="one view"):
        tta.add(torch.zeros(2, 3, 6), torch.zeros(2, 3, 8, 12), (30, 45), (32, 48), (29, 41), False)
    with pytest.raises(ValueError, match="one view"):
        tta.add(lg, torch.zeros(4, 8, 12), (30, 45), (32, 48), (29, 41), False)   # queries of masks and logits differ
    with pytest.raises(RuntimeError, match="no view"):                             # a refused view was not counted
        tta.result()
    tta.reset()


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib


def test_tta_symbols_declared_exported_and_bound(built):
    src = open(os.path.join(ROOT, "include", "mpformer_hip.h")).read()
    assert "test_time_augmentation.py:71-98" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    raw = ctypes.CDLL(built.LIB_PATH)
    for name in TTA_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} not declared"
        assert hasattr(raw, name) and name in built.SIGNATURES, name
    assert built.ABI_VERSION == 1 and built.lib().mpf_abi_version() == 1          # additions only


def test_tta_entry_points_reject_bad_arguments(built):
    lib = built.lib()
    one = ctypes.c_void_p(16)       # never dereferenced: the checks come first
    geom = [10, 14, 40, 56, 37, 50, 29, 41]
    E_DTYPE, E_SHAPE, E_NULL = -1, -2, -3
    acc = lambda masks, stride, dt, probs, K, mode, out: lib.mpf_seg_tta_accumulate(masks, stride, dt, 4, *geom, probs, K, mode, out, None)
    assert acc(None, 140, 0, one, 3, 0, one) == E_NULL
    assert acc(one, 140, 0, None, 3, 0, one) == E_NULL
    assert acc(one, 140, 0, one, 3, 1, None) == E_NULL and b"seg_tta_accumulate" in lib.mpf_last_error()
    assert acc(one, 140, 99, one, 3, 0, one) == E_DTYPE
    assert acc(one, 100, 0, one, 3, 0, one) == E_SHAPE                              # stride_q < h * w
    assert acc(one, 140, 0, one, 0, 0, one) == E_SHAPE
    for mode in (4, 7, -1, 1 << 8):
        assert acc(one, 140, 0, one, 3, mode, one) == E_SHAPE and b"mode" in lib.mpf_last_error(), mode
    assert lib.mpf_seg_tta_resize_add(None, 3, 37, 50, 29, 41, 0, one, None) == E_NULL
    assert lib.mpf_seg_tta_resize_add(one, 3, 37, 50, 29, 41, 3, None, None) == E_NULL
    assert lib.mpf_seg_tta_resize_add(one, 0, 37, 50, 29, 41, 0, one, None) == E_SHAPE
    assert lib.mpf_seg_tta_resize_add(one, 3, 37, 50, 0, 41, 0, one, None) == E_SHAPE
    assert lib.mpf_seg_tta_resize_add(one, 3, 37, 50, 29, 41, 4, one, None) == E_SHAPE and b"mode" in lib.mpf_last_error()
    assert lib.mpf_seg_tta_finish(None, 3, 29, 41, 6, None, None) == E_NULL
    assert lib.mpf_seg_tta_finish(one, 3, 29, 41, 0, None, None) == E_SHAPE and b"count" in lib.mpf_last_error()
    assert lib.mpf_seg_tta_finish(one, 3, 29, 41, -2, one, None) == E_SHAPE
    assert lib.mpf_seg_tta_finish(one, 0, 29, 41, 6, None, None) == E_SHAPE
    assert lib.mpf_seg_tta_finish(one, 3, 1 << 16, 1 << 16, 6, None, None) == -4                  # MPF_E_TOO_LARGE, as mpf_seg_semantic

# ---- the wrapper ------------------------------------------------------------------------------------------------------------------
class HFlipTransform:
    """Named as fvcore's class: where fvcore is absent the wrapper matches the name."""


class VFlipTransform:
    pass


def _model(**kw):
    base = dict(sem_seg_head=SimpleNamespace(num_classes=5), num_queries=10, object_mask_threshold=0.8, overlap_threshold=0.8,
                test_topk_per_image=100, semantic_on=True, instance_on=False, panoptic_on=False,
                sem_seg_postprocess_before_inference=False, metadata=None)
    base.update(kw)
    return SimpleNamespace(**base)


def test_flip_detection():
    from mp_former_amd import d2_plugin
    if importlib.util.find_spec("fvcore") is not None:
        from fvcore.transforms import HFlipTransform as Flip, NoOpTransform
        assert d2_plugin.is_hflip(SimpleNamespace(transforms=[NoOpTransform(), Flip(10)]))
        assert not d2_plugin.is_hflip(SimpleNamespace(transforms=[NoOpTransform()]))
        return
    assert d2_plugin.is_hflip(SimpleNamespace(transforms=[VFlipTransform(), HFlipTransform()]))
    assert not d2_plugin.is_hflip(SimpleNamespace(transforms=[VFlipTransform()]))
    assert not d2_plugin.is_hflip(SimpleNamespace(transforms=[]))
    assert d2_plugin.is_hflip([HFlipTransform()])                                   # a bare list of transforms


def test_wrapper_construction():
    from mp_former_amd import d2_plugin
    mapper = lambda inp: []
    seg = d2_plugin.SemanticSegmentorWithTTAHIP(None, _model(), mapper, batch_size=3, semantic_labels=True)
    assert seg.tta_mapper is mapper and seg.batch_size == 3
    assert seg.inference_cfg.semantic_labels and seg.inference_cfg.num_classes == 5
    assert not seg.inference_cfg.sem_seg_postprocess_before_inference
    assert not d2_plugin.SemanticSegmentorWithTTAHIP(None, _model(), mapper).inference_cfg.semantic_labels
    with pytest.raises(ValueError, match="semantic_on"):
        d2_plugin.SemanticSegmentorWithTTAHIP(None, _model(semantic_on=False, sem_seg_postprocess_before_inference=True), mapper)
    if importlib.util.find_spec("detectron2") is None:
        with pytest.raises(ImportError, match="tta_mapper"):
            d2_plugin.SemanticSegmentorWithTTAHIP(None, _model())
