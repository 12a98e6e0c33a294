"""CPU: the host side of the clip decoder (mp_former_amd/video_decoder.py, d2_plugin.register_video) against the fixtures that
tests/golden/make_golden_vdec.py recorded from the reference's own module."""
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _vdec_common as V
from conftest import GOLDEN


def _fixture(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


@pytest.mark.parametrize("name", list(V.CONFIGS))
def test_position_tables_recompose_the_reference_embedding(name):
    """pos_yx[s] + pos_z[t] is the reference's [T, C, H, W] PositionEmbeddingSine3D value (position_encoding.py:56), on every
    level of the training run and of the 3-frame eval run"""
    from mp_former_amd.video_decoder import PositionEmbeddingSine3D
    cfg, z = V.CONFIGS[name], _fixture(name)
    pe = PositionEmbeddingSine3D(cfg["hidden"] // 2, normalize=True)
    for tag, T in (("train", cfg["num_frames"]), ("eval", cfg["eval_frames"])):
        if T is None:
            continue
        for i, (h, w) in enumerate(cfg["levels"]):
            pos_yx, pos_z = pe.tables(T, h, w, torch.device("cpu"))
            assert pos_yx.shape == (h * w, cfg["hidden"]) and pos_z.shape == (T, cfg["hidden"])
            assert pe.tables(T, h, w, torch.device("cpu"))[0] is pos_yx                                   # cached
            full = (pos_yx[None, :, :] + pos_z[:, None, :]).view(T, h, w, -1).permute(0, 3, 1, 2)         # [T, C, H, W]
            np.testing.assert_allclose(V.sample(full), z[f"{tag}.pos{i}"], rtol=1e-6, atol=0)
            assert torch.equal(pe(torch.zeros(2, T, 1, h, w))[1], full)


@pytest.mark.parametrize("name", list(V.CONFIGS))
def test_state_dict_keys_are_the_reference_names(name):
    from mp_former_amd.video_decoder import VideoMultiScaleMaskedTransformerDecoder
    cfg, z = V.CONFIGS[name], _fixture(name)
    m = VideoMultiScaleMaskedTransformerDecoder(**V.module_kwargs(cfg))
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == json.loads(str(z["param_names"]))
    assert "query_embed.weight" in m.state_dict()


def test_static_query_checkpoint_loads():
    """a checkpoint from before version 2 names ``query_feat`` ``static_query`` (:213-234)"""
    from mp_former_amd.video_decoder import VideoMultiScaleMaskedTransformerDecoder
    cfg = V.CONFIGS["vdec_small"]
    m = VideoMultiScaleMaskedTransformerDecoder(**V.module_kwargs(cfg))
    sd = {k.replace("query_feat", "static_query"): v.clone() + 1.0 for k, v in m.state_dict().items()}
    assert "static_query.weight" in sd and "query_feat.weight" not in sd
    want = sd["static_query.weight"].clone()
    m.load_state_dict(sd, strict=True)                       # no metadata: version None
    assert torch.equal(m.query_feat.weight, want)
    # a version-2 state dict is taken as it is, and one with the old name is then an error
    m.load_state_dict(m.state_dict(), strict=True)
    old = m.state_dict()
    old["static_query.weight"] = old.pop("query_feat.weight")
    with pytest.raises(RuntimeError):
        m.load_state_dict(old, strict=True)


def test_register_video_with_a_fake_registry():
    from mp_former_amd import d2_plugin
    from mp_former_amd.video_decoder import VideoMultiScaleMaskedTransformerDecoder

    class Registry:
        def __init__(self):
            self._map = {}

        def register(self, obj=None):
            if obj is None:
                return lambda o: self.register(o) or o
            assert obj.__name__ not in self._map
            self._map[obj.__name__] = obj
            return obj

        def get(self, name):
            return self._map[name]

    reg = Registry()
    cls = d2_plugin.register_video(reg)
    assert cls and cls.__name__ == "VideoMultiScaleMaskedTransformerDecoder" == d2_plugin.VIDEO_TRANSFORMER_DECODER_NAME
    assert reg.get("VideoMultiScaleMaskedTransformerDecoder") is cls and issubclass(cls, VideoMultiScaleMaskedTransformerDecoder)
    assert d2_plugin.register_video() is False              # no detectron2 / mask2former here: nothing to register with
    cfg = NS(MODEL=NS(SEM_SEG_HEAD=NS(NUM_CLASSES=40, MASK_DIM=256),
                      MASK_FORMER=NS(NHEADS=8, HIDDEN_DIM=256, NUM_OBJECT_QUERIES=100, DIM_FEEDFORWARD=64, DEC_LAYERS=4, PRE_NORM=False,
                                     ENFORCE_INPUT_PROJ=False)),
             INPUT=NS(SAMPLING_FRAME_NUM=2))
    dec = cls(cfg, 256, True)                               # build_transformer_decoder's call
    assert dec.num_layers == 3 and dec.num_frames == 2 and dec.num_queries == 100 and dec.class_embed.out_features == 41
    by_kw = cls(**V.module_kwargs(V.CONFIGS["vdec_small"]))
    assert by_kw.num_layers == 4 and by_kw.num_queries == 7


def test_cpu_tensors_are_refused():
    from mp_former_amd.video_decoder import VideoMultiScaleMaskedTransformerDecoder
    cfg = V.CONFIGS["vdec_small"]
    m = VideoMultiScaleMaskedTransformerDecoder(**V.module_kwargs(cfg))
    xs, mf = V.inputs("vdec_small", cfg, 0, cfg["B"], cfg["num_frames"])
    with pytest.raises(RuntimeError, match="GPU only"):
        m(xs, mf)
