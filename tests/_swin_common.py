"""What tests/golden/make_golden_swin.py (reference side) and the Swin tests (this side) share: the tiny configuration, its input
and closed-form parameters by key (tests/golden/det_params.py), so that the fixture holds results only."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import det_params  # noqa: E402

TINY = dict(embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], window_size=7, drop_path_rate=0.0)
INPUT_SHAPE = (2, 3, 54, 70)        # neither side a multiple of 4; token maps 14 x 18, 7 x 9, 4 x 5, 2 x 3: every stage pads its windows
OUTPUTS = ("res2", "res3", "res4", "res5")
# the parameters whose gradients the fixture stores: each stage's first bias table and qkv bias
GRAD_PARAMS = [f"layers.{i}.blocks.0.attn.{leaf}" for i in range(4) for leaf in ("relative_position_bias_table", "qkv.bias")]
# the two published sizes whose key sets are recorded (tests/golden/swin_keys.json)
SIZES = {
    "swin_t": dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24], window_size=7),
    "swin_b": dict(embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32], window_size=12),
}


def det_state(model, dtype=torch.float64):
    """closed-form values for every floating-point entry of the model's state dict, by key; bias tables as `weight` kind
    (U(-1.5, 1.5) / sqrt(heads): large enough to move the softmax)"""
    out = {}
    for k, v in model.state_dict().items():
        if not v.is_floating_point():
            out[k] = v.clone()
            continue
        kind = "weight" if k.endswith("relative_position_bias_table") else None
        out[k] = det_params.det_tensor("swin." + k, v.shape, kind).to(dtype)
    return out


def det_input(dtype=torch.float64):
    return det_params.det_tensor("swin.input", INPUT_SHAPE, "gain").to(dtype) - 1.0 + det_params.det_tensor("swin.input2", INPUT_SHAPE,
                                                                                                             "weight").to(dtype) * 20.0


def loss_of(outs):
    return sum((outs[k].double() ** 2).sum() for k in OUTPUTS)
