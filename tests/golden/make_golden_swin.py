#!/usr/bin/env python3
"""Generate tests/golden/swin_tiny.npz and tests/golden/swin_keys.json by running the reference's OWN Swin backbone
(mask2former/modeling/backbone/swin.py, unmodified, imported by path) on the CPU, where the reference is importable; no test or
benchmark reads the reference.  Usage:

    python tests/golden/make_golden_swin.py

Behind _ref_import.setup(), with stand-ins of its own for the two imports the file needs beyond it: ``timm.models.layers``
(DropPath, to_2tuple, trunc_normal_) and, added to the ``detectron2.modeling`` stand-in, BACKBONE_REGISTRY, Backbone, ShapeSpec.

swin_tiny.npz: the tiny configuration of tests/_swin_common.py in fp64 on its closed-form input and parameters — the four output
maps, the gradient of sum(out^2) with respect to the input image and to each stage's first relative_position_bias_table and
qkv.bias.  swin_keys.json: names and shapes of the state dicts of Swin-T (window 7) and Swin-B (window 12)."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import as R  # noqa: E402
import _swin_common as S  # noqa: E402


class DropPath(nn.Module):
    """timm's stochastic depth, documented semantics: per-sample keep with probability 1 - p, scaled by 1 / (1 - p), identity in eval"""

    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1.0 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        return x * mask / keep


def to_2tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x, x)


def load_reference():
    R.setup()
    R._mod("timm")
    R._mod("timm.models")
    R._mod("timm.models.layers", DropPath=DropPath, to_2tuple=to_2tuple, trunc_normal_=nn.init.trunc_normal_)
    d2 = sys.modules["detectron2.modeling"]
    d2.BACKBONE_REGISTRY = R.Registry("BACKBONE")
    d2.Backbone = nn.Module
    d2.ShapeSpec = R.ShapeSpec
    folder = os.path.join(R.M2F, "modeling", "backbone")
    R._pkg(R.PKG + ".modeling.backbone", folder)
    spec = importlib.util.spec_from_file_location(R.PKG + ".modeling.backbone.swin", os.path.join(folder, "swin.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference()
    model = ref.SwinTransformer(**S.TINY).double()
    model.load_state_dict(S.det_state(model), strict=True)
    model.train()
    x = S.det_input().requires_grad_(True)
    outs = model(x)
    S.loss_of(outs).backward()
    params = dict(model.named_parameters())
    data = {k: outs[k].detach().numpy() for k in S.OUTPUTS}
    data["grad.input"] = x.grad.numpy()
    for k in S.GRAD_PARAMS:
        data["grad." + k] = params[k].grad.numpy()
    path = os.path.join(HERE, "swin_tiny.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes", {k: v.shape for k, v in data.items()})

    keys = {}
    for name, cfg in S.SIZES.items():
        m = ref.SwinTransformer(**cfg)
        keys[name] = {k: list(v.shape) for k, v in m.state_dict().items()}
    path = os.path.join(HERE, "swin_keys.json")
    with open(path, "w") as f:
        json.dump(keys, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes", {k: len(v) for k, v in keys.items()})


if __name__ == "__main__":
    main()
