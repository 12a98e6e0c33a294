#!/usr/bin/env python3
"""Generate tests/golden/vdec_small.npz and vdec_odd.npz by running the reference's OWN video decoder on the CPU in fp32: the
unmodified ``VideoMultiScaleMaskedTransformerDecoder`` (mask2former_video/modeling/transformer_decoder/
video_mask2former_transformer_decoder.py) and ``PositionEmbeddingSine3D`` (position_encoding.py), run where the reference is
importable; no test or benchmark reads it.  Usage:

    python tests/golden/make_golden_vdec.py

The two files are loaded from their paths as one package behind _ref_import.setup(), so that the decoder's relative import of the
position encoding works, with one more stand-in: ``mask2former.modeling.transformer_decoder.maskformer_transformer_decoder`` holding
a ``TRANSFORMER_DECODER_REGISTRY``.  Parameters, inputs and gradient seeds are closed-form by name (tests/_vdec_common.py), so the
fixtures hold results only; tensors above ``SAMPLE_CAP`` elements are recorded as strided samples (``_vdec_common.sample``).

Recorded per run ("train": the configuration's B clips of ``num_frames`` frames in training mode; "eval", vdec_small only: the same
module in eval mode on 3 frames, bs = 1): class and mask logits of every layer, the dec_layers + 1 attention masks as
``forward_prediction_heads`` returns them (head 0 of the 8 identical copies, before the all-masked-row rule of :409, bit-packed),
the position embedding of every level; for "train" also the gradients of sum(seed * output) with respect to the three feature
maps, ``mask_features``, ``query_embed``, ``query_feat``, ``level_embed`` and layer 0's attention weights.

Seed condition: the seed in the inputs' names is advanced until no resized mask logit (the tensor ``F.interpolate`` returns inside
``forward_prediction_heads``) lies within margin x (RMS of its [h, w] plane) of zero, in any run of the fixture; margin starts at
1e-4 and drops by a power of ten whenever 50 seeds in a row fail.  Seed and margin are stored.  A second fp32 pipeline whose logits
differ by less than that therefore thresholds every position the same way."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _ref_import as R  # noqa: E402
import _vdec_common as V  # noqa: E402

PKG = "_mpf_ref_vdec"


def load_reference():
    R.setup()
    for name in ("mask2former", "mask2former.modeling", "mask2former.modeling.transformer_decoder"):
        if name not in sys.modules:
            R._mod(name)
    R._mod("mask2former.modeling.transformer_decoder.maskformer_transformer_decoder",
           TRANSFORMER_DECODER_REGISTRY=R.Registry("TRANSFORMER_MODULE"))
    folder = os.path.join(R.REF, "mask2former_video", "modeling", "transformer_decoder")
    R._pkg(PKG, folder)
    mods = {}
    for leaf in ("position_encoding", "video_mask2former_transformer_decoder"):
        spec = importlib.util.spec_from_file_location(PKG + "." + leaf, os.path.join(folder, leaf + ".py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[spec.name] = mod
        spec.loader.exec_module(mod)
        mods[leaf] = mod
    return mods["video_mask2former_transformer_decoder"], mods["position_encoding"]


class _RecordingF:
    """torch.nn.functional with ``interpolate`` recording what it returns (the resized mask logits)"""

    def __init__(self, real):
        self._real, self.resized = real, []

    def __getattr__(self, name):
        return getattr(self._real, name)

    def interpolate(self, *a, **k):
        out = self._real.interpolate(*a, **k)
        self.resized.append(out.detach())
        return out


def closest_to_zero(resized):
    """min over the resized logits of |v| / RMS(its [h, w] plane)"""
    worst = float("inf")
    for r in resized:
        rms = r.double().pow(2).mean((-2, -1), keepdim=True).sqrt()
        worst = min(worst, float((r.double().abs() / rms).min()))
    return worst


def run(dec_mod, module, name, cfg, seed, training, B, T):
    module.train(training)
    xs, mf = V.inputs(name, cfg, seed, B, T)
    xs = [x.requires_grad_(training) for x in xs]
    mf = mf.requires_grad_(training)
    rec = _RecordingF(torch.nn.functional)
    masks = []
    heads = module.forward_prediction_heads

    def recording_heads(*a, **k):
        c, m, am = heads(*a, **k)
        b = m.shape[0]
        masks.append(am.view(b, module.num_heads, am.shape[1], am.shape[2])[:, 0].clone())
        return c, m, am

    dec_mod.F = rec
    module.forward_prediction_heads = recording_heads
    try:
        out = module(xs, mf)
    finally:
        dec_mod.F = rec._real
        del module.forward_prediction_heads
    tag = "train" if training else "eval"
    outs = V.outputs_list(out)
    z = {f"{tag}.cls": np.stack([c.detach().numpy() for c, _ in outs])}
    for l, (_, m) in enumerate(outs):
        assert m.shape[:3] == (B, cfg["Q"], T)
        z[f"{tag}.masks{l}"] = V.sample(m)
    assert len(masks) == cfg["dec_layers"] + 1
    for l, am in enumerate(masks):
        z[f"{tag}.attn{l}"] = np.packbits(am.numpy())
    for i, (h, w) in enumerate(cfg["levels"]):
        pos = module.pe_layer(torch.zeros(1, T, 1, h, w), None)[0]            # [T, C, h, w]
        z[f"{tag}.pos{i}"] = V.sample(pos)
    if training:
        module.zero_grad()
        V.seeded_loss(f"{name}.{tag}", outs).backward()
        params = dict(module.named_parameters())
        for i, x in enumerate(xs):
            z[f"{tag}.grad.x{i}"], z[f"{tag}.gradnorm.x{i}"] = V.sample(x.grad), np.float64(x.grad.double().norm())
        z[f"{tag}.grad.mf"], z[f"{tag}.gradnorm.mf"] = V.sample(mf.grad), np.float64(mf.grad.double().norm())
        for k in V.SMALL_GRADS + V.WEIGHT_GRADS:
            z[f"{tag}.grad.{k}"], z[f"{tag}.gradnorm.{k}"] = V.sample(params[k].grad), np.float64(params[k].grad.double().norm())
    return z, closest_to_zero(rec.resized)


def make(dec_mod, name):
    cfg = V.CONFIGS[name]
    module = dec_mod.VideoMultiScaleMaskedTransformerDecoder(**V.module_kwargs(cfg))
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict(V.DP.det_state_dict(shapes, name + "."), strict=True)
    runs = [(True, cfg["B"], cfg["num_frames"])] + ([(False, 1, cfg["eval_frames"])] if cfg["eval_frames"] else [])
    seed, margin, tried = 0, 1e-4, 0
    while True:
        z, ok = {}, True
        for training, B, T in runs:
            zz, closest = run(dec_mod, module, name, cfg, seed, training, B, T)
            z.update(zz)
            if closest < margin:
                ok = False
                break
        if ok:
            break
        seed, tried = seed + 1, tried + 1
        if tried == 50:
            margin, tried = margin / 10.0, 0
    z["cfg"] = json.dumps(cfg)
    z["seed"], z["margin"] = np.int64(seed), np.float64(margin)
    z["param_names"] = json.dumps({k: list(s) for k, s in shapes.items()})
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **z)
    print(f"{path}: {os.path.getsize(path)} bytes, seed {seed}, margin {margin:g}")


def main():
    torch.set_num_threads(1)
    dec_mod, _ = load_reference()
    for name in V.CONFIGS:
        make(dec_mod, name)


if __name__ == "__main__":
    main()
