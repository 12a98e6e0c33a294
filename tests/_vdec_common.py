"""What tests/golden/make_golden_vdec.py (reference side) and the video-decoder tests (native side) share: the two fixture
configurations, the closed-form inputs and gradient seeds (tests/golden/det_params.py, so the fixtures hold results only), and the
rule by which a large tensor is recorded as a strided sample."""
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import det_params as DP  # noqa: E402

CONFIGS = {
    # T*HW = 64 / 192 / 480 in training (T = 2): multiples of 16 on every level; layer 3 returns to level 0
    "vdec_small": dict(hidden=256, heads=8, ffn=64, Q=7, K=5, dec_layers=4, num_frames=2, B=2, levels=[(4, 8), (8, 12), (12, 20)],
                       mf=(24, 40), eval_frames=3),
    # T*HW = 30 at level 0: not a multiple of 16, the attention masks of that level come from the torch route
    "vdec_odd": dict(hidden=256, heads=8, ffn=64, Q=33, K=5, dec_layers=4, num_frames=2, B=2, levels=[(3, 5), (6, 10), (12, 20)],
                     mf=(24, 40), eval_frames=None),
}
SAMPLE_CAP = 6000
# gradients the fixtures record besides the inputs' (layer 0's attention weights)
WEIGHT_GRADS = ["transformer_cross_attention_layers.0.multihead_attn.in_proj_weight",
                "transformer_cross_attention_layers.0.multihead_attn.out_proj.weight",
                "transformer_self_attention_layers.0.self_attn.in_proj_weight",
                "transformer_self_attention_layers.0.self_attn.out_proj.weight"]
SMALL_GRADS = ["query_embed.weight", "query_feat.weight", "level_embed.weight"]


def module_kwargs(cfg):
    return dict(in_channels=cfg["hidden"], mask_classification=True, num_classes=cfg["K"], hidden_dim=cfg["hidden"],
                num_queries=cfg["Q"], nheads=cfg["heads"], dim_feedforward=cfg["ffn"], dec_layers=cfg["dec_layers"], pre_norm=False,
                mask_dim=cfg["hidden"], enforce_input_project=False, num_frames=cfg["num_frames"])


def unit(name, shape):
    """closed-form U(-1, 1) values, fp32"""
    return DP.det_tensor(name, shape, "bias") * 20.0


def inputs(name, cfg, seed, B, T):
    """-> ([x0, x1, x2] each [B*T, C, h, w], mask_features [B*T, C, H, W]) of one run"""
    C = cfg["hidden"]
    xs = [unit(f"{name}.s{seed}.T{T}.x{i}", (B * T, C, h, w)) for i, (h, w) in enumerate(cfg["levels"])]
    mf = unit(f"{name}.s{seed}.T{T}.mf", (B * T, C) + tuple(cfg["mf"]))
    return xs, mf


def outputs_list(out):
    """the output dict -> [(class logits, mask logits)] of layer 0 .. L (the final one last)"""
    return [(a["pred_logits"], a["pred_masks"]) for a in out["aux_outputs"]] + [(out["pred_logits"], out["pred_masks"])]


def seeded_loss(name, outs):
    """sum over every output of seed * output, the seeds closed-form and of the output's shape"""
    total = 0.0
    for l, (c, m) in enumerate(outs):
        total = total + (unit(f"{name}.seed.cls{l}", c.shape).to(c.device) * c.float()).sum()
        total = total + (unit(f"{name}.seed.mask{l}", m.shape).to(m.device) * m.float()).sum()
    return total


def sample(a):
    """a tensor / array as the fixtures record it: whole up to SAMPLE_CAP elements, else every step-th element of the flattened
    array with the smallest odd step that keeps it under the cap"""
    a = a.detach().float().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    a = a.reshape(-1)
    if a.size <= SAMPLE_CAP:
        return a
    step = -(-a.size // SAMPLE_CAP) | 1
    return a[::step]


def clip_row_rule(am):
    """:409 on bool [B, Q, T*HW]: a query masked at every position of the clip attends everywhere"""
    am = am.clone()
    am[am.all(-1)] = False
    return am
