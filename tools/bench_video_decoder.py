#!/usr/bin/env python3
"""Device time and kernel launches of the clip decoder (mp_former_amd/video_decoder.py) next to a plain-torch statement of the
reference's layer loop (video_mask2former_transformer_decoder.py:370-461) on the same parameters, under bf16 autocast:

  train   B = 2 clips x T = 2 frames of 360 x 640 (YouTube-VIS training), Q = 100, 9 layers: forward + backward
  eval    B = 1, T = 36 frames (a whole video): forward under no_grad

    python tools/bench_video_decoder.py [--shape train|eval|both] [--iters 20] [--json out.json]

Routes: "ops" = the module with every layer op by op (``fused_layers = False``: one autograd node per op on the native attention /
small-GEMM / residual-LayerNorm kernels; clip-inputs kernel, fused mask head, batched key / value projections and prediction
heads); "native" = native, one call per layer (``fused_layers = True``: the same kernels issued by decoder_layer.decoder_layer_pos,
one autograd node per layer); "torch" = ``reference_forward`` below: nn.MultiheadAttention per attention, the
[B, Q, T, H/4, W/4] logits map resized and thresholded per layer, the bool mask repeated for the heads.  The routes ALTERNATE call
by call in one process (after 3 warm calls each), so that they see the same clocks; times are medians (min, max) of device-event
intervals around whole calls; launches are the device kernels one forward enqueues, counted by the profiler in a pass of its own
(not timed)."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"train": dict(B=2, T=2, training=True), "eval": dict(B=1, T=36, training=False)}
FRAME = (360, 640)
Q, K, LAYERS, FFN = 100, 40, 9, 2048


def reference_forward(m, x, mask_features):
    """The reference's forward, op for op, on the parameters of the native module ``m`` (whose attention layers hold
    nn.MultiheadAttention modules under the reference's names)."""
    bt, c_m, h_m, w_m = mask_features.shape
    bs = bt // m.num_frames if m.training else 1
    t = bt // bs
    mf = mask_features.view(bs, t, c_m, h_m, w_m)
    src, pos, size_list = [], [], []
    for i in range(m.num_feature_levels):
        size_list.append(x[i].shape[-2:])
        p = m.pe_layer(x[i].view(bs, t, -1, size_list[-1][0], size_list[-1][1]), None).flatten(3)
        s = x[i].flatten(2) + m.level_embed.weight[i][None, :, None]
        _, c, hw = s.shape
        pos.append(p.reshape(bs, t, c, hw).permute(1, 3, 0, 2).flatten(0, 1))
        src.append(s.view(bs, t, c, hw).permute(1, 3, 0, 2).flatten(0, 1))
    query_embed = m.query_embed.weight.unsqueeze(1).repeat(1, bs, 1)
    output = m.query_feat.weight.unsqueeze(1).repeat(1, bs, 1)

    def heads(output, size):
        d = m.decoder_norm(output).transpose(0, 1)
        cls = m.class_embed(d)
        om = torch.einsum("bqc,btchw->bqthw", m.mask_embed(d), mf)
        b, q, tt = om.shape[:3]
        am = F.interpolate(om.flatten(0, 1), size=size, mode="bilinear", align_corners=False).view(b, q, tt, size[0], size[1])
        am = (am.sigmoid().flatten(2).unsqueeze(1).repeat(1, m.num_heads, 1, 1).flatten(0, 1) < 0.5).bool()
        return cls, om, am.detach()

    classes, masks = [], []
    c, om, attn_mask = heads(output, size_list[0])
    classes.append(c)
    masks.append(om)
    for i in range(m.num_layers):
        lv = i % m.num_feature_levels
        attn_mask[torch.where(attn_mask.sum(-1) == attn_mask.shape[-1])] = False
        ca, sa, ff = m.transformer_cross_attention_layers[i], m.transformer_self_attention_layers[i], m.transformer_ffn_layers[i]
        t2 = ca.multihead_attn(query=output + query_embed, key=src[lv] + pos[lv], value=src[lv], attn_mask=attn_mask)[0]
        output = ca.norm(output + t2)
        qk = output + query_embed
        output = sa.norm(output + sa.self_attn(qk, qk, value=output)[0])
        output = ff.norm(output + ff.linear2(F.relu(ff.linear1(output))))
        c, om, attn_mask = heads(output, size_list[(i + 1) % m.num_feature_levels])
        classes.append(c)
        masks.append(om)
    return {"pred_logits": classes[-1], "pred_masks": masks[-1],
            "aux_outputs": [{"pred_logits": a, "pred_masks": b} for a, b in zip(classes[:-1], masks[:-1])]}


def make_inputs(B, T, dev, seed=0):
    """the pixel decoder's hand-over: three fp32 channel-last maps (1/32, 1/16, 1/8) and the 1/4 mask features"""
    g = torch.Generator().manual_seed(seed)
    H, W = FRAME

    def planes(h, w):
        return torch.randn(B * T, h, w, 256, generator=g).to(dev).permute(0, 3, 1, 2)

    xs = [planes(-(-H // s), -(-W // s)) for s in (32, 16, 8)]
    return xs, planes(H // 4, W // 4)


def seeds_for(out, dev):
    g = torch.Generator().manual_seed(1)
    outs = [(a["pred_logits"], a["pred_masks"]) for a in out["aux_outputs"]] + [(out["pred_logits"], out["pred_masks"])]
    return [(torch.randn(c.shape, generator=g).to(dev).to(c.dtype), torch.randn(mk.shape[1:], generator=g).to(dev).to(mk.dtype))
            for c, mk in outs]


def step_fn(route, m, xs, mf, training):
    def module_forward():
        m.fused_layers = route == "native"
        try:
            return m(xs, mf)
        finally:
            m.fused_layers = None

    fwd = module_forward if route in ("ops", "native") else (lambda: reference_forward(m, xs, mf))
    seeds = []

    def forward():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            return fwd()

    def step():
        if not training:
            with torch.no_grad():
                return forward()
        out = forward()
        if not seeds:
            seeds.extend(seeds_for(out, mf.device))
        outs = [(a["pred_logits"], a["pred_masks"]) for a in out["aux_outputs"]] + [(out["pred_logits"], out["pred_masks"])]
        loss = sum((c.float() * sc.float()).sum() + (mk.float() * sm.float()).sum() for (c, mk), (sc, sm) in zip(outs, seeds))
        m.zero_grad(set_to_none=True)
        for t in xs + [mf]:
            t.grad = None
        loss.backward()
        return out

    def forward_only():
        with torch.no_grad():
            return forward()

    return step, forward_only


def timed(fns, iters):
    """{route: fn} -> {route: (median, min, max) ms}: 3 warm calls each, then ``iters`` rounds in which the routes take turns"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = {r: [] for r in fns}
    for _ in range(iters):
        for r, fn in fns.items():
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[r].append(e0.elapsed_time(e1))
    out = {}
    for r, t in ts.items():
        t.sort()
        out[r] = (t[len(t) // 2], t[0], t[-1])
    return out


def count_launches(fn):
    """device kernels enqueued by one call (copies and fills left out), by the profiler; None where it records no device events"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = 0
    for e in prof.events():
        if str(e.device_type).endswith("CUDA") and not e.name.lower().startswith(("memcpy", "memset")):
            n += 1
    return n or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["train", "eval", "both"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--routes", default="ops,native,torch")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_video_decoder needs the GPU: nothing is measured without one")
    from mp_former_amd.video_decoder import VideoMultiScaleMaskedTransformerDecoder
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = VideoMultiScaleMaskedTransformerDecoder(256, True, num_classes=K, hidden_dim=256, num_queries=Q, nheads=8, dim_feedforward=FFN,
                                                dec_layers=LAYERS, pre_norm=False, mask_dim=256, enforce_input_project=False,
                                                num_frames=2).to(dev)
    results = []
    for shape in (["train", "eval"] if args.shape == "both" else [args.shape]):
        sp = SHAPES[shape]
        m.train(sp["training"])
        xs, mf = make_inputs(sp["B"], sp["T"], dev)
        if sp["training"]:
            xs, mf = [x.requires_grad_(True) for x in xs], mf.requires_grad_(True)
        fns = {route: step_fn(route, m, xs, mf, sp["training"]) for route in args.routes.split(",")}
        times = timed({route: step for route, (step, _) in fns.items()}, args.iters)
        for route, (_, forward_only) in fns.items():
            med, lo, hi = times[route]
            launches = count_launches(forward_only)
            r = {"shape": shape, "B": sp["B"], "T": sp["T"], "route": route, "what": "forward+backward" if sp["training"] else "forward",
                 "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "iters": args.iters,
                 "launches_per_forward": launches}
            print(json.dumps(r), flush=True)
            results.append(r)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
