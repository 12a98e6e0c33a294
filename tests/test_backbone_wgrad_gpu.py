"""The two weight-gradient routes of the bench backbone (MPF_BACKBONE_WGRAD / backbone.set_wgrad_route) on res3 + res4 of
ResNet50 under bf16 autocast: "native" defers the weight gradients of the stride-1 convolutions to the stage's grouped launches
(csrc/gemm3_conv_wgrad.h), "miopen" is the library's convolution backward for all of them.

Every parameter gradient is float(bf16_rn(dW)) * scale with dW the weight gradient of the folded convolution, so it is checked
against an fp64 CPU evaluation from the bf16 (dY, x) of that very convolution, captured on the way, with the bound of
tests/test_conv_wgrad_gpu.py: (2^-8 |ref| + 4 R 2^-24 |dY|^T|X|) |scale| + 2^-24 |ref scale|."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GEMM, REDUCE = "gemm3_nt_group_kernel<bf16 conv>", "conv_wgrad_reduce_kernel"


@pytest.fixture(scope="module")
def net():
    import mp_former_amd.backbone as bb
    torch.manual_seed(5)
    m = bb.ResNet50().to(DEV).to(memory_format=torch.channels_last)
    for mod in m.modules():
        if hasattr(mod, "running_var"):
            mod.running_var.uniform_(0.5, 2.0); mod.running_mean.normal_(0, 0.1); mod.weight.uniform_(0.5, 1.5); mod.bias.normal_(0, 0.1)
    return m


@pytest.fixture
def deterministic_library():
    """At these small shapes the library's default forward and data-gradient kernels are not reproducible call to call (the same
    route run twice differs in its outputs), so "bitwise equal between the routes" is only defined with the library held to its
    deterministic algorithms.  The native launches do not read the switch."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = prev


def stages(net):
    return [("res3", net.res3), ("res4", net.res4)]


def capture(bb, monkeypatch):
    """-> log of {"conv", "x", "gy"} per convolution of the forwards that follow: the input and the output gradient as the
    convolution's backward sees them"""
    log, cur = [], {}
    conv_bn, bias_act, bias_act_fork = bb.conv_bn, bb.bias_act, bb.bias_act_fork

    def hook(y):
        e = cur["e"]
        if y.requires_grad:
            y.register_hook(lambda g, e=e: e.__setitem__("gy", g.detach()))

    def conv_bn_(conv, bn, x, *a, **k):
        cur["e"] = {"conv": conv, "bn": bn, "x": x.detach()}
        log.append(cur["e"])
        return conv_bn(conv, bn, x, *a, **k)

    def bias_act_(y, *a, **k):
        hook(y)
        return bias_act(y, *a, **k)

    def bias_act_fork_(y, *a, **k):
        hook(y)
        return bias_act_fork(y, *a, **k)

    monkeypatch.setattr(bb, "conv_bn", conv_bn_)
    monkeypatch.setattr(bb, "bias_act", bias_act_)
    monkeypatch.setattr(bb, "bias_act_fork", bias_act_fork_)
    return log


def step(bb, net, x0, gs, route):
    prev = bb.set_wgrad_route(route)
    try:
        for p in net.parameters():
            p.grad = None
        x = x0.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = bb.run_stages(x, stages(net))
        sum((out[k].float() * gs[k]).sum() for k in out).backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
        return {k: v.detach().clone() for k, v in out.items()}, x.grad.clone(), grads
    finally:
        bb.set_wgrad_route(prev)


def eligible(bb, log):
    """(1x1 count, 3x3 count, flops) of the convolutions the native route takes"""
    n1 = n3 = 0
    flops = 0.0
    for e in log:
        c, x = e["conv"], e["x"]
        if c.stride != (1, 1):
            continue
        R = x.shape[0] * x.shape[2] * x.shape[3]
        if c.kernel_size == (1, 1):
            n1 += 1
            flops += 2.0 * R * c.out_channels * c.in_channels
        elif c.in_channels % 128 == 0 and x.shape[3] % 8 == 0:
            n3 += 1
            flops += 2.0 * R * c.out_channels * 9 * c.in_channels
    return n1, n3, flops


def check_against_fp64(log, grads, net):
    names = {id(p): n for n, p in net.named_parameters()}
    for e in log:
        conv, x, gy = e["conv"], e["x"].double().cpu(), e["gy"].double().cpu()
        w = conv.weight
        ref, mag = (torch.ops.aten.convolution_backward(a, b, torch.zeros_like(w, dtype=torch.float64, device="cpu"), None, list(conv.stride),
                                                        list(conv.padding), [1, 1], False, [0, 0], 1, [False, True, False])[1]
                    for a, b in ((gy, x), (gy.abs(), x.abs())))
        s = e["bn"].scale_bias()[0].double().cpu().view(-1, 1, 1, 1)
        R = gy.shape[0] * gy.shape[2] * gy.shape[3]
        bound = (2.0 ** -8 * ref.abs() + 4.0 * R * 2.0 ** -24 * mag) * s.abs() + 2.0 ** -24 * (ref * s).abs()
        err = (grads[names[id(w)]].double().cpu() - ref * s).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{names[id(w)]}: max |err| / bound = {worst:.3f}")
        assert bool((err <= bound).all()), f"{names[id(w)]}: {worst:.3f} x the bound"


@pytest.mark.parametrize("side,native_3x3", [(16, 3), (32, 8)])
def test_routes_agree_and_match_fp64(net, monkeypatch, deterministic_library, side, native_3x3):
    """side 16: res3 runs at 8 x 8 (its 3x3 convolutions are eligible), res4 at 4 x 4 (W % 8 != 0: they fall back to the
    library); side 32: 16 x 16 and 8 x 8, none falls back"""
    import mp_former_amd.backbone as bb
    from mp_former_amd import _lib
    g = torch.Generator().manual_seed(side)
    x0 = torch.randn(2, 256, side, side, generator=g).bfloat16().to(DEV).contiguous(memory_format=torch.channels_last)
    gs = {"res3": torch.randn(2, 512, side // 2, side // 2, generator=g).to(DEV), "res4": torch.randn(2, 1024, side // 4, side // 4, generator=g).to(DEV)}
    log = capture(bb, monkeypatch)

    _lib.profile_enable(True)
    try:
        native = step(bb, net, x0, gs, "native")
        n_gemm, n_red, flops = _lib.profile_get(GEMM)[0], _lib.profile_get(REDUCE)[0], _lib.profile_get_flops(GEMM)
    finally:
        _lib.profile_enable(False)
    log_native, n = list(log), len(log)
    assert n == 4 * 3 + 1 + 6 * 3 + 1 and all("gy" in e for e in log_native)
    n1, n3, want_flops = eligible(bb, log_native)
    assert (n1, n3) == (20, native_3x3)
    # res3: 8 + 3 items, one launch; res4: 12 (+ 5) items, one (two) launches; as many reduces; and every eligible
    # convolution's weight gradient in them: the logged flops are theirs, those of the fallen-back 3x3 are not
    cap = _lib.lib().mpf_conv_wgrad_group_max()
    launches = -(-11 // cap) + -(-(12 + native_3x3 - 3) // cap)
    assert n_gemm == launches and n_red == launches
    assert flops == want_flops
    check_against_fp64(log_native, native[2], net)

    _lib.profile_enable(True)
    try:
        miopen = step(bb, net, x0, gs, "miopen")
        assert _lib.profile_get(GEMM)[0] == 0 and _lib.profile_get(REDUCE)[0] == 0
    finally:
        _lib.profile_enable(False)
    log_miopen = log[n:]
    check_against_fp64(log_miopen, miopen[2], net)

    for k in native[0]:
        assert torch.equal(native[0][k], miopen[0][k]), k
    assert torch.equal(native[1], miopen[1]), "input gradient"
    assert sorted(native[2]) == sorted(miopen[2]) and len(native[2]) == n
    for e_n, e_m in zip(log_native, log_miopen):         # the same (dY, x) reached every convolution
        assert torch.equal(e_n["gy"], e_m["gy"]) and torch.equal(e_n["x"], e_m["x"])
    again = step(bb, net, x0, gs, "native")
    assert all(torch.equal(native[2][k], again[2][k]) for k in native[2] if "conv1" in k or "conv3" in k), "native gradients not reproducible"


def test_no_grad_and_fp32_take_the_old_path(net):
    import mp_former_amd.backbone as bb
    from mp_former_amd import _lib
    x = torch.randn(2, 256, 16, 16, device=DEV).contiguous(memory_format=torch.channels_last)
    assert bb.set_wgrad_route("native") == "native"            # the default
    with pytest.raises(ValueError):
        bb.set_wgrad_route("cudnn")
    _lib.profile_enable(True)
    try:
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            y = bb.run_stages(x.bfloat16(), [("res3", net.res3)])["res3"]
        assert not y.requires_grad
        for p in net.parameters():
            p.grad = None
        xg = x.clone().requires_grad_(True)
        y32 = bb.run_stages(xg, [("res3", net.res3)])["res3"]              # fp32, no autocast
        y32.sum().backward()
        torch.cuda.synchronize()
        assert _lib.profile_get(GEMM)[0] == 0 and _lib.profile_get(REDUCE)[0] == 0
        assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in net.res3.parameters())
        # a channels-first bf16 input: the convolutions it reaches stay on the library
        with torch.autocast("cuda", dtype=torch.bfloat16):
            blk = net.res3[1]
            xc = torch.randn(2, 512, 8, 8, device=DEV).bfloat16().requires_grad_(True)
            folded = bb.ResNet50._fold_group(blk.pairs(), torch.bfloat16)
            assert bb._wgrad_kind(blk.conv1, xc, folded[0][0]) is None
            assert bb._wgrad_kind(blk.conv1, xc.contiguous(memory_format=torch.channels_last), folded[0][0]) == bb._CW_1X1
    finally:
        _lib.profile_enable(False)
