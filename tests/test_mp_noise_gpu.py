"""GPU: the native point noise of the mask-piloted rows (csrc/mp_noise.hip) against the numpy restatement of its contract
(test_mp_noise_cpu.py), against the torch route fed with the same draws, and inside the head.  Every comparison of bytes is
exact: the kernel is integer arithmetic plus one fp32 multiply and one fp32 compare."""
import numpy as np
import pytest
import torch

from test_mp_noise_cpu import (FLIP_CASE, check_flip_rate, flip_case_rows, noise_rows_ref, noise_u, rect_rows, src_of_table)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(600)]

DEV = torch.device("cuda:0")
KERNEL = "mp_noise_rows_kernel"


def _native(base, src_of, N, pad, noise_scale, seed, draw):
    from mp_former_amd import _lib, transformer_decoder as TD
    b = torch.from_numpy(np.ascontiguousarray(base)).to(DEV).bool()
    s = torch.from_numpy(np.ascontiguousarray(src_of, dtype=np.int32)).to(DEV)
    out = TD.mp_noise_rows(b, s, N, pad, noise_scale, seed, draw)
    assert _lib.last_kernel() == KERNEL, _lib.last_kernel()
    assert out.dtype == torch.bool and tuple(out.shape) == (N, pad, base.shape[1])
    return out.view(torch.uint8).cpu().numpy()


def _case(name):
    """-> (base uint8 [R, HW], src_of int32 [N * pad], N, pad)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ("hw32", "hw64", "hw128"):
        side = int(name[2:])
        num, scalar = [4, 7], 2
        base = np.tile(rect_rows(sum(num), side, side, rng), (scalar, 1))
    elif name == "hw_odd":                       # 30 x 25 = 750: not a multiple of 16 (nor of 4): the byte-wise route and its tail
        num, scalar = [3, 2], 3
        base = np.tile(rect_rows(sum(num), 30, 25, rng), (scalar, 1))
    elif name == "one_row":
        num, scalar = [1], 1
        base = rect_rows(1, 32, 32, rng)
    elif name == "scalar5_ragged":               # scalar 5, ragged T_b, an image without instances (all its rows -1)
        num, scalar = [3, 0, 6, 1], 5
        base = np.tile(rect_rows(sum(num), 64, 64, rng), (scalar, 1))
    elif name == "full_and_empty_rows":          # rows that are all 1 (ratio 0: nothing flips) and all 0 (ratio = noise_scale)
        num, scalar = [4], 2
        one = rect_rows(4, 32, 32, rng)
        one[1] = 1
        one[2] = 0
        base = np.tile(one, (scalar, 1))
    else:
        raise KeyError(name)
    src_of, pad = src_of_table(num, scalar)
    return base, src_of, len(num), pad


CASES = ["hw32", "hw64", "hw128", "hw_odd", "one_row", "scalar5_ragged", "full_and_empty_rows"]


@pytest.mark.parametrize("name", CASES)
def test_rows_equal_the_restatement_bit_for_bit(name):
    base, src_of, N, pad = _case(name)
    seed, draw = 0x0123456789ABCDEF, (3 << 32) | 40
    got = _native(base, src_of, N, pad, 0.2, seed, draw)
    want = noise_rows_ref(base, src_of, N, pad, 0.2, seed, draw)
    bad = int((got != want).sum())
    print(f"{name}: R = {base.shape[0]}, HW = {base.shape[1]}, N = {N}, pad = {pad}: {bad} mismatching bytes, "
          f"{int((want.reshape(N * pad, -1)[src_of >= 0] != base[src_of[src_of >= 0]]).sum())} flips")
    assert bad == 0
    assert set(np.unique(got)) <= {0, 1}
    assert (got.reshape(N * pad, -1)[src_of < 0] == 1).all()
    if name == "full_and_empty_rows":
        rows = got.reshape(N * pad, -1)
        assert (rows[1] == 1).all(), "a row without open positions has ratio 0: no flip"
        assert 0 < rows[2].sum() < rows.shape[1], "an all-open row flips with probability noise_scale"
    if name == "scalar5_ragged":
        assert (got[1] == 1).all(), "the image without instances has only padding rows"


def test_open_counts():
    from mp_former_amd import _lib, transformer_decoder as TD
    for name in ("hw128", "hw_odd", "full_and_empty_rows"):
        base = _case(name)[0]
        got = TD.mp_open_counts(torch.from_numpy(base).to(DEV).bool())
        assert _lib.last_kernel() == "mp_open_counts_kernel"
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), (base == 0).sum(1))


def _small_decoder(num_queries=4):
    from mp_former_amd.transformer_decoder import MultiScaleMaskedTransformerDecoderMaskDN
    return MultiScaleMaskedTransformerDecoderMaskDN(
        256, True, num_classes=5, hidden_dim=256, num_queries=num_queries, nheads=8, dim_feedforward=64, dec_layers=1,
        pre_norm=False, mask_dim=256, enforce_input_project=False, dn_mode="points", head_dn=False, all_lys=True,
        dn_label_noise_ratio=-1.0).to(DEV)


def _rect_targets(num, size, seed, num_classes=5, min_side=8):
    g = np.random.default_rng(seed)
    targets = []
    for T in num:
        masks = np.zeros((T, size, size), dtype=bool)
        for t in range(T):
            hh, ww = int(g.integers(min_side, size // 2)), int(g.integers(min_side, size // 2))
            y0, x0 = int(g.integers(0, size - hh)), int(g.integers(0, size - ww))
            masks[t, y0:y0 + hh, x0:x0 + ww] = True
        targets.append({"labels": torch.from_numpy(g.integers(0, num_classes, T)).to(DEV), "masks": torch.from_numpy(masks).to(DEV),
                        "boxes": torch.zeros(T, 4, device=DEV)})
    return targets


def test_same_draws_give_the_rows_of_the_torch_route():
    """the unchanged torch route (`noisy_rows`, reached through `_rng.install_replay`) fed with the restatement's u(r, j)
    against the native rows of the same (seed, draw): equal.  This also settles that the kernel's ratio is torch's."""
    from mp_former_amd import _rng, transformer_decoder as TD
    num, scalar, noise_scale, size = [3, 0, 5], 5, 0.2, 256
    sizes = [(8, 8), (16, 16), (32, 32), (16, 20)]           # (16 x 20 does not divide 256: gt_block_or's interpolate branch)
    targets = _rect_targets(num, size, seed=3)
    dec = _small_decoder()
    all_masks = torch.cat([t["masks"] for t in targets])
    bases = [TD.gt_block_or(all_masks, s).repeat(scalar, 1) for s in sizes]
    seed = 77
    draws = [4 * (i + 1) for i in range(len(sizes))]
    u = [torch.from_numpy(noise_u(seed, d, np.arange(b.shape[0]), b.shape[1])) for b, d in zip(bases, draws)]
    _rng.install_replay({"mp_noise": u})
    try:
        mp = dec._mp_setup({"tgt": targets, "scalar": scalar, "noise_scale": noise_scale}, len(num), sizes, DEV)
        torch_rows = [mp["rows"](lv) for lv in range(len(sizes))]
        assert _rng.remaining() == 0
    finally:
        _rng.install_replay(None)
    src_of, pad = src_of_table(num, scalar)
    src_of = torch.from_numpy(src_of).to(DEV)
    for lv, (b, d) in enumerate(zip(bases, draws)):
        native = TD.mp_noise_rows(b, src_of, len(num), pad, noise_scale, seed, d)
        assert native.shape == torch_rows[lv].shape and native.dtype == torch_rows[lv].dtype
        flips = int((native[0, :num[0]] != b[:num[0]]).sum())
        print(f"level {sizes[lv]}: {flips} flips in the first image's first copy")
        assert torch.equal(native, torch_rows[lv]), sizes[lv]


def test_rows_do_not_depend_on_the_launch_shape():
    base, src_of, N, pad = _case("scalar5_ragged")
    R, HW = base.shape
    seed, draw = 99, 16
    ref = _native(base, src_of, N, pad, 0.2, seed, draw).reshape(N * pad, HW)
    by_row = {int(r): ref[i] for i, r in enumerate(src_of) if r >= 0}
    assert len(by_row) == R
    # the rows permuted through src_of, in another N / pad (one image of R + 3 slots)
    perm = np.random.default_rng(0).permutation(R + 3).astype(np.int32)
    table = np.where(perm < R, perm, -1).astype(np.int32)
    got = _native(base, table, 1, R + 3, 0.2, seed, draw)[0]
    for i, r in enumerate(table):
        assert np.array_equal(got[i], by_row[int(r)] if r >= 0 else np.ones(HW, np.uint8)), (i, r)
    # a side stream
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        on_side = _native(base, src_of, N, pad, 0.2, seed, draw)
    torch.cuda.current_stream(DEV).wait_stream(side)
    assert np.array_equal(on_side.reshape(N * pad, HW), ref)
    # another draw, another seed: other rows
    nxt = _native(base, src_of, N, pad, 0.2, seed, draw + 4).reshape(N * pad, HW)
    other = _native(base, src_of, N, pad, 0.2, seed + 1, draw).reshape(N * pad, HW)
    for i, r in enumerate(src_of):
        if r >= 0 and (base[r] == 0).sum() * 0.2 >= 25:           # (a row with a few expected flips may repeat by chance)
            assert not np.array_equal(nxt[i], ref[i]) and not np.array_equal(other[i], ref[i])
    assert np.array_equal(nxt, noise_rows_ref(base, src_of, N, pad, 0.2, seed, draw + 4).reshape(N * pad, HW))


def test_flip_rate_within_the_binomial_bound():
    """config B's finest level, 200 rows: per row |k - p HW| <= 5 sqrt(HW p (1 - p)); no row excluded (check_flip_rate
    asserts that every instance is large enough for the normal bound)."""
    c = FLIP_CASE
    base = flip_case_rows()
    src_of, pad = src_of_table(list(c["num"]), c["scalar"])
    N = len(c["num"])
    got = _native(base, src_of, N, pad, c["noise_scale"], c["seed"], c["draw"]).reshape(N * pad, -1)
    assert (src_of >= 0).all() and sorted(src_of) == list(range(base.shape[0]))
    rows = np.empty_like(base)
    rows[src_of] = got
    check_flip_rate(base, rows, c["noise_scale"])


class _Spy:
    """counts and records the native calls of `rows` (every call runs with sync debug mode "error"), and the torch draws"""

    def __init__(self, monkeypatch):
        from mp_former_amd import _lib, _rng, transformer_decoder as TD
        self.calls, self.kernels, self.rand_tags = [], [], []
        orig_rows, orig_draw, orig_rand = TD.mp_noise_rows, TD._next_noise_draw, _rng.rand

        def strict(fn):
            def run(*a, **k):
                prev = torch.cuda.get_sync_debug_mode()
                torch.cuda.set_sync_debug_mode("error")
                try:
                    return fn(*a, **k)
                finally:
                    torch.cuda.set_sync_debug_mode(prev)
            return run

        def rows(base, src_of, N, pad, noise_scale, seed, draw, counts=None):
            out = strict(orig_rows)(base, src_of, N, pad, noise_scale, seed, draw, counts)
            self.kernels.append(_lib.last_kernel())
            self.calls.append(dict(base=base, src_of=src_of, N=N, pad=pad, seed=seed, draw=draw, out=out))
            return out

        def rand(tag, shape, device):
            self.rand_tags.append(tag)
            return orig_rand(tag, shape, device)

        monkeypatch.setattr(TD, "mp_noise_rows", rows)
        monkeypatch.setattr(TD, "_next_noise_draw", strict(orig_draw))
        monkeypatch.setattr(_rng, "rand", rand)


def test_head_at_config_B_takes_the_native_route(monkeypatch):
    """MPFormerHead at config-B feature shapes (1024 x 1024 image: levels 32^2 / 64^2 / 128^2), N = 2, scalar 5, noise 0.2,
    bf16 autocast, one forward + backward."""
    from mp_former_amd.head import MPFormerHead
    dec_layers, scalar, num, size = 9, 5, [20, 13], 1024
    torch.manual_seed(0)
    h = MPFormerHead(dec_layers=dec_layers, scalar=scalar, noise_scale=0.2).to(DEV).train()
    feats = {k: torch.randn(len(num), c, size // s, size // s, device=DEV).requires_grad_(True) for k, (c, s) in
             {"res2": (256, 4), "res3": (512, 8), "res4": (1024, 16), "res5": (2048, 32)}.items()}
    targets = _rect_targets(num, size, seed=1, num_classes=80, min_side=32)
    spy = _Spy(monkeypatch)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        losses, out = h(feats, targets)
    total = sum(losses.values())
    total.backward()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v)) for v in losses.values()) and bool(torch.isfinite(total))
    assert all(bool(torch.isfinite(f.grad).all()) for f in feats.values())
    assert out["dn_out"] is not None and out["dn_out"]["dn_args"]["pad_size"] == scalar * max(num)
    assert len(spy.calls) == dec_layers + 1, len(spy.calls)
    assert "mp_noise" not in spy.rand_tags, spy.rand_tags
    assert spy.kernels == [KERNEL] * (dec_layers + 1), spy.kernels
    want_table, pad = src_of_table(num, scalar)
    draws = [c["draw"] for c in spy.calls]
    assert len(set(draws)) == len(draws) and all(d % 4 == 0 for d in draws)
    for i, c in enumerate(spy.calls):
        HW = (32 << (i % 3)) ** 2
        assert c["N"] == len(num) and c["pad"] == pad and tuple(c["out"].shape) == (len(num), pad, HW)
        assert np.array_equal(c["src_of"].cpu().numpy(), want_table)
        assert c["seed"] == torch.cuda.default_generators[0].initial_seed()
    # the rows the layers saw are the contract's rows (first and finest level), and two masks of one level differ
    for i in (0, 2):
        c = spy.calls[i]
        want = noise_rows_ref(c["base"].view(torch.uint8).cpu().numpy(), want_table, len(num), pad, 0.2, c["seed"], c["draw"])
        assert np.array_equal(c["out"].view(torch.uint8).cpu().numpy(), want)
    assert not torch.equal(spy.calls[0]["out"], spy.calls[3]["out"])


def _small_head_run(monkeypatch):
    from mp_former_amd.head import MPFormerHead
    torch.manual_seed(0)
    h = MPFormerHead(num_classes=7, num_queries=10, enc_layers=1, dec_layers=4, num_points=112, scalar=2, noise_scale=0.2).to(DEV).train()
    size, num = 256, [3, 2]
    feats = {k: torch.randn(len(num), c, size // s, size // s, device=DEV) for k, (c, s) in
             {"res2": (256, 4), "res3": (512, 8), "res4": (1024, 16), "res5": (2048, 32)}.items()}
    targets = _rect_targets(num, size, seed=2, num_classes=7, min_side=48)
    spy = _Spy(monkeypatch)

    def forward():
        spy.calls.clear()
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            h(feats, targets)
        assert len(spy.calls) == 4 + 1            # levels 0, 1, 2, 0, 1
        return [c["out"].clone() for c in spy.calls]
    return forward


def test_manual_seed_and_generator_state_reproduce_the_rows(monkeypatch):
    forward = _small_head_run(monkeypatch)

    def same(a, b):
        return all(torch.equal(x, y) for x, y in zip(a, b))

    torch.manual_seed(1234)
    first = forward()
    state = torch.cuda.get_rng_state(DEV)
    second = forward()
    third = forward()
    assert not same(first, second) and not same(second, third), "consecutive forwards must draw fresh noise"
    assert not torch.equal(first[0], first[3]) and not torch.equal(first[1], first[4]), \
        "two masks of one forward at the same level must differ"
    torch.manual_seed(1234)
    assert same(forward(), first), "torch.manual_seed must reproduce the rows"
    torch.cuda.set_rng_state(state, DEV)
    assert same(forward(), second), "a restored generator state must reproduce the forward that followed it"
    torch.manual_seed(4321)
    assert not same(forward(), first)
