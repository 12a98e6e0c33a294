"""CPU: the planner of the grouped bf16 convolution weight gradients (mpf_conv_wgrad_plan) on the 33 + 10 stride-1
convolutions of the bench backbone at config B (batch 2, 1024 x 1024), and the argument checks of the entry point, which
come before any launch."""
import ctypes

import pytest

SLOTS = 512            # two workgroups per compute unit of an MI355X


@pytest.fixture(scope="module")
def bb():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import backbone
    return backbone


def config_b_stages(bb):
    """{stage: [items in backward order]} — (R, Cout, Cin, kind, H, W) of every eligible convolution"""
    one, three = bb._CW_1X1, bb._CW_3X3
    stages = {}
    cin, side = 64, 256                        # after the stem and the max pool: 2 x 64 x 256 x 256
    for name, blocks, cmid, cout, stride in (("res2", 3, 64, 256, 1), ("res3", 4, 128, 512, 2), ("res4", 6, 256, 1024, 2),
                                             ("res5", 3, 512, 2048, 2)):
        fwd = []
        for b in range(blocks):
            s = stride if b == 0 else 1
            r_in, side_out = 2 * side * side, side // s
            r_out = 2 * side_out * side_out
            fwd.append((r_in, cmid, cin, one, side, side))                       # conv1 (the stride is in the 3x3)
            if s == 1 and cmid % 128 == 0:
                fwd.append((r_out, cmid, cmid, three, side_out, side_out))       # conv2
            fwd.append((r_out, cout, cmid, one, side_out, side_out))             # conv3
            if b == 0 and s == 1:
                fwd.append((r_in, cout, cin, one, side, side))                   # res2's shortcut
            cin, side = cout, side_out
        stages[name] = fwd[::-1]
    return stages


def make_items(bb, shapes):
    arr = (bb._CwItem * len(shapes))()
    for i, (R, Cout, Cin, kind, H, W) in enumerate(shapes):
        arr[i] = bb.conv_wgrad_item(R, Cout, Cin, kind, H, W)
    return arr


def test_config_b_has_33_plus_10_items(bb):
    st = config_b_stages(bb)
    kinds = [s[3] for v in st.values() for s in v]
    assert kinds.count(bb._CW_1X1) == 33 and kinds.count(bb._CW_3X3) == 10
    assert [len(st[k]) for k in ("res2", "res3", "res4", "res5")] == [7, 11, 17, 8]


@pytest.mark.parametrize("stage", ["res2", "res3", "res4", "res5"])
def test_plan_of_the_real_stage(bb, stage):
    shapes = config_b_stages(bb)[stage]
    items = make_items(bb, shapes)
    plans, ws_bytes = bb.conv_wgrad_plan(items, SLOTS)
    cap = bb._lib.lib().mpf_conv_wgrad_group_max()
    assert cap <= 12
    launches = -(-len(shapes) // cap)
    assert sorted({p.launch for p in plans}) == list(range(launches))
    assert [p.launch for p in plans] == sorted(p.launch for p in plans)
    spans = []
    per_launch = [0] * launches
    for (R, Cout, Cin, kind, H, W), it, p in zip(shapes, items, plans):
        K = Cin * (9 if kind == bb._CW_3X3 else 1)
        print(stage, (R, Cout, K), "rows_per_split", p.rows_per_split, "nsplit", p.nsplit, "workgroups", p.tiles, "launch", p.launch)
        assert p.rows_per_split > 0 and p.rows_per_split % 32 == 0
        assert it.rows_per_split == p.rows_per_split and it.ws_offset == p.ws_offset        # copied into the item
        assert p.nsplit == -(-R // p.rows_per_split)
        assert p.tiles == -(-Cout // 128) * -(-K // 128) * p.nsplit
        part_bytes = 4 * p.nsplit * Cout * K
        assert part_bytes <= p.ws_bytes and p.ws_offset % 256 == 0
        assert part_bytes <= 2 * R * (Cout + K), "partial sums above the operand bytes"
        spans.append((p.ws_offset, p.ws_offset + p.ws_bytes))
        per_launch[p.launch] += p.tiles
    spans.sort()
    assert spans[0][0] == 0 and spans[-1][1] == ws_bytes
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "workspace slices overlap"
    print(stage, "workgroups per launch", per_launch)
    # one to three rounds of the slots, and whole ones: a last round under 80 % full would idle a fifth of the chip for the
    # length of a split
    for wgs in per_launch:
        rounds = -(-wgs // SLOTS)
        assert 1 <= rounds <= 3
        assert wgs >= 0.8 * rounds * SLOTS


def test_plan_balances_rows_per_workgroup(bb):
    """items with 16 x the rows get about 16 x the splits: every workgroup contracts about the same number of rows (where the
    partial-sum cap does not bind)"""
    items = make_items(bb, [(131072, 64, 64, 0, 0, 0), (8192, 64, 64, 0, 0, 0)])
    plans, _ = bb.conv_wgrad_plan(items, SLOTS)
    assert plans[0].nsplit > plans[1].nsplit >= 1
    assert 0.5 <= plans[0].rows_per_split / plans[1].rows_per_split <= 2.0


def test_argument_errors_without_a_gpu(bb):
    lib = bb._lib.lib()
    one = ctypes.c_void_p(256)                # never dereferenced: the checks come first

    def item(R=256, Cout=64, Cin=128, kind=0, H=0, W=0, rps=32):
        it = bb.conv_wgrad_item(R, Cout, Cin, kind, H, W)
        it.dy = it.x = it.scale = it.out = 256
        it.rows_per_split = rps
        return it

    def run(it, ws_bytes=1 << 30):
        arr = (bb._CwItem * 1)(it)
        return lib.mpf_conv_wgrad_bf16_grouped(arr, 1, one, ws_bytes, None)

    assert run(item(rps=48)) != 0 and b"multiple of 32" in lib.mpf_last_error()
    assert run(item(rps=0)) != 0
    assert run(item(Cin=64, kind=1, H=16, W=16)) != 0 and b"Cin % 128" in lib.mpf_last_error()
    assert run(item(kind=1, H=16, W=12, R=192)) != 0
    assert run(item(kind=1, H=16, W=16, R=200)) != 0          # not whole images
    assert run(item(Cin=42)) != 0
    assert run(item(kind=7)) != 0
    assert run(item(), ws_bytes=1024) != 0 and b"workspace" in lib.mpf_last_error()
    bad = item()
    bad.out = None
    assert run(bad) != 0
    plans = (bb._CwPlan * 1)()
    ws = ctypes.c_size_t(0)
    arr = (bb._CwItem * 1)(item(Cin=64, kind=1, H=16, W=16))
    assert lib.mpf_conv_wgrad_plan(arr, 1, SLOTS, plans, ctypes.byref(ws)) != 0
    assert lib.mpf_conv_wgrad_plan(None, 1, SLOTS, plans, ctypes.byref(ws)) != 0
