"""CPU side of the decoder layer with query positions (mp_former_amd/decoder_layer.py decoder_layer_pos): the fp64 reference the
GPU tests measure against is the layer nn.MultiheadAttention / nn.LayerNorm / nn.Linear compose when called as the clip decoder's
reference calls them; the single faults a position operand invites fall outside the bar of the GPU parity test; the arena
layout and the struct mirror are consistent."""
import ctypes

import pytest
import torch

from _decoder_layer_pos_common import ACTS, CASES, FAULTS, problem, ref_layer_pos, run_torch, tag
from test_decoder_layer_direct_gpu import E, EPS, H, NAMES, _judge, _seed_scale


@pytest.mark.parametrize("mp", [False, True])
def test_cpu_reference_matches_fp64_torch_modules(mp):
    """ref_layer_pos against the modules in fp64 with the same parameters, composed as video_mask2former_transformer_decoder.py
    composes them: cross-attention query = tgt + query_pos (:45-47), self-attention query = key = tgt + query_pos, value = tgt
    (:104-106).  The cross-attention module gets identity key / value projections (k_c / v_c are the projected ones).  Outputs and
    every gradient, d_qpos included, to 1e-10 of scale."""
    import torch.nn as nn
    Qt, N, S, F_ = 7, 3, 20, 96
    P = problem((Qt, N, S, F_, mp, None), seed=1)
    g = torch.Generator().manual_seed(5)
    prm = {n: torch.randn(t.shape, generator=g, dtype=torch.float64).mul_(0.3 if t.dim() == 1 else t.shape[1] ** -0.5).requires_grad_(True)
           for n, t in P["params"].items()}
    x, k_c, v_c = (torch.randn(s, N, E, generator=g, dtype=torch.float64).requires_grad_(True) for s in (Qt, S, S))
    qpos = torch.randn(Qt, E, generator=g, dtype=torch.float64).requires_grad_(True)
    go = torch.randn(Qt, N, E, generator=g, dtype=torch.float64)
    pr = qpos[:, None].expand(Qt, N, E)
    ref_layer_pos(x, pr, pr, k_c, v_c, P["mask_c"], P["mask_s"], prm, EPS).backward(go)
    want = {"x": x.grad, "qpos": qpos.grad, "k_c": k_c.grad, "v_c": v_c.grad, **{n: t.grad for n, t in prm.items()}}

    ca, sa = (nn.MultiheadAttention(E, H, dropout=0.0).double() for _ in range(2))
    n1, n2, n3 = (nn.LayerNorm(E, eps=EPS).double() for _ in range(3))
    l1, l2 = nn.Linear(E, F_).double(), nn.Linear(F_, E).double()
    eye, zero = torch.eye(E, dtype=torch.float64), torch.zeros(E, dtype=torch.float64)
    d = {n: t.detach() for n, t in prm.items()}
    with torch.no_grad():
        ca.in_proj_weight.copy_(torch.cat([d["ca_wq"], eye, eye]))
        ca.in_proj_bias.copy_(torch.cat([d["ca_bq"], zero, zero]))
        sa.in_proj_weight.copy_(torch.cat([d["sa_wq"], d["sa_wk"], d["sa_wv"]]))
        sa.in_proj_bias.copy_(torch.cat([d["sa_bq"], d["sa_bk"], d["sa_bv"]]))
        for m, blk in ((ca, "ca"), (sa, "sa")):
            m.out_proj.weight.copy_(d[blk + "_wo"])
            m.out_proj.bias.copy_(d[blk + "_bo"])
        for m, blk in ((n1, "ca"), (n2, "sa"), (n3, "ff")):
            m.weight.copy_(d[blk + "_gamma"])
            m.bias.copy_(d[blk + "_beta"])
        l1.weight.copy_(d["ff_w1"]); l1.bias.copy_(d["ff_b1"]); l2.weight.copy_(d["ff_w2"]); l2.bias.copy_(d["ff_b2"])
    xm, km, vm, pm = (t.detach().clone().requires_grad_(True) for t in (x, k_c, v_c, qpos))
    query_pos = pm.unsqueeze(1).repeat(1, N, 1)                                 # :396
    mc = P["mask_c"][:, None].expand(N, H, Qt, S).reshape(N * H, Qt, S)        # nn.MultiheadAttention: batch index n * H + h
    y1 = n1(xm + ca(query=xm + query_pos, key=km, value=vm, attn_mask=mc, need_weights=False)[0])
    qk = y1 + query_pos
    y2 = n2(y1 + sa(qk, qk, value=y1, attn_mask=P["mask_s"], need_weights=False)[0])
    y3 = n3(y2 + l2(torch.relu(l1(y2))))
    y3.backward(go)
    got = {"x": xm.grad, "qpos": pm.grad, "k_c": km.grad, "v_c": vm.grad,
           "ca_wq": ca.in_proj_weight.grad[:E], "ca_bq": ca.in_proj_bias.grad[:E],
           "sa_wq": sa.in_proj_weight.grad[:E], "sa_wk": sa.in_proj_weight.grad[E:2 * E], "sa_wv": sa.in_proj_weight.grad[2 * E:],
           "sa_bq": sa.in_proj_bias.grad[:E], "sa_bk": sa.in_proj_bias.grad[E:2 * E], "sa_bv": sa.in_proj_bias.grad[2 * E:],
           "ca_wo": ca.out_proj.weight.grad, "ca_bo": ca.out_proj.bias.grad, "sa_wo": sa.out_proj.weight.grad, "sa_bo": sa.out_proj.bias.grad,
           "ca_gamma": n1.weight.grad, "ca_beta": n1.bias.grad, "sa_gamma": n2.weight.grad, "sa_beta": n2.bias.grad,
           "ff_gamma": n3.weight.grad, "ff_beta": n3.bias.grad,
           "ff_w1": l1.weight.grad, "ff_b1": l1.bias.grad, "ff_w2": l2.weight.grad, "ff_b2": l2.bias.grad}
    assert set(got) == set(want) and len(got) == 4 + len(NAMES)
    with torch.no_grad():
        out = ref_layer_pos(x, pr, pr, k_c, v_c, P["mask_c"], P["mask_s"], prm, EPS)
    assert float((out - y3.detach()).abs().max()) <= 1e-10 * float(y3.detach().abs().max())
    for n in want:
        # (a key bias shifts all scores of a query alike: its gradient is zero, ~1e-16 on both sides — measured on the query bias's scale)
        scale = float(got["sa_bq" if n == "sa_bk" else n].abs().max())
        assert float((want[n] - got[n]).abs().max()) <= 1e-10 * scale, n
    assert float(want["sa_bk"].abs().max()) <= 1e-10 * float(want["sa_bq"].abs().max())


_torch_runs = {}


def _cpu_run(case, what):
    """fp64 reference / bf16 yardstick of a case on the CPU, once"""
    key = (case, what)
    if key not in _torch_runs:
        P = _torch_runs.setdefault((case, "problem"), problem(case))
        _torch_runs[key] = run_torch(P, torch.device("cpu"), what == "ref")
    return _torch_runs[key]


@pytest.mark.parametrize("fault", FAULTS)
def test_single_faults_fall_outside_the_parity_bar(fault):
    """Torch statements of the faulty math, exact in fp64, judged as the GPU parity test judges the native layer (``_judge``: every
    statistic <= 2 x torch's own bf16 composition against fp64 + 2^-9): each fault leaves at least one tensor outside its bar in
    at least one case.  qpos left out of the self-attention key; qpos added to the self-attention value; qpos indexed by r % Q
    instead of r / N; d_qpos from the self-attention operand only."""
    names = ("x3", "xb3") + ACTS + tuple("d_" + n for n in NAMES)
    failures = []
    for case in (CASES[1], CASES[2]):
        P = _torch_runs.setdefault((case, "problem"), problem(case))
        ref, yard = _cpu_run(case, "ref"), _cpu_run(case, "yard")
        got = run_torch(P, torch.device("cpu"), True, fault=fault)
        G = _seed_scale(P)
        for n in names:
            failures += _judge(f"{fault} {tag(case)}", n, got, ref, yard, ref, 0.0 if n in ("x3", "xb3") else G)
    assert failures, f"{fault}: every tensor of every case inside its bar"
    print("\n".join(failures))


def test_arena_layout_and_struct_mirror():
    """offsets of the saved tensors: 256-byte aligned, disjoint, in order, the position operands behind the image layer's tensors
    (whose offsets do not move); the total is the end of the last one; the mirror of MpfDecoderLayerPos is four pointers, the size
    the library reports."""
    from mp_former_amd import decoder_layer as DL
    for Qt, N, S, F_ in ((1, 1, 8, 32), (7, 3, 77, 96), (100, 2, 480, 2048)):
        R = Qt * N
        base, base_total = DL._arena_layout(R, E, N, S, Qt, H, F_)
        offs, total = DL._arena_layout(R, E, N, S, Qt, H, F_, True)
        assert len(base) == len(DL._SAVED) and len(offs) == len(DL._SAVED) + len(DL._SAVED_POS) == len(base) + 2
        assert offs[:len(base)] == base and offs[len(base)] == base_total
        assert all(o % 256 == 0 for o in offs) and total % 256 == 0
        ends = list(offs[1:]) + [total]
        assert all(b > a for a, b in zip(offs, ends))                                    # in order, so disjoint
        need = R * E * 2
        assert all(e - o >= need for o, e in zip(offs[len(base):], ends[len(base):]))    # each holds a bf16 [R, 256] operand
        assert total == base_total + 2 * ((need + 255) & ~255)
    assert [n for n, _ in DL.MpfDecoderLayerPos._fields_] == ["qpos", "xq0", "xq1", "d_qpos"]
    assert ctypes.sizeof(DL.MpfDecoderLayerPos) == 4 * ctypes.sizeof(ctypes.c_void_p)
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    assert _lib.lib().mpf_decoder_layer_pos_struct_bytes() == ctypes.sizeof(DL.MpfDecoderLayerPos)
    # the argument checks precede every HIP call: a NULL position operand is the library's NULL code, with nothing launched
    L, Pz = DL.MpfDecoderLayer(), DL.MpfDecoderLayerPos()
    assert _lib.lib().mpf_decoder_layer_pos_forward(ctypes.byref(L), None, None) == -3
    assert _lib.lib().mpf_decoder_layer_pos_forward(ctypes.byref(L), ctypes.byref(Pz), None) == -3
