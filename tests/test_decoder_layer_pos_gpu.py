"""``decoder_layer_pos()`` (mp_former_amd/decoder_layer.py, csrc/decoder_layer.hip with csrc/query_pos.hip) called directly: the
one-call decoder layer with learned query positions, forward and every gradient against the fp64 reference of
tests/_decoder_layer_pos_common.py and against the op-by-op composition of the clip decoder, at the smallest shapes that reach
each branch (one row; the three-GEMM form; strided key / value column blocks with the packed dK / dV; many queries of one image;
the clip shape of the bench width).  The single faults a position operand invites are shown to fall outside the same bar in
tests/test_decoder_layer_pos_cpu.py."""
import ctypes

import pytest
import torch

from _decoder_layer_pos_common import (ACTS, CASES, UNPACKED, forward_native, problem, run_by_ops, run_native, run_torch, tag)
from test_decoder_layer_direct_gpu import E, NAMES, _judge, _seed_scale

gpu = pytest.mark.gpu

_cache = {}


def _shared(case, what):
    """problem, fp64 reference, bf16 yardstick and native results of a case, computed once (read only)"""
    key = (case, what)
    if key not in _cache:
        dev = torch.device("cuda:0")
        P = _cache.setdefault((case, "problem"), problem(case))
        if what == "ref":
            _cache[key] = run_torch(P, dev, True)
        elif what == "yard":
            _cache[key] = run_torch(P, dev, False)
        elif what == "native":
            _cache[key] = run_native(P, dev, packed=case != UNPACKED)
    return _cache[key]


@gpu
@pytest.mark.parametrize("case", CASES, ids=tag)
def test_layer_matches_fp64_reference(case):
    """x3, xb3, d_x0, d_qpos, d_k_c, d_v_c and the 22 parameter gradients of the native layer against fp64 autograd through
    ref_layer_pos, all three gradient operands present, at the bar of ``_judge`` (every statistic <= 2 x torch's own bf16
    composition of the layer with positions against fp64 + 2^-9, with its two vanishing-reference clauses).  Measured on an
    MI355X over the five cases (native | torch bf16; the lines this test prints):
      x3 / xb3 rows            median 0.0025-0.0038 | 0.0025-0.0046, p99 <= 0.0045 | 0.0063, max <= 0.0050 | 0.0071
      d_x0 rows                median 0.0025-0.027  | 0.0025-0.031,  p99 <= 0.098  | 0.117,  max <= 0.118  | 0.140
      d_qpos                   l2 0.009-0.030 | 0.032-0.038, rows: median <= 0.029 | 0.036, p99 <= 0.084 | 0.116, max <= 0.151 | 0.193
      d_k_c / d_v_c rows       median <= 0.029      | <= 0.035,      p99 <= 0.131  | 0.194,  max <= 0.190  | 0.316
      parameter tensors (l2)   <= 0.033 | <= 0.042 (d_ff_w1 / d_ff_b1, behind the ReLU gate: <= 0.051 | 0.064)
      weight rows              median 0.003-0.031 | 0.003-0.039, p99 <= 0.085 | 0.140, max <= 0.123 | 0.243 (d_ff_w1: max <= 0.62 | 0.79)
      d_sa_bk (zero gradient)  residue / |d_sa_bq| 0.0046-0.0057 | 0.0024-0.0029 (bar 0.06-0.09)
      Qt = 1                   d_qpos, d_k_c and the query / key projections' gradients vanish in the reference: native max-abs
                               <= 9.4e-7 (fp32 round-off of terms that cancel, allowed 2^-16 of the seed's scale), torch bf16 0
    i.e. the native layer sits where torch's own bf16 composition sits, tensor by tensor, d_qpos included."""
    P = _cache.setdefault((case, "problem"), problem(case))
    ref, yard, got = _shared(case, "ref"), _shared(case, "yard"), _shared(case, "native")
    G, t = _seed_scale(P), tag(case)
    assert got["alias"]
    assert torch.equal(got["xb3"], got["x3"].bfloat16())
    bad = []
    for n in ("x3", "xb3") + ACTS + tuple("d_" + n for n in NAMES):
        bad += _judge(t, n, got, ref, yard, ref, 0.0 if n in ("x3", "xb3") else G)
    if case[5] is not None:                 # the column blocks of the packed gradient that are not this layer's: zero, not stale
        j = case[5][0]
        for n in ("d_Kp", "d_Vp"):
            others = [got[n][..., c * E:(c + 1) * E] for c in range(3) if c != j]
            assert all(bool((o == 0).all()) for o in others), n
    assert not bad, "\n".join(bad)


@gpu
@pytest.mark.parametrize("case", CASES, ids=tag)
def test_fused_layer_equals_the_op_by_op_composition(case):
    """Same kernels, same rounding points as ``_layer_by_ops`` of the clip decoder: the forward bit for bit; every gradient
    tensor, d_qpos included, to relative L2 2e-2 (the order of bf16 accumulation differs, as for the image layer)."""
    P = _cache.setdefault((case, "problem"), problem(case))
    got, ops = _shared(case, "native"), run_by_ops(P, torch.device("cuda:0"))
    assert torch.equal(got["x3"], ops["x3"]) and torch.equal(got["xb3"], ops["xb3"])
    G, bad = _seed_scale(P), []
    for n in ACTS + tuple("d_" + n for n in NAMES):
        a, b = got[n].double(), ops[n].double()
        if max(float(a.abs().max()), float(b.abs().max())) < 2.0 ** -16 * G:       # round-off where the gradient vanishes (see _judge)
            continue
        # (the key bias's gradient is zero, both sides hold rounding residue: measured on the scale of its sibling, see _judge)
        rel = float((a - b).norm() / (ops["d_sa_bq"].double().norm() if n == "d_sa_bk" else b.norm()))
        print(f"[layer pos] {tag(case)} fused vs ops {n}: {rel:.2e}")
        if not rel < 2e-2:
            bad.append((n, rel))
    assert not bad, bad


@gpu
@pytest.mark.parametrize("option,values", [("decoder_dw_group", (2, 1, 0)), ("decoder_row_chain", (1, 0))])
def test_options_are_bit_identical(option, values):
    """the weight gradients as one grouped launch on transposed copies / one grouped launch / separate launches, and the row
    chains against their separate launches: the same bits, outputs and every gradient, as for the image layer"""
    from mp_former_amd import _lib
    dev = torch.device("cuda:0")
    case = CASES[2]
    P = _cache.setdefault((case, "problem"), problem(case))
    runs = []
    try:
        for v in values:
            _lib.set_option(option, v)
            runs.append(run_native(P, dev))
    finally:
        _lib.set_option(option, values[0])
    for other in runs[1:]:
        for n, t in runs[0].items():
            if n != "alias":
                assert torch.equal(t, other[n]), (option, n)


@gpu
def test_null_position_operand_is_rejected_before_any_launch():
    """a NULL qpos (or a missing record) returns the library's NULL code; nothing is launched"""
    from mp_former_amd import _lib
    from mp_former_amd import decoder_layer as DL
    dev = torch.device("cuda:0")
    P = _cache.setdefault((CASES[0], "problem"), problem(CASES[0]))
    T = forward_native(P, dev)
    node = T["outs"][0].grad_fn
    L, Pz = node.layer, node.pos
    lib = _lib.lib()
    _lib.profile_enable(True)
    try:
        n0 = _lib.profile_get("")[0]
        last = _lib.last_kernel()
        bad = DL.MpfDecoderLayerPos()
        bad.xq0, bad.xq1, bad.d_qpos = Pz.xq0, Pz.xq1, Pz.xq0
        G = DL.MpfDecoderLayerGrad()
        assert lib.mpf_decoder_layer_pos_forward(ctypes.byref(L), ctypes.byref(bad), None) == -3
        assert lib.mpf_decoder_layer_pos_forward(ctypes.byref(L), None, None) == -3
        assert lib.mpf_decoder_layer_pos_backward(ctypes.byref(L), ctypes.byref(bad), ctypes.byref(G), None) == -3
        assert b"MpfDecoderLayerPos" in lib.mpf_last_error()
        assert _lib.profile_get("")[0] == n0 and _lib.last_kernel() == last
    finally:
        _lib.profile_enable(False)
