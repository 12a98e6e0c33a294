"""GPU: the 256-channel residual LayerNorm family against the per-element fp64 references of tests/_resln_cases.py, through the C ABI
(mpf_res_ln256_forward / _forward_b, every mpf_res_ln256_backward* entry, mpf_ln_partial_reduce, mpf_lin256_res_ln_forward,
mpf_ln256_mlp3_forward) and through the autograd wrapper (resln.res_ln).  The problems, bounds and check functions are that file's;
tests/test_resln_cases_cpu.py holds them to the library's grid rule and to aten, and shows that each of 15 single faults fails them.

  forward    every FWD_CASES row: all outputs; y16 alone with s_out NULL (same bits); _forward_b (same bits, both bound slots exact)
  backward   every BWD_CASES row in the four forms (atomics, _ws, _partial + mpf_ln_partial_reduce, _det up to 1028 rows): ds32, ds16,
             dgamma, dbeta per element; _ws_amax / _partial_amax write the bits of the calls without the slot and max|ds32| exactly;
             _partial + reduce equals _ws bit for bit; _det leaves its ticket word zero, repeats its bits on a second call and is
             within (D_det + D_ws) u S of _ws; the large-mean rows are within 4 x the error of aten's fp32 backward on this device
  exact      the integer problem at every backward row count in the four forms: ds32, dgamma, dbeta equal fp64 exactly
  reduce     three slots a stride larger than the slot apart: each output equals the single-slot reduce, the gaps stay untouched
  wrapper    res_ln at 1024 / 1025 rows (the _det / _ws switch), t in {None, fp32, bf16}, the three output requests, std and m40,
             against fp64 F.layer_norm(x + t) with autograd
  chains     mpf_lin256_res_ln_forward per element; mpf_ln256_mlp3_forward bit-equal to the four launches it replaces
Every input is NaN behind what a call addresses, every output a sentinel that must survive there.  Every comparison prints its
worst err / bound (`pytest -s`); no element is excluded.

Worst err / bound seen per quantity (one MI355X run, all cases passing; nothing is asserted about these beyond <= 1).  K = 8, the y32
form as stated at KY = 64 (tests/_resln_cases.py, Y FORM); dgamma / dbeta relative to K + D:
  route                        mean   rstd   y32    y32 + sigma term  ds32 / dx  dgamma dbeta  s_out  ds err / aten's (bar 4)
  C ABI, every entry           0.309  0.227  0.199  0.422             0.258      0.037  0.146         1.16
  res_ln (autograd)                          0.519  0.324             0.364      0.008  0.009         0.98
  mpf_lin256_res_ln_forward    0.040  0.219  0.064  0.255                                      0.918
_det against _ws: 0.027 (dgamma), 0.033 (dbeta) of (D_det + D_ws) u S.  A bf16 output checked without its fp32 twin (y16 or ds16
alone, the bf16 gradient of t) sits at 0.995: that is the rounding to bf16 just above a power of two, not the arithmetic.  The
wrapper's 0.519 of KY is 33 of the y32 form at K = 1, at an element with |s| + |mu| << sigma: the reason for KY.  The exact problem
was exact in all four forms at all twelve row counts.  No bug was found in csrc/elementwise.hip, csrc/row_chain.hip or resln.py: every
test passed on the kernels as they were.
"""
import pytest
import torch
import torch.nn.functional as F

import _resln_cases as RC

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C = RC.C
F32, F64, BF16 = RC.F32, RC.F64, RC.BF16


def _dev(t):
    return t.to(DEV) if t is not None else None


def _params(pb, beta=True):
    return _dev(RC.inbuf(pb.gamma)), (_dev(RC.inbuf(pb.beta)) if beta else None)


def _cpu(ns):
    for k, v in vars(ns).items():
        if torch.is_tensor(v):
            setattr(ns, k, v.cpu())
    return ns


# ---- forward -----------------------------------------------------------------------------------------------------------------------------------
def _forward(pb, want, bounds=False):
    from mp_former_amd import _lib, gemm3 as g
    x, t, padd = _dev(pb.x_buf), _dev(pb.t_buf), _dev(pb.padd_buf)
    gamma, beta = _params(pb)
    out = RC.fwd_buffers(pb, want)
    for k in ("s_out", "y32", "y16", "y_plus", "mean", "rstd"):
        setattr(out, k, _dev(getattr(out, k)))
    args = (x.data_ptr(), _lib.ptr(t), _lib.DTYPE[t.dtype] if t is not None else 0, gamma.data_ptr(), beta.data_ptr(), _lib.ptr(out.s_out),
            _lib.ptr(out.y32), _lib.ptr(out.y16), out.mean.data_ptr(), out.rstd.data_ptr(), pb.rows, pb.eps, _lib.ptr(padd), pb.padd_rows,
            _lib.ptr(out.y_plus))
    if bounds:
        slots = g.amax_slots(2, DEV)
        padd_amax = g.amax(_dev(pb.padd).contiguous()) if out.y_plus is not None else None
        _lib.call("mpf_res_ln256_forward_b", DEV, *args, slots[0].data_ptr(), _lib.ptr(padd_amax),
                  slots[1].data_ptr() if out.y_plus is not None else None, _lib.stream_ptr(DEV))
        out.y_bound, out.yplus_bound = g.amax_value(slots[0]).cpu(), g.amax_value(slots[1]).cpu()
    else:
        _lib.call("mpf_res_ln256_forward", DEV, *args, _lib.stream_ptr(DEV))
    assert _lib.last_kernel() == "res_ln256_fwd_kernel", _lib.last_kernel()
    return _cpu(out)


@pytest.mark.parametrize("name", list(RC.FWD_CASES))
def test_forward_every_entry_against_fp64(name):
    pb = RC.fwd_problem(name)
    full = _forward(pb, ("s_out", "y32", "y16", "y_plus"))
    frac = RC.check_forward(pb, full, route="all outputs")
    assert {"mean", "rstd", "y32", "y32_sigma"} <= set(frac)
    # y16 alone, s_out NULL: the same bits as the y16 of the call with both
    only16 = _forward(pb, ("y16",))
    assert only16.s_out is None and only16.y32 is None
    RC.check_forward(pb, only16, route="y16 only, s_out NULL")
    for q in ("y16", "mean", "rstd"):
        assert RC.same_bits(getattr(only16, q), getattr(full, q)), (name, q)
    # y32 alone
    only32 = _forward(pb, ("y32", "y_plus"))
    RC.check_forward(pb, only32, route="y32 only, s_out NULL")
    assert RC.same_bits(only32.y32, full.y32)
    # _forward_b: the same bits, and the bound slots
    b = _forward(pb, ("s_out", "y32", "y16", "y_plus"), bounds=True)
    for q in ("s_out", "y32", "y16", "y_plus", "mean", "rstd"):
        assert (getattr(b, q) is None and getattr(full, q) is None) or RC.same_bits(getattr(b, q), getattr(full, q)), (name, q)
    yb, ypb = RC.y_bounds(pb)
    assert RC.same_bits(b.y_bound.reshape(1), yb.reshape(1)), (name, float(b.y_bound), float(yb))
    if pb.padd_rows:
        assert RC.same_bits(b.yplus_bound.reshape(1), ypb.reshape(1)), (name, float(b.yplus_bound), float(ypb))


# ---- backward ----------------------------------------------------------------------------------------------------------------------------------
def _upload_bwd(pb):
    d = RC.SimpleNamespace(s=_dev(pb.s_buf), mean=_dev(pb.mean_buf), rstd=_dev(pb.rstd_buf), gamma=_params(pb, beta=False)[0],
                           gy32=_dev(pb.gy32_buf), gy16=_dev(pb.gy16_buf), gyp=_dev(pb.gyp_buf))
    return d


def _backward(pb, d, form, ds=None, amax=False, det_ws=None):
    """one backward call of ``form`` -> its output buffers on the CPU (``partials``: the workspace behind the ticket word; ``ticket``)"""
    from mp_former_amd import _lib, gemm3 as g
    out = RC.bwd_buffers(pb, form, ds)
    ds32, ds16, dgamma, dbeta = _dev(out.ds32), _dev(out.ds16), _dev(out.dgamma), _dev(out.dbeta)
    head = (d.s.data_ptr(), d.mean.data_ptr(), d.rstd.data_ptr(), d.gamma.data_ptr(), _lib.ptr(d.gy32), _lib.ptr(d.gy16), _lib.ptr(d.gyp),
            _lib.ptr(ds32), _lib.ptr(ds16))
    floats, st = pb.blocks * 512, _lib.stream_ptr(DEV)
    assert floats * 4 == RC.workspace_bytes(pb.rows) == _lib.lib().mpf_res_ln256_backward_workspace_bytes(pb.rows)
    slot = g.amax_slots(1, DEV)[0] if amax else None
    tail = (slot.data_ptr(),) if amax else ()
    suffix = "_amax" if amax else ""
    out.partials = out.ticket = None
    if form == "atomic":
        assert not amax
        _lib.call("mpf_res_ln256_backward", DEV, *head, dgamma.data_ptr(), dbeta.data_ptr(), pb.rows, st)
    elif form == "ws":
        ws = _dev(RC.outbuf(floats))
        _lib.call("mpf_res_ln256_backward_ws" + suffix, DEV, *head, dgamma.data_ptr(), dbeta.data_ptr(), pb.rows, ws.data_ptr(), floats * 4, *tail, st)
        out.partials = ws
    elif form == "partial":
        part, red = _dev(RC.outbuf(floats)), _dev(RC.outbuf(2 * C))
        _lib.call("mpf_res_ln256_backward_partial" + suffix, DEV, *head, pb.rows, part.data_ptr(), floats * 4, *tail, st)
        kernel = _lib.last_kernel()
        _lib.call("mpf_ln_partial_reduce", DEV, part.data_ptr(), floats * 4, pb.rows, 1, red.data_ptr(), st)
        assert kernel == _lib.last_kernel()                      # (the reduce names no kernel)
        out.partials = part
        dgamma, dbeta = torch.cat([red[:C], red[2 * C:]]), red[C:]
    else:
        assert not amax and RC.det_workspace_bytes(pb.rows) == _lib.lib().mpf_res_ln256_backward_det_workspace_bytes(pb.rows)
        ws = det_ws if det_ws is not None else _dev(torch.cat([torch.zeros(64), RC.outbuf(floats)]))
        dgb = _dev(RC.outbuf(2 * C))
        _lib.call("mpf_res_ln256_backward_det", DEV, *head, dgb.data_ptr(), pb.rows, ws.data_ptr(), 256 + floats * 4, st)
        out.det_ws, out.partials, out.ticket = ws, ws[64:], int(ws[:1].view(torch.int32).item())
        dgamma, dbeta = torch.cat([dgb[:C], dgb[2 * C:]]), dgb[C:]
    assert _lib.last_kernel() == "res_ln256_bwd_kernel", _lib.last_kernel()
    out.ds32, out.ds16, out.dgamma, out.dbeta = ds32, ds16, dgamma, dbeta
    out.ds_amax = float(g.amax_value(slot)) if amax else None
    det = getattr(out, "det_ws", None)
    out = _cpu(out)
    out.det_ws = det
    if out.partials is not None:
        RC.take(f"bwd {pb.name} {form}", "partials", out.partials, floats)
    return out


def _same(a, b, names, what):
    for q in names:
        x, y = getattr(a, q), getattr(b, q)
        assert (x is None and y is None) or RC.same_bits(x, y), (what, q)


def _forms(pb):
    return [f for f in RC.FORMS if f != "det" or pb.rows <= RC.DET_MAX_ROWS]


@pytest.mark.parametrize("name", list(RC.BWD_CASES))
def test_backward_every_form_against_fp64(name):
    pb, ref = RC.bwd_case(name)
    d = _upload_bwd(pb)
    outs = {form: _backward(pb, d, form) for form in _forms(pb)}
    for form, out in outs.items():
        RC.check_backward(pb, ref, out, form)
    # the base every output subset is compared with: the same form with both ds outputs
    base = _backward(pb, d, "ws", ds="ds32+ds16")
    RC.check_backward(pb, ref, base, "ws", route="ds32+ds16")
    for form, out in outs.items():
        for q in ("ds32", "ds16"):
            assert getattr(out, q) is None or RC.same_bits(getattr(out, q), getattr(base, q)), (name, form, q)
    _same(outs["partial"], outs["ws"], ("dgamma", "dbeta", "partials"), f"{name}: _partial + reduce against _ws")
    # the amax entries: the bits of the calls without the slot, and max|ds32| exactly (of the base where this call writes ds16 alone)
    for form in ("ws", "partial"):
        a = _backward(pb, d, form, amax=True)
        _same(a, outs[form], ("ds32", "ds16", "dgamma", "dbeta", "partials"), f"{name}: {form}_amax against {form}")
        assert a.ds_amax == float(RC.take(name, "ds32", base.ds32, pb.rows * C).abs().max()), (name, form, a.ds_amax)
        a.ds_amax = a.ds_amax if a.ds32 is not None else None
        RC.check_backward(pb, ref, a, form, route="amax entry")
    if "det" in outs:
        det, ws = outs["det"], outs["ws"]
        assert det.ticket == 0, (name, det.ticket)
        again = _backward(pb, d, "det", det_ws=det.det_ws)
        assert again.ticket == 0
        _same(again, det, ("ds32", "ds16", "dgamma", "dbeta"), f"{name}: second _det call on the same workspace")
        kd = RC.depth("det", pb.rows) + RC.depth("ws", pb.rows)
        for q in ("dgamma", "dbeta"):
            RC.hold(f"bwd {name}", f"{q}: _det against _ws", getattr(det, q)[:C], getattr(ws, q)[:C].to(F64), getattr(ref, "b_" + q), kd)
    if bool(pb.large.any()) and base.ds32 is not None:
        ds_aten = RC.aten_backward(pb, DEV)[0]
        RC.check_vs_aten(pb, ref, base.ds32[:pb.rows * C].view(pb.rows, C), ds_aten, route="_ws")


@pytest.mark.parametrize("rows", [5, 132])
def test_backward_on_the_moments_the_forward_kernel_wrote(rows):
    """mixed rows: mean / rstd come from mpf_res_ln256_forward instead of the fp64 moments; the reference takes them as given"""
    fw = RC.fwd_problem(f"mix r{rows} feeds the backward", rows=rows, dist="mix", t="none", padd_rows=0)
    f = _forward(fw, ("s_out", "y32"))
    RC.check_forward(fw, f, route="all outputs")
    pb = RC.bwd_problem(f"mix r{rows} fed by the forward", rows=rows, dist="mix", ops="gy32+gy16", ds="ds32+ds16")
    pb.s, pb.large = fw.x, fw.large
    pb.mean, pb.rstd = f.mean[:rows].clone(), f.rstd[:rows].clone()
    pb = RC._finish_bwd(pb)
    ref = RC.bwd_reference(pb)
    d = _upload_bwd(pb)
    for form in _forms(pb):
        out = _backward(pb, d, form)
        RC.check_backward(pb, ref, out, form, route="forward's moments")
    RC.check_vs_aten(pb, ref, out.ds32[:rows * C].view(rows, C), RC.aten_backward(pb, DEV)[0], route="forward's moments")


@pytest.mark.parametrize("rows", list(RC.BWD_ROWS))
def test_exact_problem_counts_every_row_once_in_every_form(rows):
    pb, ref = RC.exact_case(rows)
    d = _upload_bwd(pb)
    outs = {form: _backward(pb, d, form) for form in _forms(pb)}
    for form, out in outs.items():
        RC.check_exact(pb, ref, out, form)
    if "det" in outs:
        assert outs["det"].ticket == 0
        _same(outs["det"], outs["ws"], ("ds32", "dgamma", "dbeta"), f"exact r{rows}: _det against _ws")


@pytest.mark.parametrize("rows", [125, 900])
def test_reduce_of_three_slots_with_a_stride_larger_than_the_slot(rows):
    from mp_former_amd import _lib
    names = ("std", "m40", "big") if rows == 125 else ("mix", "mix", "mix")
    slot, gap = RC.grid_rule(rows)[1] * 512, 64
    stride = slot + gap
    buf = _dev(RC.outbuf(3 * stride))
    single, st = [], _lib.stream_ptr(DEV)
    for z, dist in enumerate(names):
        pb = RC.bwd_problem(f"reduce slot {z}", rows=rows, dist=dist, ops="gy32", ds="ds32")
        d = _upload_bwd(pb)
        single.append(_backward(pb, d, "partial"))
        ds32 = _dev(RC.outbuf(rows * C))
        _lib.call("mpf_res_ln256_backward_partial", DEV, d.s.data_ptr(), d.mean.data_ptr(), d.rstd.data_ptr(), d.gamma.data_ptr(), d.gy32.data_ptr(),
                  None, None, ds32.data_ptr(), None, rows, buf.data_ptr() + z * stride * 4, slot * 4, st)
        assert RC.same_bits(ds32.cpu(), single[z].ds32)
    out = _dev(RC.outbuf(3 * 2 * C))
    _lib.call("mpf_ln_partial_reduce", DEV, buf.data_ptr(), stride * 4, rows, 3, out.data_ptr(), st)
    # the partials are where the three calls put them, the gaps between the slots and the tail are untouched
    got = buf.cpu()
    for z in range(3):
        assert RC.same_bits(got[z * stride:z * stride + slot], single[z].partials[:slot]), z
        behind = got[z * stride + slot:(z + 1) * stride] if z < 2 else got[z * stride + slot:]
        assert RC.same_bits(behind, RC.outbuf(0, pad=behind.numel())), f"the gap behind slot {z} was written"
    res = RC.take("reduce", "out", out.cpu(), 3 * 2 * C).view(3, 2, C)
    for z in range(3):
        assert RC.same_bits(res[z, 0], single[z].dgamma[:C]) and RC.same_bits(res[z, 1], single[z].dbeta[:C]), z


# ---- the autograd wrapper ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want", [(True, False), (False, True), (True, True)], ids=["y32", "y16", "y32+y16"])
@pytest.mark.parametrize("t_kind", ["none", "f32", "bf16"])
@pytest.mark.parametrize("dist", ["std", "m40"])
@pytest.mark.parametrize("rows", RC.WRAPPER_ROWS)
def test_res_ln_wrapper_against_fp64_autograd(rows, dist, t_kind, want):
    from mp_former_amd import _lib
    from mp_former_amd.resln import res_ln
    want32, want16 = want
    name = f"wrapper {dist} r{rows} t={t_kind} {'y32' if want32 else ''}{'+y16' if want16 else ''}"
    pb = RC.fwd_problem(name, rows=rows, dist=dist, t=t_kind, padd_rows=0)
    g = RC._gen(name + " gy")
    g32 = torch.randn(rows, C, generator=g) if want32 else None
    g16 = torch.randn(rows, C, generator=g).to(BF16) if want16 else None
    norm = torch.nn.LayerNorm(C, eps=1e-5).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(pb.gamma)
        norm.bias.copy_(pb.beta)
    x = pb.x.to(DEV).requires_grad_(True)
    t = pb.t.to(DEV).requires_grad_(True) if pb.t is not None else None
    y32, y16 = res_ln(norm, x, t, want32, want16)
    assert _lib.last_kernel() == "res_ln256_fwd_kernel" and (y32 is not None) == want32 and (y16 is not None) == want16
    leaves = [x, norm.weight, norm.bias] + ([t] if t is not None else [])
    grads = torch.autograd.grad([y for y in (y32, y16) if y is not None], leaves, [_dev(v) for v in (g32, g16) if v is not None])
    assert _lib.last_kernel() == "res_ln256_bwd_kernel"
    # fp64: F.layer_norm(x + t) with autograd
    x64 = pb.x.to(F64).requires_grad_(True)
    t64 = pb.t.to(F64).requires_grad_(True) if pb.t is not None else None
    gm64, bt64 = pb.gamma.to(F64).requires_grad_(True), pb.beta.to(F64).requires_grad_(True)
    s64 = x64 if t64 is None else x64 + t64
    y64 = F.layer_norm(s64, (C,), gm64, bt64, RC.EPS)
    gsum = sum(v.to(F64) for v in (g32, g16) if v is not None)
    r64 = torch.autograd.grad(y64, [x64, gm64, bt64] + ([t64] if t64 is not None else []), gsum)
    y64 = y64.detach()
    # the bounds: the forward forms on the fp32 s, the backward forms with that s and its fp64 moments
    fr = RC.fwd_reference(pb.s, pb.gamma, pb.beta)
    q = RC.SimpleNamespace(s=pb.s, mean=fr.mean, rstd=fr.rstd, gamma=pb.gamma, gy32=g32, gy16=g16, gy_plus=None)
    br = RC.bwd_reference(q)
    K = RC.K
    if want32:
        RC.hold(name, "y32", y32, y64, fr.b_y, RC.KY)
        RC.hold(name, "y32 (sigma form)", y32, y64, fr.b_y_sigma, K)
        if want16:
            assert RC.same_bits(y16.cpu(), y32.cpu().to(BF16)), f"{name}: y16 is not the rounded y32"
    else:
        RC.hold(name, "y16", y16, y64, fr.b_y_sigma + 2.0 ** -8 * y64.abs() / K, K)
    RC.hold(name, "dx", grads[0], r64[0], br.b_ds, K)
    if t is not None:
        assert grads[3].dtype == pb.t.dtype
        extra = 2.0 ** -8 * r64[3].abs() / K if t_kind == "bf16" else 0.0            # its one rounding to bf16
        RC.hold(name, "dt", grads[3], r64[3], br.b_ds + extra, K)
        if t_kind == "f32":
            assert RC.same_bits(grads[3].cpu(), grads[0].cpu())
    kd = K + RC.depth("det" if rows <= 1024 else "ws", rows)
    RC.hold(name, "dgamma", grads[1], r64[1], br.b_dgamma, kd)
    RC.hold(name, "dbeta", grads[2], r64[2], br.b_dbeta, kd)
    if dist == "m40":                                           # the large-mean rule, against aten's fp32 LayerNorm on this device
        xa = pb.s.to(DEV).requires_grad_(True)
        ya = F.layer_norm(xa, (C,), _dev(pb.gamma), _dev(pb.beta), RC.EPS)
        dxa = torch.autograd.grad(ya, xa, _dev(gsum.to(F32)))[0]
        e, ea = float((grads[0].cpu().to(F64) - r64[0]).abs().max()), float((dxa.cpu().to(F64) - r64[0]).abs().max())
        print(f"[resln] {name} | dx against aten fp32 | max abs err {e:.3e} | aten {ea:.3e} | ratio {e / ea:.3e}")
        assert e <= RC.ATEN_FACTOR * ea, (name, e, ea)


# ---- the row chains ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", RC.CHAIN_LIN_ROWS)
def test_row_chain_projection_residual_layernorm_against_fp64(rows):
    from mp_former_amd import _lib
    pb = RC.lin_problem(rows)
    a, w, b, x = _dev(pb.a_buf), _dev(RC.inbuf(pb.w)), _dev(RC.inbuf(pb.b)), _dev(pb.x_buf)
    gamma, beta = _params(pb)
    for want in (("s_out", "y32", "y16"), ("s_out", "y16"), ("s_out", "y32")):
        out = RC.fwd_buffers(pb, want)
        for k in ("s_out", "y32", "y16", "mean", "rstd"):
            setattr(out, k, _dev(getattr(out, k)))
        _lib.call("mpf_lin256_res_ln_forward", DEV, a.data_ptr(), w.data_ptr(), b.data_ptr(), x.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                  out.s_out.data_ptr(), _lib.ptr(out.y32), _lib.ptr(out.y16), out.mean.data_ptr(), out.rstd.data_ptr(), rows, pb.eps,
                  _lib.stream_ptr(DEV))
        assert _lib.last_kernel() == "lin256_res_ln_kernel"
        out = _cpu(out)
        frac = RC.check_lin(pb, out, route="+".join(want))
        assert "s_out" in frac and "mean" in frac and ("y32" in frac or "y16" in frac)
        if len(want) == 3:
            full = out
        else:
            _same(out, full, [k for k in want] + ["mean", "rstd"], f"lin r{rows}: {want} against all outputs")


@pytest.mark.parametrize("rows", RC.CHAIN_MLP_ROWS)
def test_row_chain_decoder_norm_mask_embed_bit_equal_and_inside_its_rows(rows):
    from mp_former_amd import _lib
    pb = RC.mlp_problem(rows)
    lib, st = _lib.lib(), _lib.stream_ptr(DEV)
    x = _dev(pb.x_buf)
    gamma, beta = _params(pb)
    ws, bs = [_dev(RC.inbuf(v)) for v in pb.ws], [_dev(RC.inbuf(v)) for v in pb.bs]
    out = _dev(RC.outbuf(rows * C, BF16))
    _lib.call("mpf_ln256_mlp3_forward", DEV, x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), ws[0].data_ptr(), bs[0].data_ptr(), ws[1].data_ptr(),
              bs[1].data_ptr(), ws[2].data_ptr(), bs[2].data_ptr(), out.data_ptr(), rows, pb.eps, st)
    assert _lib.last_kernel() == "ln_mlp3_kernel"
    got = RC.take(f"mlp r{rows}", "out", out.cpu(), rows * C)
    # the four launches it replaces: bit for bit
    d16, e1, e2 = (torch.empty(rows, C, device=DEV, dtype=BF16) for _ in range(3))
    m2, r2 = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    _lib.check(lib.mpf_res_ln256_forward(x.data_ptr(), None, 0, gamma.data_ptr(), beta.data_ptr(), None, None, d16.data_ptr(), m2.data_ptr(),
                                         r2.data_ptr(), rows, pb.eps, None, 0, None, st), "ln")
    for src, dst, k, relu in ((d16, e1, 0, 1), (e1, e2, 1, 1), (e2, d16, 2, 0)):
        _lib.check(lib.mpf_small_gemm_bf16(src.data_ptr(), C, 1, None, ws[k].data_ptr(), C, 1, bs[k].data_ptr(), None, 0, dst.data_ptr(), C,
                                           None, rows, C, C, relu, st), "gemm")
    assert RC.same_bits(got.view(rows, C), d16.cpu())
