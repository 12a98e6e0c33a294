"""CPU: tests/_resln_cases.py held to itself, to the built library and to aten, so that the GPU test (tests/test_resln_parity_gpu.py)
can rely on it: every backward row count has the block count it is listed for and reaches the loop tail it is there for, the grid
mirror equals the library's workspace queries over a sweep, aten's fp32 LayerNorm stays inside half of every bound, the exact
problem is exact in fp32 in two summation orders, and the emulation passes every check function the GPU test uses while each of its
15 single faults fails its named case.

aten fp32 (native_layer_norm and native_layer_norm_backward on the CPU), worst err / bound at K = 1 over all cases: mean 2.75,
rstd 2.01, ds32 2.64, dgamma 0.88 to 1.23 (its sum over the rows moves with the thread count), dbeta 1.90 (the last two without
the depth term), y32 16.5 against the form as stated and 3.02 against the form with the sigma term (tests/_resln_cases.py, Y FORM).  Twice 16.5 rounded up to a power of two is KY = 64, held on the
y32 form as stated; every other form is held at K = 8, twice 3.02 rounded up.  aten is asserted inside K / 2 = 4 and KY / 2 = 32 here
(test_zz_worst_figures_printed prints the figures of a run, relative to these).  The emulation, in torch's summation order, is at
3.7 (mean), 2.2 (rstd), 6.3 (y32 as stated), 3.4 (y32 with the sigma term) and 2.8 (ds32) of K = 1, and at 0.05 (dgamma) and 0.15
(dbeta) of K + D."""
import numpy as np
import pytest
import torch

import _resln_cases as RC

C = RC.C


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib.lib()


# ---- the grid rule and the row counts ------------------------------------------------------------------------------------------------------
def test_grid_mirror_equals_the_library(lib):
    for rows in list(range(1, 4200)) + [8191, 8192, 8193, 8195, 12288, 12289, 65536, 1 << 20, (1 << 20) + 1]:
        assert lib.mpf_res_ln256_backward_workspace_bytes(rows) == RC.workspace_bytes(rows), rows
        assert lib.mpf_res_ln256_backward_det_workspace_bytes(rows) == RC.det_workspace_bytes(rows) == 256 + RC.workspace_bytes(rows), rows
        rpb, blocks = RC.grid_rule(rows)
        assert rpb % 4 == 0 and blocks <= 1024 and (blocks - 1) * rpb < rows <= blocks * rpb
    for rows in (0, -1):
        assert lib.mpf_res_ln256_backward_workspace_bytes(rows) == 0 == RC.workspace_bytes(rows)
        assert lib.mpf_res_ln256_backward_det_workspace_bytes(rows) == 0 == RC.det_workspace_bytes(rows)


def _trips(nb, slices, first, step, stride):
    """per slice: how often the unrolled loop `for (b = slice; b + first < nb; b += step)` runs, and the tail walk's length"""
    out = []
    for sl in range(slices):
        b, n = sl, 0
        while b + first < nb:
            b, n = b + step, n + 1
        out.append((n, len(range(b, nb, stride))))
    return out


def test_every_row_count_reaches_what_it_is_listed_for():
    for rows, blocks in RC.BWD_ROWS.items():
        assert RC.grid_rule(rows)[1] == blocks, rows
    det = {r: _trips(b, 2, 30, 32, 2) for r, b in RC.BWD_ROWS.items() if r <= RC.DET_MAX_ROWS}      # PART == 2: 16 deep, 2 slices
    red = {r: _trips(b, 32, 224, 256, 32) for r, b in RC.BWD_ROWS.items()}                          # the reduce kernel: 8 deep, 32 slices
    assert det[124] == [(1, 0), (0, 15)] and det[128] == [(1, 0), (1, 0)] and det[132] == [(1, 1), (1, 0)]     # 31 / 32 / 33 blocks
    assert det[5] == [(0, 1), (0, 1)] and det[1] == det[4] == [(0, 1), (0, 0)]
    assert det[1024] == [(8, 0), (8, 0)] and det[1028] == [(8, 1), (8, 0)]
    assert [t[0] for t in red[900]] == [1] + [0] * 31 and red[900][0][1] == 0                        # 225 blocks: slice 0 only
    assert all(t == (1, 0) for t in red[1024]) and red[1028][0] == (1, 1) and red[1028][1] == (1, 0)
    assert all(t == (4, 0) for t in red[4096])
    assert RC.grid_rule(4097) == (8, 513) and 4097 - 512 * 8 == 1
    assert RC.grid_rule(8195) == (12, 683) and 8195 - 682 * 12 == 11                                # waves get 3, 3, 3, 2 rows
    assert [len(range(w, 11, 4)) for w in range(4)] == [3, 3, 3, 2]
    assert RC.grid_rule(RC.SUBSET_ROWS) == (4, 32)
    assert all(r <= RC.DET_MAX_ROWS or RC.grid_rule(r)[1] > 257 for r in RC.BWD_ROWS)
    assert max(RC.BWD_ROWS) * C * 4 <= 8 * 1024 * 1024 + 4096                                        # the largest tensor: 8 MB
    # forward: one wave per row, four rows per workgroup
    assert {r % 4 for r in RC.FWD_ROWS} == {0, 1, 3} and RC.FWD_ROWS == (1, 3, 4, 5, 17, 1027)
    assert {(c["rows"], c["padd_rows"]) for c in RC.FWD_CASES.values() if c["padd_rows"] and c["rows"] < 100} == {
        (r, p) for r in (5, 17) for p in (1, 3, 7)}
    assert {(c["ops"], c["ds"]) for c in RC.BWD_CASES.values() if c["rows"] == RC.SUBSET_ROWS and c["dist"] == "std"} >= {
        (o, d) for o in RC.OPERANDS for d in RC.OUTPUTS}


def test_problems_meet_their_input_conditions():
    for name in RC.FWD_CASES:
        pb = RC.fwd_problem(name)
        n = pb.rows * C
        assert torch.equal(pb.x_buf[:n].view(pb.rows, C), pb.x) and bool(torch.isnan(pb.x_buf[n:]).all()) and pb.x_buf.numel() == n + RC.PAD
        assert pb.t is None or bool(torch.isnan(pb.t_buf[n:].float()).all())
        if pb.padd_rows:
            assert pb.padd_buf.numel() == pb.padd_rows * C + RC.PAD and bool(torch.isnan(pb.padd_buf[pb.padd_rows * C:]).all())
        assert float(pb.gamma[7]) == 0.0 and float(pb.gamma[100]) < 0 and int((pb.gamma < 0).sum()) >= 1
        if pb.dist in ("const", "mix") and pb.rows > 1:
            const = (pb.x == pb.x[:, :1]).all(1)
            assert bool(const.any()) and bool((pb.x == 0).all(1).any())
            assert len({float(v) for v in pb.x[const, 0]}) == int(const.sum())                       # a different constant per row
        if pb.dist == "mix" and pb.rows >= 3:
            assert pb.large.tolist() == [i % 3 == 0 for i in range(pb.rows)] and abs(float(pb.x[0].mean()) - 300) < 0.05
    for name in ("m40 r125", "m300 r125", "tiny r125", "big r125"):
        pb, _ = RC.bwd_case(name)
        sd = float(pb.s.std())
        assert {"m40": abs(sd - 0.3) < 0.01, "m300": abs(sd - 0.05) < 0.002, "tiny": sd < 2e-20, "big": sd > 5e14}[pb.dist]
    b = RC.bwd_buffers(RC.bwd_case("std r125")[0], "ws", "ds32+ds16")
    sent = int(RC.bits(torch.full((1,), RC.SENT)))
    assert all(bool((RC.bits(v) == int(RC.bits(torch.full((1,), RC.SENT, dtype=v.dtype)))).all()) for v in (b.ds32, b.ds16, b.dgamma, b.dbeta))
    assert sent != 0
    b = RC.bwd_buffers(RC.bwd_case("std r125")[0], "atomic")
    assert bool((b.dgamma[:C] == 0).all()) and bool((RC.bits(b.dgamma[C:]) == sent).all())


# ---- aten inside half the bounds, the emulation inside them -----------------------------------------------------------------------------------
WORST = {}


def _note(tag, frac):
    for q, v in frac.items():
        WORST[(tag, q)] = max(WORST.get((tag, q), 0.0), v)


@pytest.mark.parametrize("name", list(RC.FWD_CASES))
def test_forward_aten_inside_half_the_bounds_and_the_emulation_inside_them(name):
    pb = RC.fwd_problem(name)
    _note("aten", RC.check_forward(pb, RC.aten_forward(pb), k=RC.K / 2, route="aten fp32 (cpu)"))
    frac = RC.check_forward(pb, RC.emulate_forward(pb), route="emulation")
    _note("emulation", frac)
    assert {"mean", "rstd", "y32", "y32_sigma"} <= set(frac)
    only16 = RC.emulate_forward(pb, want=("y16",))
    assert only16.s_out is None and only16.y32 is None
    assert "y16" in RC.check_forward(pb, only16, route="emulation, y16 only")
    assert RC.same_bits(only16.y16, RC.emulate_forward(pb).y16)


def _as_buffers(ds, dg, db):
    tail = lambda v: torch.cat([v.reshape(-1), RC.outbuf(0)])                             # noqa: E731
    return RC.SimpleNamespace(ds32=tail(ds), ds16=None, ds_amax=None, dgamma=tail(dg), dbeta=tail(db))


@pytest.mark.parametrize("name", list(RC.BWD_CASES))
def test_backward_aten_inside_half_the_bounds_and_the_emulation_inside_them(name):
    pb, ref = RC.bwd_case(name)
    ds_aten, dg, db = RC.aten_backward(pb)
    # aten's parameter sums get no depth term: "ws" is the smallest D of the forms, and K / 2 is asserted without it below
    frac = RC.check_backward(pb, ref, _as_buffers(ds_aten, dg, db), "ws", k=RC.K / 2, route="aten fp32 (cpu)")
    for q in ("dgamma", "dbeta"):
        at_half = frac[q] * (RC.K / 2 + RC.depth("ws", pb.rows)) / (RC.K / 2)
        assert at_half <= 1.0, (name, q, at_half)
        frac[q] = at_half
    _note("aten", frac)
    for form in RC.FORMS:
        if form == "det" and pb.rows > RC.DET_MAX_ROWS:
            continue
        out = RC.emulate_backward(pb, form, amax="ds32" in pb.ds)
        _note("emulation", RC.check_backward(pb, ref, out, form, route="emulation"))
        if out.ds32 is not None:
            RC.check_vs_aten(pb, ref, out.ds32[:pb.rows * C].view(pb.rows, C), ds_aten, route="emulation")


@pytest.mark.parametrize("rows", RC.CHAIN_LIN_ROWS)
def test_row_chain_emulation_inside_the_bounds(rows):
    pb = RC.lin_problem(rows)
    frac = RC.check_lin(pb, RC.emulate_lin(pb), route="emulation")
    assert {"s_out", "mean", "rstd", "y32", "y32_sigma"} <= set(frac)
    bad = RC.emulate_lin(pb)
    bad.s_out[:C] = pb.x[0]                                            # the projection left out of one row
    with pytest.raises(AssertionError):
        RC.check_lin(pb, bad, route="row 0 without its projection")


def test_zz_worst_figures_printed():
    """(runs last in this file) the worst err / bound per quantity of the parametrised tests above, at the K each was held to"""
    for (tag, q), v in sorted(WORST.items()):
        print(f"[resln] worst over the cases | {tag} | {q} | {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())


# ---- the exact problem ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [5, 132, 4097, 8195])
def test_exact_problem_is_exact_in_fp32_in_two_summation_orders(rows):
    pb, ref = RC.exact_case(rows)
    f = lambda t: t.float().numpy().astype(np.float32)                                   # noqa: E731
    s, mu, rs, gm = f(pb.s), f(pb.mean)[:, None], f(pb.rstd)[:, None], f(pb.gamma)
    assert set(np.unique(rs)) <= {np.float32(0.5), np.float32(1.0)} and set(np.unique(gm)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert np.all(s == np.round(s)) and np.abs(s).max() <= 4 and np.all(mu == np.round(mu))
    assert all(np.all(f(v) == np.round(f(v))) and np.abs(f(v)).max() <= 3 for v in (pb.gy32, pb.gy16, pb.gy_plus))
    g = (f(pb.gy32) + f(pb.gy16)) + f(pb.gy_plus)
    xh = (s - mu) * rs
    dg = g * gm

    def seq(v, axis, reverse):                  # one element after the other, from the front or from the back, all in fp32
        v = np.moveaxis(v, axis, 0)
        v = v[::-1] if reverse else v
        acc = np.zeros_like(v[0])
        for row in v:
            acc = (acc + row).astype(np.float32)
        return acc

    def tree(v, axis):                          # pairs of halves: the order of a butterfly
        v = np.moveaxis(v, axis, 0)
        while v.shape[0] > 1:
            if v.shape[0] % 2:
                v = np.concatenate([v, np.zeros_like(v[:1])])
            v = (v[: v.shape[0] // 2] + v[v.shape[0] // 2:]).astype(np.float32)
        return v[0]

    inv = np.float32(1.0 / 256.0)
    for order in ("front to back", "tree, then back to front"):
        if order == "front to back":
            s1, s2 = seq(dg, 1, False) * inv, seq(dg * xh, 1, False) * inv
            dgamma, dbeta = seq(g * xh, 0, False), seq(g, 0, False)
        else:
            s1, s2 = tree(dg, 1) * inv, tree(dg * xh, 1) * inv
            dgamma, dbeta = seq(g * xh, 0, True), tree(g, 0)
        ds = rs * (dg - s1[:, None] - xh * s2[:, None])
        assert ds.dtype == np.float32 and dgamma.dtype == np.float32
        for what, got, want in (("ds", ds, ref.ds), ("dgamma", dgamma, ref.dgamma), ("dbeta", dbeta, ref.dbeta)):
            assert np.array_equal(got.astype(np.float64), want.numpy()), (rows, order, what)
    assert float(ref.dgamma.abs().max()) < 2 ** 23 and float(ref.dbeta.abs().max()) > 0
    RC.check_exact(pb, ref, RC.emulate_backward(pb, "ws"), "ws", route="emulation")


@pytest.mark.parametrize("fault", sorted(RC.EXACT_FAULTS))
def test_faults_that_move_rows_fail_the_exact_problem(fault):
    pb, ref = RC.exact_case(RC.EXACT_FAULTS[fault])
    RC.check_exact(pb, ref, RC.emulate_backward(pb, "ws"), "ws", route="emulation")
    with pytest.raises(AssertionError):
        RC.check_exact(pb, ref, RC.emulate_backward(pb, "ws", fault), "ws", route=f"fault {fault}")


# ---- single faults ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault", RC.FAULTS)
def test_each_single_fault_fails_its_named_case(fault):
    assert set(RC.FAULT_CASE) == set(RC.FAULTS) and len(RC.FAULTS) == 15
    if fault in RC.FWD_FAULTS:
        pb = RC.fwd_problem(RC.FAULT_CASE[fault])
        RC.check_forward(pb, RC.emulate_forward(pb), route="emulation")
        with pytest.raises(AssertionError):
            RC.check_forward(pb, RC.emulate_forward(pb, fault), route=f"fault {fault}")
    else:
        name, form = RC.FAULT_CASE[fault]
        pb, ref = RC.bwd_case(name)
        RC.check_backward(pb, ref, RC.emulate_backward(pb, form, amax=True), form, route="emulation")
        with pytest.raises(AssertionError):
            RC.check_backward(pb, ref, RC.emulate_backward(pb, form, fault, amax=True), form, route=f"fault {fault}")


def test_a_written_tail_an_unwritten_element_and_a_read_nan_are_seen():
    pb = RC.fwd_problem("mix r5 t=bf16")
    for spoil in ("tail", "unwritten", "nan"):
        out = RC.emulate_forward(pb)
        if spoil == "tail":
            out.y32[pb.rows * C] = 0.0
        elif spoil == "unwritten":
            out.y16[3] = RC.SENT
        else:
            out.mean[pb.rows - 1] = RC.NAN
        with pytest.raises(AssertionError):
            RC.check_forward(pb, out, route=spoil)
