"""CPU: tests/_groupnorm_cases.py held to its own table, the built library and aten, so that the GPU test
(tests/test_groupnorm_routes_gpu.py) can rely on it: every row reaches the branch it is tagged with and every branch of the list
has a row, the geometry mirrors equal the library's queries over a sweep, the entry points refuse bad arguments before any launch,
aten's fp32 GroupNorm stays inside the bounds at K = 4 (the measurement behind K = 8), the ReLU kink cap holds, and the emulation
passes every check function the GPU test uses while each of its 14 single faults fails its named cases.

aten fp32 on the CPU, worst err / bound at K = 1 over all cases: y 3.96 (plain / relu), mean 2.41, rstd 1.13, dx 2.58, dgamma 2.74,
dbeta 1.57: inside K = 4.  The two quantities that pass through the bilinear taps are wider for aten: y of the ``top`` mode 4.66 (6 of
4.2 M elements of c256g32_82x100 above 4) and dtop 4.49 (aten's adjoint adds its up to 16 terms one by one); they are asserted
inside K = 8, the bound the kernels get, which is 1.7 x aten's worst instead of 2 x.  The emulation, whose taps and adjoint are the
kernels' expressions, is at 3.0 (dtop) of K = 1."""
import ctypes

import pytest
import torch

import _groupnorm_cases as GC

ATEN_K, ATEN_K_TAPS = 4.0, 8.0


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from mp_former_amd import _lib
    return _lib.lib()


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GC.CL_CASES))
def test_rows_reach_the_branches_they_are_tagged_with(name):
    row = GC.CL_CASES[name]
    H, W = row["hw"]
    P = GC.make_plane(H * W, row["C"], row["G"])
    t = row["tags"]
    assert P is not None
    assert (P.pr, P.cpg, P.chunks, P.tail) == (t["pr"], t["cpg"], t["chunks"], t["tail"])
    assert t.get("hw_lt_pr", False) == (H * W < P.pr)
    merge_trips, reduce_trips = -(-P.chunks // GC.MERGE_LANES), -(-P.chunks // GC.RED_SLICES)
    assert (merge_trips, reduce_trips) == {1: (1, 1), 2: (1, 1), 5: (1, 1), 33: (1, 2), 65: (2, 3), 130: (3, 5)}[P.chunks]
    # register blocks of the statistics kernel: a thread's pixels of the last chunk, in blocks of KSUB
    last = P.tail or GC.STAT_PIX
    per_thread = [len(range(r, last, P.pr)) for r in range(P.pr)]
    if P.pr <= 2:
        assert GC.STAT_PIX // (P.pr * GC.KSUB) >= 8 and any(n % GC.KSUB for n in per_thread), "pr 1 / 2: 8 or 16 blocks, one partial"
    if "top" in row["modes"]:
        assert H % 2 == 0 and W % 2 == 0
        kind = {(True, False): "wide", (False, True): "high", (True, True): "1x1"}.get((H == 2, W == 2), "rect")
        assert t.get("top", "rect") == kind
    if row["gaps"]:
        pb = GC.cl_problem(name, row["modes"][0])
        extra = [pb.bs[k] - (pb.tplane if k in ("top", "dtop") else pb.plane) for k in pb.bs]
        assert len(set(extra)) == len(extra) and all(e > 0 and e % 4 == 0 for e in extra)


def test_every_branch_of_the_list_has_a_row():
    tags = [r["tags"] for r in GC.CL_CASES.values()]
    assert {t["pr"] for t in tags} == {1, 2, 4, 8, 16, 32}
    assert {t["cpg"] for t in tags} == {4, 8, 16, 32}
    chunks = {t["chunks"] for t in tags}
    assert {1, 33, 65} <= chunks and max(chunks) > 128
    assert {0, 1, 4, 5, 8} <= {t["tail"] for t in tags}
    assert any(t.get("hw_lt_pr") for t in tags)
    assert {"wide", "high", "1x1", "rect"} <= {t.get("top") for t in tags}
    rows = GC.CL_CASES
    # H != W at small sizes, on both sides
    assert rows["c256g32_top_2x6"]["hw"] == (2, 6) and rows["c256g32_top_6x2"]["hw"] == (6, 2) and rows["c256g32_top_4x10"]["hw"] == (4, 10)
    # one row with gaps in every tensor per mode; both large-mean distributions at both shapes; an N = 1 row
    assert set(rows["c128g8_6x10_gaps"]["modes"]) == {"plain", "relu", "top"} and rows["c128g8_6x10_gaps"]["gaps"]
    assert {(r["C"], r["G"], r["hw"], r["dist"]) for r in rows.values() if r["dist"] != "std"} == {
        (32, 8, (90, 92), "m40"), (32, 8, (90, 92), "m300"), (256, 32, (34, 18), "m40"), (256, 32, (34, 18), "m300")}
    assert any(r["N"] == 1 for r in rows.values())
    prod = rows["c256g32_82x100"]
    assert prod["gaps"] and prod["N"] == 2 and prod["tags"]["chunks"] == 65
    # the NCHW rows: a row shorter than one sweep, rows ending 4 before, at and 4 behind a chunk, 12 into the fourth chunk
    lens = {v[1] for v in GC.NCHW_CASES.values()}
    assert lens == {4, 1020, 1024, 8188, 8192, 8196, 16388, 3 * 8192 + 12}
    assert [GC.group_stats_chunks(n) for n in (4, 8188, 8192, 8196, 16388, 3 * 8192 + 12)] == [1, 1, 1, 2, 3, 4]
    for (shape, G), key in zip(GC.NCHW_MODULE_CASES.values(), GC.NCHW_MODULE_CASES):
        N, C, H, W = shape
        assert (N * G, C // G * H * W) == GC.NCHW_CASES[key][:2]
    for shape, G, _ in GC.FALLBACK_CASES:
        assert GC.make_plane(shape[2] * shape[3], shape[1], G) is None


def test_problems_meet_their_input_conditions():
    for name, mode in GC.CL_RUNS:
        if GC.CL_CASES[name]["hw"][0] * GC.CL_CASES[name]["hw"][1] > 4000 and mode != "plain":
            continue
        pb = GC.cl_problem(name, mode)
        for key, vals in (("x", pb.x), ("gy", pb.gy), ("top", pb.top)):
            if vals is None:
                continue
            buf = getattr(pb, key + "_buf").view(pb.N, pb.bs[key])
            plane = vals[0].numel()
            assert torch.equal(buf[:, :plane].reshape(vals.shape), vals) and bool(torch.isfinite(vals).all())
            assert bool(torch.isnan(buf[:, plane:]).all()) and buf.shape[1] - plane == pb.gap[key] and pb.bs[key] % 4 == 0
        out = GC.new_buffers(pb)
        assert all(bool((GC._bits(b) == int(GC._bits(GC.sentinel(1)))).all()) for b in out.values())
        if pb.dist != "std":
            mu, sd = GC.LARGE_MEAN[pb.dist]
            assert abs(float(pb.x.mean()) - mu) < 0.01 * sd + 1e-3 * mu and abs(float(pb.x.std()) - sd) < 0.02 * sd


# ---- mirrors against the built library ---------------------------------------------------------------------------------------------------
def test_plane_and_workspace_mirrors_equal_the_library(lib):
    accepted = set()
    for C in range(4, 1101, 4):
        for G in (g for g in range(1, C + 1) if C % g == 0):
            for HW in (1, 127, 128, 129, 8193):
                P = GC.make_plane(HW, C, G)
                assert lib.mpf_gn_cl_supported(HW, C, G) == int(P is not None), (HW, C, G)
                for N in (1, 3):
                    assert lib.mpf_gn_cl_workspace_bytes(N, HW, C, G) == GC.cl_workspace_bytes(N, HW, C, G), (N, HW, C, G)
                if P is not None:
                    accepted.add((C, P.cpg))
                    assert (P.tpc, P.pr, P.chunks) == (C // 4, 1024 // C, (HW + 127) // 128)
    assert {c for c, _ in accepted} == {32, 64, 128, 256, 512, 1024} and {k for _, k in accepted} == {4, 8, 16, 32}
    for bad in [(0, 128, 256, 32), (-1, 128, 256, 32), (2, 0, 256, 32), (2, 128, 0, 32), (2, 128, 256, 0), (2, 128, 96, 32), (2, 128, 256, 4)]:
        assert lib.mpf_gn_cl_workspace_bytes(*bad) == 0 == GC.cl_workspace_bytes(*bad)
    # G <= C / 4, so the backward layout is the larger one for every accepted plane: the query returns bwd_ws
    for C, cpg in accepted:
        P = GC.make_plane(8193, C, C // cpg)
        assert GC.fwd_ws(2, P) < GC.bwd_ws(2, P) == lib.mpf_gn_cl_workspace_bytes(2, 8193, C, C // cpg)
    for name, row in GC.CL_CASES.items():
        HW = row["hw"][0] * row["hw"][1]
        assert lib.mpf_gn_cl_workspace_bytes(row["N"], HW, row["C"], row["G"]) == GC.cl_workspace_bytes(row["N"], HW, row["C"], row["G"]) > 0, name


def test_group_stats_chunk_mirror_equals_the_library(lib):
    for rows in (1, 5, 64):
        for n in (1, 4, 1020, 1024, 8188, 8192, 8193, 8196, 16384, 16388, 3 * 8192 + 12, 1 << 20, (1 << 31) + 8):
            assert lib.mpf_group_stats_workspace_bytes(rows, n) == GC.group_stats_workspace_bytes(rows, n) == rows * GC.group_stats_chunks(n) * 12
    for bad in [(0, 8), (-1, 8), (1, 0), (1, -4)]:
        assert lib.mpf_group_stats_workspace_bytes(*bad) == 0 == GC.group_stats_workspace_bytes(*bad)


# ---- argument checks: every call fails a check before any launch ---------------------------------------------------------------------------
SH, NUL = -2, -3                               # MPF_E_SHAPE, MPF_E_NULL


def _caller(fn, ok):
    return lambda **kw: fn(*{**ok, **kw}.values())


def test_forward_argument_errors(lib):
    one = ctypes.c_void_p(16)
    need = GC.fwd_ws(2, GC.make_plane(48, 256, 32))
    fw = _caller(lib.mpf_gn_cl_forward, dict(x=one, xbs=48 * 256, gamma=one, beta=one, N=2, HW=48, C=256, G=32, eps=1e-5, relu=0, top=None, tbs=0,
                                             W=8, y=one, ybs=48 * 256, mean=one, rstd=one, ws=one, wsb=need - 1, st=None))
    assert fw() == SH and b"workspace" in lib.mpf_last_error()                        # one byte short, everything else valid
    for k in ("x", "gamma", "beta", "y", "mean", "rstd", "ws"):
        assert fw(**{k: None}) == NUL and b"NULL" in lib.mpf_last_error(), k
    for C, G in ((96, 32), (256, 4), (64, 32), (256, 3), (2048, 64), (48, 4)):       # C/G = 3, 64, 2; G does not divide; C > 1024; C % 32
        assert fw(C=C, G=G, wsb=1 << 30) == SH and b"power of two" in lib.mpf_last_error(), (C, G)
    assert fw(N=0) == SH and fw(HW=0) == SH
    for k in ("xbs", "ybs", "tbs"):
        assert fw(**{k: 48 * 256 + 2}, wsb=need) == SH and b"multiples of 4" in lib.mpf_last_error(), k
    top = dict(top=one, tbs=12 * 256, wsb=need)
    assert fw(**top, W=7) == SH and b"even" in lib.mpf_last_error()                   # HW % W != 0
    assert fw(**top, HW=40, W=5, xbs=40 * 256, ybs=40 * 256) == SH and b"even" in lib.mpf_last_error()       # odd W
    assert fw(**top, HW=40, W=8, xbs=40 * 256, ybs=40 * 256) == SH and b"even" in lib.mpf_last_error()       # odd H = 5
    assert fw(**top, W=0) == SH
    assert fw(**top, relu=1) == SH and b"exclusive" in lib.mpf_last_error()


def test_backward_argument_errors(lib):
    one = ctypes.c_void_p(16)
    need = GC.bwd_ws(2, GC.make_plane(48, 256, 32))
    assert need > GC.fwd_ws(2, GC.make_plane(48, 256, 32))
    bw = _caller(lib.mpf_gn_cl_backward, dict(gy=one, gbs=48 * 256, x=one, xbs=48 * 256, gamma=one, beta=one, mean=one, rstd=one, N=2, HW=48, C=256,
                                              G=32, relu=0, dx=one, dbs=48 * 256, dg=one, db=one, ws=one, wsb=need - 1, st=None))
    assert bw() == SH and b"workspace" in lib.mpf_last_error()
    for k in ("gy", "x", "gamma", "beta", "mean", "rstd", "dx", "ws"):
        assert bw(**{k: None}) == NUL and b"NULL" in lib.mpf_last_error(), k
    for C, G in ((96, 32), (256, 4), (64, 32)):
        assert bw(C=C, G=G, wsb=1 << 30) == SH and b"power of two" in lib.mpf_last_error(), (C, G)
    for k in ("gbs", "xbs", "dbs"):
        assert bw(**{k: 48 * 256 + 1}, wsb=need) == SH and b"multiples of 4" in lib.mpf_last_error(), k
    assert bw(N=0) == SH and bw(HW=-1) == SH


def test_upsample_backward_argument_errors(lib):
    one = ctypes.c_void_p(16)
    up = _caller(lib.mpf_upsample2x_cl_backward, dict(gy=one, gbs=48 * 256, N=2, Ht=3, Wt=4, C=256, dtop=one, tbs=12 * 256, st=None))
    assert up(gy=None) == NUL and up(dtop=None) == NUL
    for kw in (dict(N=0), dict(Ht=0), dict(Wt=0), dict(C=0), dict(C=254), dict(C=2048), dict(C=96), dict(gbs=48 * 256 + 2), dict(tbs=12 * 256 + 2)):
        assert up(**kw) == SH and b"upsample2x_cl_backward" in lib.mpf_last_error(), kw


def test_group_stats_argument_errors(lib):
    one = ctypes.c_void_p(16)
    need = lib.mpf_group_stats_workspace_bytes(5, 8196)
    gs = _caller(lib.mpf_group_stats, dict(x=one, rows=5, n=8196, eps=1e-5, mean=one, rstd=one, ws=one, wsb=need - 1, st=None))
    assert gs() == SH and b"workspace" in lib.mpf_last_error()
    for k in ("x", "mean", "rstd", "ws"):
        assert gs(**{k: None}) == NUL, k
    for n in (8194, 8195, 18, 0, -4):
        assert gs(n=n, wsb=1 << 30) == SH and b"multiple of 4" in lib.mpf_last_error(), n
    assert gs(rows=0) == SH


# ---- the measurement behind K, the kink cap, the emulation -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GC.CL_CASES))
def test_aten_fp32_is_inside_half_the_bounds_and_the_emulation_inside_them(name):
    for mode in GC.CL_CASES[name]["modes"]:
        pb, ref = GC.cl_case(name, mode)
        assert pb.kink_share <= GC.KINK_CAP and (pb.relu or pb.kink_share == 0.0), (name, mode, pb.kink_share)
        aten = GC.aten_results(pb)
        taps = ("y", "dtop") if pb.has_top else ()
        GC.check_all(pb, ref, aten, k=ATEN_K, route="aten fp32 (cpu)", only=[q for q in GC.QUANTITIES if q not in taps])
        GC.check_all(pb, ref, aten, k=ATEN_K_TAPS, route="aten fp32 (cpu)", only=taps)
        res = GC.take_all(pb, GC.emulate(pb))
        frac = GC.check_all(pb, ref, res, route="emulation")
        assert set(frac) == set(GC.QUANTITIES) - (set() if pb.has_top else {"dtop"})
        if pb.dist != "std":
            GC.check_vs_aten(pb, ref, res.dx, aten.dx, route="emulation")


def test_the_squared_rstd_form_would_not_see_a_one_pass_variance():
    """why the rstd form kept is the first-order one: fault 4 is 40 and 5000 first-order bounds off at the two large-mean
    distributions, but 0.3 of the issue's squared form at 40 + 0.3 randn (0.9 at 300 + 0.05 randn: not asserted)"""
    for name, inside_squared in (("c32g8_90x92_m40", True), ("c256g32_34x18_m300", None)):
        pb, ref = GC.cl_case(name, "plain")
        res = GC.take_all(pb, GC.emulate(pb, "naive_var"))
        err = (res.rstd.to(GC.F64) - ref.rstd).abs()
        assert float((err / (GC.K * ref.b_rstd)).max()) > 10.0
        assert float((ref.b_rstd_squared / ref.b_rstd).min()) > 100.0
        if inside_squared:
            assert float((err / (GC.K * ref.b_rstd_squared)).max()) < 0.5


@pytest.mark.parametrize("name", list(GC.NCHW_CASES))
def test_nchw_rows_aten_moments_inside_half_the_bounds(name):
    np_ = GC.nchw_problem(name)
    assert bool(torch.isnan(np_.buf[:GC.NCHW_PAD]).all()) and bool(torch.isnan(np_.buf[-GC.NCHW_PAD:]).all())
    assert torch.equal(np_.buf[GC.NCHW_PAD:-GC.NCHW_PAD].view(np_.rows, np_.row_len), np_.x)
    _, mean, rstd = torch.native_group_norm(np_.x.view(1, np_.rows, np_.row_len), None, None, 1, np_.rows, np_.row_len, np_.rows, np_.eps)
    pad = lambda t: torch.cat([t.reshape(-1), GC.sentinel(GC.GUARD)])                 # noqa: E731
    GC.check_stats(np_, pad(mean), pad(rstd), k=ATEN_K, route="aten fp32 (cpu)")
    with pytest.raises(AssertionError):
        GC.check_stats(np_, pad(mean), torch.cat([rstd.reshape(-1), GC.sentinel(GC.GUARD - 1), torch.zeros(1)]))      # a guard element written


@pytest.mark.parametrize("fault", GC.FAULTS)
def test_each_single_fault_fails_its_named_cases(fault):
    assert set(GC.FAULT_CASE) == set(GC.FAULTS) and len(GC.FAULTS) == 14
    for name, mode in GC.FAULT_CASE[fault]:
        assert (name, mode) in GC.CL_RUNS
        pb, ref = GC.cl_case(name, mode)
        with pytest.raises(AssertionError):
            GC.check_all(pb, ref, GC.take_all(pb, GC.emulate(pb, fault)), route=f"fault {fault}")
