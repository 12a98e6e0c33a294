"""The small-row GEMM family of csrc/small_gemm.hip through its C ABI, one output element at a time against fp64: every operand
form, tile width, contraction tail and epilogue of ``mpf_small_gemm_bf16``, the blocked forms of ``mpf_small_gemm_bf16_blocked``,
``mpf_transpose_group_bf16`` (exact), both operand forms of ``mpf_small_gemm_bf16_group`` and the ``decoder_dw_group`` switch.

The reference and the bound (derived, not measured; the same everywhere in this file).  Operands are random bf16 numbers from a
seeded generator; the reference is the same expression in fp64:

    ref[i, j] = sum_k A(i, k) [gate(i, k) > 0] B(j, k) + bias[j] + c_in[i, j]            (ReLU on top where asked)
    S[i, j]   = sum_k |A(i, k)| [gate(i, k) > 0] |B(j, k)| + |bias[j]| + |c_in[i, j]|

and EVERY output element must satisfy

    |got - ref| <= 2^-8 |ref| + (Kc + 8) 2^-22 S + 1e-30.

- 2^-8 |ref|: the one round-to-nearest of the fp32 result to bf16.  bf16 has 8 significant bits, half an ulp is at most 2^-8
  relative.
- (Kc + 8) 2^-22 S: fp32 accumulation of Kc exact bf16 x bf16 products (a product of two 8-bit significands is exact in fp32) plus
  the epilogue adds.  Each operation costs at most 2^-23 of the running magnitude (<= S) if the matrix core truncates instead of
  rounding; the bound doubles that once more as margin, because the sum over the four waves through LDS reassociates.  (That
  margin also covers the second-order term: the value that is rounded to bf16 is the fp32 result, not ref.)
- ReLU is 1-Lipschitz: the same bound holds against relu(ref) with the pre-activation S.
- rowsum_a: the same bound with ref = sum_k A [gate > 0], S = sum_k |A| [gate > 0].

No element is excluded, no percentile is taken.  A dropped 8-element fragment leaves an error of order sqrt(8) sigma_a sigma_b,
hundreds of times this bound for the unit-scale operands used here.  Each case prints its largest err / bound; nothing is
asserted about that figure except that it is at most 1.

Poison and canaries, in every case: operand buffers are larger than the addressed region and NaN wherever the problem does not
address them (between rows where the stride exceeds the width, between blocks, behind the last row), so an out-of-range read that
is used shows as NaN; result buffers start as the bf16 sentinel 3.0 and every element outside the addressed I x J region
(columns J .. ldc - 1, the gaps between column blocks, the rows behind I, rowsum_a behind I) must still hold it afterwards.

NaN gates are out of scope: the kernel tests the sign and zero-ness of the gate's bit pattern as an integer (a positive NaN
passes), IEEE ``>`` is false for every NaN.  The planted gate values (+0, -0, the smallest positive normal, -1, +inf) pin the
rule for everything else bit for bit.
"""
import itertools

import pytest
import torch

from test_decoder_layer_direct_gpu import ACTS, CASES, NAMES, _problem, _run_native

pytestmark = pytest.mark.gpu

SENT = 3.0                      # what result buffers hold before a call
E_SHAPE = -2                    # MPF_E_SHAPE
BF16 = torch.bfloat16


def _dev():
    return torch.device("cuda:0")


def _lib():
    from mp_former_amd import _lib as L
    return L


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
def _addr(n, Kc, contig, blk=0):
    """Element offsets of an operand (n rows, contraction Kc) in its buffer -> (offsets [n, Kc], row stride, contraction stride,
    block stride, buffer elements).  Strides exceed the widths, block strides exceed the blocks: the addressed elements have gaps
    between them.  contig: contraction-contiguous (rows 16-byte aligned); blk: blocked contraction (contig) / blocked rows."""
    i = torch.arange(n).view(-1, 1)
    k = torch.arange(Kc).view(1, -1)
    if contig and blk:
        rs, ks = blk + 8, 1
        bs = n * rs + 16
        off = i * rs + (k // blk) * bs + k % blk
    elif contig:
        rs, ks, bs = Kc + 8, 1, 0
        off = i * rs + k
    elif blk:
        rs, ks = 1, blk + 5
        bs = Kc * ks + 7
        off = (i // blk) * bs + i % blk + k * ks
    else:
        rs, ks, bs = 1, n + 3, 0
        off = k * ks + i
    return off, rs, ks, bs, int(off.max()) + 1 + 64


def _filled(size, off, vals, fill):
    buf = torch.full((size,), fill, dtype=BF16, device=_dev())
    if off is not None:
        buf[off.reshape(-1).to(_dev())] = vals.reshape(-1).to(_dev())
    return buf


def _plant_gate(g):
    """the values that pin `gate > 0` bit for bit, spread over a random gate (NaN gates: see the module docstring)"""
    flat = g.view(-1)
    n = flat.numel()
    assert n >= 8
    special = torch.tensor([0.0, -0.0, 2.0 ** -126, -1.0, float("inf")]).bfloat16()
    assert special.view(torch.int16).tolist() == [0, -32768, 0x0080, -16512, 0x7f80]
    flat[torch.tensor([0, n // 5, 2 * n // 5, 3 * n // 5, n - 1])] = special
    return g


def _untouched(buf, off):
    """every element of a result buffer that the problem does not address still holds the sentinel"""
    free = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    if off is not None:
        free[off.reshape(-1).to(buf.device)] = False
    return bool((buf[free] == SENT).all())


def _within(got, ref, S, Kc, what):
    """the per-element bound of the module docstring -> largest err / bound"""
    assert bool(torch.isfinite(got.float()).all()), f"{what}: not finite"
    err = (got.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + (Kc + 8) * 2.0 ** -22 * S + 1e-30
    ratio = err / bound
    worst = int(ratio.argmax())
    assert bool((err <= bound).all()), (f"{what}: {int((err > bound).sum())} of {err.numel()} elements outside the bound, worst at flat "
                                        f"index {worst}: got {float(got.reshape(-1)[worst])} ref {float(ref.reshape(-1)[worst])} "
                                        f"err / bound {float(ratio.reshape(-1)[worst]):.1f}")
    return float(ratio.max())


def _nj(I, J):
    """the tile width sg_fill (csrc/small_gemm.hip) picks: the widest of 4, 2, 1 that still gives >= 256 blocks"""
    nj = 4
    while nj > 1 and -(-I // 16) * -(-J // (16 * nj)) < 256:
        nj //= 2
    return nj


# ---- one GEMM --------------------------------------------------------------------------------------------------------------------
def _gemm(seed, I, J, Kc, ac, bc, gate=False, bias=False, relu=False, cin=None, ldc_pad=0, rowsum=False, a_blk=0, c_blk=0,
          blocked=False, tag=""):
    """One launch of mpf_small_gemm_bf16 (or _blocked) with poisoned operands and sentinel-filled results, checked per element.
    cin: None | "sep" (its own buffer, ldcin != ldc) | "alias" (c itself, pre-filled with the addend)."""
    L = _lib()
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(I, Kc, generator=g).bfloat16()
    B = torch.randn(J, Kc, generator=g).bfloat16()
    G = _plant_gate(torch.randn(I, Kc, generator=g).bfloat16()) if gate else None
    bias_v = torch.randn(J, generator=g).bfloat16() if bias else None
    cin_v = torch.randn(I, J, generator=g).bfloat16() if cin else None

    a_off, a_rs, a_ks, a_bs, a_size = _addr(I, Kc, ac, a_blk)
    b_off, b_rs, b_ks, _, b_size = _addr(J, Kc, bc)
    a_buf = _filled(a_size, a_off, A, float("nan"))
    b_buf = _filled(b_size, b_off, B, float("nan"))
    g_buf = _filled(a_size, a_off, G, float("nan")) if gate else None
    bias_buf = _filled(J + 8, torch.arange(J), bias_v, float("nan")) if bias else None

    ldc = (c_blk or J) + ldc_pad
    c_bs = I * ldc + 24 if c_blk else 0
    ii, jj = torch.arange(I).view(-1, 1), torch.arange(J).view(1, -1)
    c_off = ii * ldc + ((jj // c_blk) * c_bs + jj % c_blk if c_blk else jj)
    c_buf = _filled(int(c_off.max()) + 1 + 64, None, None, SENT)
    cin_buf, ldcin = None, 0
    if cin == "sep":
        ldcin = J + 4
        assert ldcin != ldc
        cin_buf = _filled(I * ldcin + 64, ii * ldcin + jj, cin_v, float("nan"))
    elif cin == "alias":
        c_buf[c_off.reshape(-1).to(dev)] = cin_v.reshape(-1).to(dev)
        cin_buf, ldcin = c_buf, ldc
    rs_buf = _filled(I + 16, None, None, SENT) if rowsum else None

    ptr = L.ptr
    st = L.stream_ptr(dev)
    if blocked or a_blk or c_blk:
        code = L.lib().mpf_small_gemm_bf16_blocked(a_buf.data_ptr(), a_rs, a_ks, a_blk, a_bs, ptr(g_buf), b_buf.data_ptr(), b_rs, b_ks,
                                                   ptr(bias_buf), ptr(cin_buf), ldcin, c_buf.data_ptr(), ldc, c_blk, c_bs, ptr(rs_buf),
                                                   I, J, Kc, int(relu), st)
    else:
        code = L.lib().mpf_small_gemm_bf16(a_buf.data_ptr(), a_rs, a_ks, ptr(g_buf), b_buf.data_ptr(), b_rs, b_ks, ptr(bias_buf),
                                           ptr(cin_buf), ldcin, c_buf.data_ptr(), ldc, ptr(rs_buf), I, J, Kc, int(relu), st)
    assert code == 0, L.lib().mpf_last_error().decode()
    torch.cuda.synchronize()

    Ad, Bd = A.to(dev).double(), B.to(dev).double()
    if gate:
        Ad = Ad * (G.to(dev).double() > 0)
    ref, S = Ad @ Bd.T, Ad.abs() @ Bd.abs().T
    if bias:
        ref, S = ref + bias_v.to(dev).double(), S + bias_v.to(dev).double().abs()
    if cin:
        ref, S = ref + cin_v.to(dev).double(), S + cin_v.to(dev).double().abs()
    if relu:
        ref = ref.relu()
    got = c_buf[c_off.to(dev)]
    worst = _within(got, ref, S, Kc, f"{tag} c")
    assert _untouched(c_buf, c_off), f"{tag}: result buffer written outside the I x J region"
    worst_rs = 0.0
    if rowsum:
        worst_rs = _within(rs_buf[:I], Ad.sum(1), Ad.abs().sum(1), Kc, f"{tag} rowsum_a")
        assert bool((rs_buf[I:] == SENT).all()), f"{tag}: rowsum_a written behind row I"
    print(f"[small_gemm] {tag}: max err / bound {worst:.3f}" + (f", rowsum_a {worst_rs:.3f}" if rowsum else ""))
    return got, (rs_buf[:I].clone() if rowsum else None)


# ---- 1: the plain entry point, every branch of small_gemm_kernel -------------------------------------------------------------------
FORMS = ((True, True), (True, False), (False, False), (False, True))       # (A, B contraction-contiguous): forward, dX, dW, unused
KCS = (8, 40, 96, 288, 544, 552)        # one step | MASK, two | three | nine | seventeen (second trip of the loop) | the same, MASK
SMALL = ((1, 4), (15, 20), (17, 40))    # nj = 1: the smallest and ragged tiles
LARGE = ((250, 520, 2), (250, 1028, 4))  # nj = 2: 17 * 16 blocks, last tile 8 columns wide; nj = 4: 17 * 16 blocks, last tile 4 wide
# (bias, relu, c_in, ldc - J, rowsum_a): taken in turn along the case list (7 is coprime to every loop length below)
EPILOGUES = ((False, False, None, 0, False), (True, False, None, 12, True), (True, True, "sep", 0, False), (False, False, "alias", 12, True),
             (False, True, None, 12, False), (True, False, "alias", 0, True), (True, True, "sep", 12, True))


def _plain_cases():
    out = []
    for (I, J), form, Kc, gate in itertools.product(SMALL, FORMS, KCS, (False, True)):
        out.append((I, J, 1, form, Kc, gate) + EPILOGUES[len(out) % 7])
    for (I, J, nj), form, Kc, gate in itertools.product(LARGE, FORMS, (40, 288), (False, True)):
        out.append((I, J, nj, form, Kc, gate) + EPILOGUES[len(out) % 7])
    return out


PLAIN = _plain_cases()


def _plain_id(c):
    I, J, nj, (ac, bc), Kc, gate, bias, relu, cin, pad, rowsum = c
    return (f"{I}x{J}x{Kc}-nj{nj}-a{'c' if ac else 'r'}b{'c' if bc else 'r'}" + ("-gate" if gate else "") + ("-bias" if bias else "")
            + ("-relu" if relu else "") + (f"-cin_{cin}" if cin else "") + (f"-ldc+{pad}" if pad else "") + ("-rowsum" if rowsum else ""))


def test_plain_case_list_reaches_every_instantiation():
    """every small_gemm_kernel<NJ, AC, BC, GATE, MASK> once, every epilogue option with at least two operand forms, rowsum_a with
    and without gate and over several column tiles"""
    inst = {(nj, form, gate, Kc % 32 != 0) for _, _, nj, form, Kc, gate, *_ in PLAIN}
    assert inst == set(itertools.product((1, 2, 4), FORMS, (False, True), (False, True)))
    forms_of = {}
    for I, J, nj, form, Kc, gate, bias, relu, cin, pad, rowsum in PLAIN:
        for opt in (("bias", bias), ("relu", relu), ("cin", cin), ("pad", pad), ("rowsum", rowsum, gate), ("rowsum tiles", rowsum and J > 16 * nj)):
            forms_of.setdefault(opt, set()).add(form)
    for opt in [("bias", True), ("bias", False), ("relu", True), ("relu", False), ("cin", None), ("cin", "sep"), ("cin", "alias"),
                ("pad", 0), ("pad", 12), ("rowsum", True, True), ("rowsum", True, False), ("rowsum tiles", True)]:
        assert len(forms_of.get(opt, ())) >= 2, opt


@pytest.mark.parametrize("case", PLAIN, ids=_plain_id)
def test_plain_entry_point_per_element(case):
    I, J, nj, (ac, bc), Kc, gate, bias, relu, cin, pad, rowsum = case
    assert _nj(I, J) == nj, "the tile-width rule no longer sends this case to the branch it was written for"
    _gemm(PLAIN.index(case), I, J, Kc, ac, bc, gate=gate, bias=bias, relu=relu, cin=cin, ldc_pad=pad, rowsum=rowsum, tag=_plain_id(case))


# ---- 2: the blocked forms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate", [False, True], ids=["", "gate"])
@pytest.mark.parametrize("a_blk,Kc,I,J,bc", [(32, 96, 17, 40, False), (32, 96, 17, 40, True), (64, 96, 17, 40, False), (64, 96, 15, 20, True),
                                             (256, 768, 33, 256, False)])
def test_blocked_contraction(a_blk, Kc, I, J, bc, gate):
    """a_ks == 1, a_blk > 0: the contraction index runs over blocks of a_blk, a_bs apart ([dq | dk | dv] . W_in of the decoder
    layer's backward: a_blk = 256, Kc = 768); a_bs > I * a_blk, so there is NaN between the blocks; with a_blk = 64, Kc = 96 the
    contraction ends inside the second block.  The gate is addressed like a."""
    _gemm(1000 + a_blk + I, I, J, Kc, True, bc, gate=gate, a_blk=a_blk, ldc_pad=12 if gate else 0,
          tag=f"blocked contraction a_blk {a_blk} Kc {Kc} I {I} J {J} b{'c' if bc else 'r'}{' gate' if gate else ''}")


@pytest.mark.parametrize("I", [96, 80])
@pytest.mark.parametrize("Kc", [33, 230])
def test_row_blocked_a(I, Kc):
    """a_rs == 1, a_blk > 0: row i of A lives in block i / a_blk (the packed in-projection weight gradient: dw_item(..., kE, R * kE)),
    with gate and rowsum_a; I = 80: a partial last block"""
    for gate in (True, False):
        _gemm(2000 + I + Kc, I, 40, Kc, False, False, gate=gate, rowsum=True, a_blk=32, tag=f"row-blocked A I {I} Kc {Kc}{' gate' if gate else ''}")


@pytest.mark.parametrize("c_blk,J,I,Kc,bias", [(64, 192, 17, 96, False), (256, 768, 33, 256, True)])
def test_column_blocked_output(c_blk, J, I, Kc, bias):
    """c_blk > 0: column j of the result lands in block j / c_blk, c_bs apart (the packed q | k | v projection: c_blk = 256,
    J = 768, with bias); ldc = c_blk, c_bs > I * ldc: the gaps between the blocks keep the sentinel"""
    _gemm(3000 + c_blk, I, J, Kc, True, True, bias=bias, c_blk=c_blk, tag=f"column-blocked c_blk {c_blk} J {J} I {I}")


# ---- 3: mpf_transpose_group_bf16, exact ------------------------------------------------------------------------------------------------
TR_SHAPES = ((1, 8, 8), (33, 40, 64), (64, 64, 64), (230, 256, 256), (70, 2048, 72))     # (R, C, Rp)


def _transpose_launch(Rp, shapes, seed):
    """[(R, C, ld, gated)] in one launch -> bit-exact checks of every destination"""
    from mp_former_amd.small_linear import MpfTransposeItem
    L = _lib()
    dev = _dev()
    g = torch.Generator().manual_seed(seed)
    items = (MpfTransposeItem * len(shapes))()
    keep = []
    for it, (R, C, ld, gated) in zip(items, shapes):
        off = torch.arange(R).view(-1, 1) * ld + torch.arange(C).view(1, -1)
        src_v = torch.randn(R, C, generator=g).bfloat16()
        src = _filled(R * ld + 64, off, src_v, float("nan"))
        gate_v = _plant_gate(torch.randn(R, C, generator=g).bfloat16()) if gated else None
        gate = _filled(R * ld + 64, off, gate_v, float("nan")) if gated else None
        dst = _filled(C * Rp + 64, None, None, SENT)
        it.src, it.gate, it.dst, it.ld, it.R, it.C = src.data_ptr(), L.ptr(gate), dst.data_ptr(), ld, R, C
        keep.append((src, gate, dst, src_v, gate_v))
    code = L.lib().mpf_transpose_group_bf16(items, len(shapes), Rp, L.stream_ptr(dev))
    assert code == 0, L.lib().mpf_last_error().decode()
    torch.cuda.synchronize()
    for (R, C, ld, gated), (src, gate, dst, src_v, gate_v) in zip(shapes, keep):
        want = src_v.to(dev)
        if gated:
            want = torch.where(gate_v.to(dev) > 0, want, torch.zeros((), dtype=BF16, device=dev))
        out = dst[:C * Rp].view(C, Rp)
        what = (R, C, Rp, ld, gated)
        assert torch.equal(out[:, :R].contiguous().view(torch.int16), want.T.contiguous().view(torch.int16)), what
        assert bool((out[:, R:].view(torch.int16) == 0).all()), what         # the padding is +0
        assert bool((dst[C * Rp:] == SENT).all()), what


@pytest.mark.parametrize("Rp", sorted({s[2] for s in TR_SHAPES}))
def test_transpose_group_sixteen_items(Rp):
    """Sixteen matrices (the most a launch takes) of mixed shapes, ld == C and ld > C, gated and ungated.  Rp is one argument of
    the launch, so one launch per Rp of the shape list, over every (R, C) of the list that fits it (R <= Rp), the list's own
    (R, C) of that Rp among them: Rp not a multiple of 64, C not a multiple of 64 and C of more than one tile."""
    fit = [(R, C) for R, C, _ in TR_SHAPES if R <= Rp]
    assert any((R, C, Rp) in TR_SHAPES for R, C in fit)
    shapes = [fit[t % len(fit)] + (fit[t % len(fit)][1] + (8 if (t // len(fit)) % 2 == 0 else 0), t % 3 != 1) for t in range(16)]
    assert {s[3] for s in shapes} == {True, False} and any(s[2] > s[1] for s in shapes)
    _transpose_launch(Rp, shapes, 4000 + Rp)


@pytest.mark.parametrize("R,C,Rp", TR_SHAPES)
def test_transpose_group_one_item(R, C, Rp):
    _transpose_launch(Rp, [(R, C, C + 8, True)], 4100 + R)
    _transpose_launch(Rp, [(R, C, C, False)], 4200 + R)


# ---- 4: the grouped launch, both operand forms -----------------------------------------------------------------------------------------
# (I, J, gated) of dW [I, J] = (dy [R, I] gated)^T . x [R, J]; I and J are multiples of 8 so that the transposed copies exist.
GROUP = ((256, 1032, False), (248, 1024, True), (248, 520, True), (768, 256, False), (40, 64, True), (16, 40, False), (24, 8, True), (8, 24, False))
GROUP_NJ = (4, 4, 2, 2, 1, 1, 1, 1)


class _GroupProblem:
    """the eight weight-gradient problems over R rows: operands (rows ld > width apart, NaN in between and behind), fp64 references"""

    def __init__(self, R, seed):
        dev = _dev()
        g = torch.Generator().manual_seed(seed)
        self.R, self.ops, self.refs = R, [], []
        for I, J, gated in GROUP:
            vals = [torch.randn(R, I, generator=g).bfloat16(), torch.randn(R, J, generator=g).bfloat16(),
                    _plant_gate(torch.randn(R, I, generator=g).bfloat16()) if gated else None]
            bufs = []
            for v in vals:
                if v is None:
                    bufs.append(None)
                    continue
                ld = v.shape[1] + 8
                bufs.append((_filled(R * ld + 64, torch.arange(R).view(-1, 1) * ld + torch.arange(v.shape[1]).view(1, -1), v, float("nan")), ld))
            self.ops.append(bufs)
            Ad = vals[0].to(dev).double().T
            if gated:
                Ad = Ad * (vals[2].to(dev).double().T > 0)
            xd = vals[1].to(dev).double().T
            self.refs.append((Ad @ xd.T, Ad.abs() @ xd.abs().T, Ad.sum(1), Ad.abs().sum(1)))

    @staticmethod
    def outputs(which=range(len(GROUP))):
        """fresh sentinel-filled (dW buffer with ldc = J + 12 and a row behind I, db buffer with 16 elements behind I) per problem"""
        return {t: (torch.full((GROUP[t][0] + 1, GROUP[t][1] + 12), SENT, dtype=BF16, device=_dev()),
                    torch.full((GROUP[t][0] + 16,), SENT, dtype=BF16, device=_dev())) for t in which}

    def item(self, it, t, out):
        """problem t in the row-contiguous form: A(i, k) = dy[k, i], B(j, k) = x[k, j]"""
        I, J, _ = GROUP[t]
        (dy, ld_a), (x, ld_b), gate = self.ops[t]
        it.a, it.gate, it.b, it.c, it.rowsum_a = dy.data_ptr(), (gate[0].data_ptr() if gate else None), x.data_ptr(), out[0].data_ptr(), out[1].data_ptr()
        it.a_rs, it.a_ks, it.a_bs, it.b_rs, it.b_ks, it.ldc = 1, ld_a, 0, 1, ld_b, J + 12
        it.a_blk, it.I, it.J, it.Kc = 0, I, J, self.R

    def check(self, outs, what):
        worst = worst_rs = 0.0
        for t, (dw, db) in outs.items():
            I, J, _ = GROUP[t]
            ref, S, rs, Srs = self.refs[t]
            worst = max(worst, _within(dw[:I, :J], ref, S, self.R, f"{what} problem {t} dW"))
            worst_rs = max(worst_rs, _within(db[:I], rs, Srs, self.R, f"{what} problem {t} db"))
            assert bool((dw[:I, J:] == SENT).all()) and bool((dw[I:] == SENT).all()) and bool((db[I:] == SENT).all()), (what, t)
        print(f"[small_gemm] {what} R {self.R}: max err / bound {worst:.3f}, rowsum_a {worst_rs:.3f}")


def _group_launch(items, n):
    L = _lib()
    code = L.lib().mpf_small_gemm_bf16_group(items, n, L.stream_ptr(_dev()))
    assert code == 0, L.lib().mpf_last_error().decode()
    torch.cuda.synchronize()


def _same(a, b):
    """two sets of result buffers bit for bit, sentinels included"""
    return all(torch.equal(a[t][0].view(torch.int16), b[t][0].view(torch.int16)) and torch.equal(a[t][1].view(torch.int16), b[t][1].view(torch.int16))
               for t in a)


@pytest.mark.parametrize("R,Rp", [(33, 64), (64, 64), (230, 256), (33, 40)])
def test_grouped_launch_both_operand_forms(R, Rp):
    """Eight weight-gradient problems that between them take the tile widths 4, 2 and 1, gated and ungated at each width.
    Row-contiguous form (small_gemm_group_kernel<MASK, false>): within the fp64 bound, bit-equal to eight single launches, and
    unchanged by an empty item in the middle of the group.  Contraction-contiguous form (<MASK, true>) on transposed, zero-padded
    [C, Rp] copies with the gate folded into the copy (mpf_transpose_group_bf16, all sixteen in one launch): within the bound and
    bit-equal to the row-contiguous form — what csrc/decoder_layer.hip says of decoder_dw_group = 2: the same 32-row contraction
    steps on the same waves, the padding adds zeros.  Rp = 40 for R = 33 (not a multiple of 32) is the masked transposed form."""
    from mp_former_amd.small_linear import MpfSmallGemmItem, MpfTransposeItem
    L = _lib()
    dev = _dev()
    assert tuple(_nj(I, J) for I, J, _ in GROUP) == GROUP_NJ
    assert {(nj, gated) for nj, (_, _, gated) in zip(GROUP_NJ, GROUP)} == set(itertools.product((1, 2, 4), (False, True)))
    P = _GroupProblem(R, 5000 + R)
    n = len(GROUP)

    grouped = P.outputs()
    items = (MpfSmallGemmItem * n)()
    for t in range(n):
        P.item(items[t], t, grouped[t])
    _group_launch(items, n)
    P.check(grouped, "group, row-contiguous")

    single = P.outputs()
    one = (MpfSmallGemmItem * 1)()
    for t in range(n):
        P.item(one[0], t, single[t])
        m = one[0]
        code = L.lib().mpf_small_gemm_bf16(m.a, m.a_rs, m.a_ks, m.gate, m.b, m.b_rs, m.b_ks, None, None, 0, m.c, m.ldc, m.rowsum_a, m.I, m.J, m.Kc,
                                           0, L.stream_ptr(dev))
        assert code == 0, L.lib().mpf_last_error().decode()
    torch.cuda.synchronize()
    assert _same(grouped, single)

    # an empty item (J = 0) in the middle: the other seven problems come out the same
    rest = [0, 1, 2, 3, 5, 6, 7]
    holed = P.outputs(rest)
    items = (MpfSmallGemmItem * n)()
    for slot, t in zip([0, 1, 2, 3, 5, 6, 7], rest):
        P.item(items[slot], t, holed[t])
    P.item(items[4], 4, grouped[4])             # (the buffers of problem 4; with J = 0 nothing of them is used)
    items[4].J = 0
    before = grouped[4][0].clone(), grouped[4][1].clone()
    _group_launch(items, n)
    assert _same(holed, {t: grouped[t] for t in rest})
    assert torch.equal(before[0].view(torch.int16), grouped[4][0].view(torch.int16)) and torch.equal(before[1].view(torch.int16), grouped[4][1].view(torch.int16))

    # the transposed copies: dy^T (gated) and x^T of every problem, sixteen matrices in one launch
    tr = (MpfTransposeItem * (2 * n))()
    copies = []
    for t, (I, J, gated) in enumerate(GROUP):
        (dy, ld_a), (x, ld_b), gate = P.ops[t]
        dyT, xT = _filled(I * Rp + 64, None, None, SENT), _filled(J * Rp + 64, None, None, SENT)
        a, b = tr[2 * t], tr[2 * t + 1]
        a.src, a.gate, a.dst, a.ld, a.R, a.C = dy.data_ptr(), (gate[0].data_ptr() if gate else None), dyT.data_ptr(), ld_a, R, I
        b.src, b.gate, b.dst, b.ld, b.R, b.C = x.data_ptr(), None, xT.data_ptr(), ld_b, R, J
        copies.append((dyT, xT))
    code = L.lib().mpf_transpose_group_bf16(tr, 2 * n, Rp, L.stream_ptr(dev))
    assert code == 0, L.lib().mpf_last_error().decode()
    transposed = P.outputs()
    items = (MpfSmallGemmItem * n)()
    for t, (I, J, _) in enumerate(GROUP):
        it, (dyT, xT), (dw, db) = items[t], copies[t], transposed[t]
        it.a, it.gate, it.b, it.c, it.rowsum_a = dyT.data_ptr(), None, xT.data_ptr(), dw.data_ptr(), db.data_ptr()
        it.a_rs, it.a_ks, it.a_bs, it.b_rs, it.b_ks, it.ldc = Rp, 1, 0, Rp, 1, J + 12
        it.a_blk, it.I, it.J, it.Kc = 0, I, J, Rp
    _group_launch(items, n)
    for (I, J, _), (dyT, xT) in zip(GROUP, copies):
        assert bool((dyT[I * Rp:] == SENT).all()) and bool((xT[J * Rp:] == SENT).all())
    P.check(transposed, f"group, contraction-contiguous Rp {Rp}")
    assert _same(transposed, grouped)


# ---- 5: the switch at layer level ---------------------------------------------------------------------------------------------------
_layer_cache = {}


def _layer(case, packed, v, fresh=False):
    """all gradients of one native decoder layer with decoder_dw_group = v (the switch goes back to 2 afterwards)"""
    key = (case, packed, v)
    if fresh or key not in _layer_cache:
        L = _lib()
        L.set_option("decoder_dw_group", v)
        try:
            res = _run_native(_problem(case), _dev(), packed=packed)
            torch.cuda.synchronize()
        finally:
            L.set_option("decoder_dw_group", 2)
        if fresh:
            return res
        _layer_cache[key] = res
    return _layer_cache[key]


@pytest.mark.parametrize("v", [0, 1, 2])
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=["Qt7-N3-S77-F96", "Qt33-N2-S200-F2048"])
def test_decoder_dw_group_settings_agree_bit_for_bit(case, packed, v):
    """mpf_set_option("decoder_dw_group", v): one launch per weight gradient (0), one grouped launch on the row-contiguous operands
    (1), grouped transposes + one grouped launch on the contraction-contiguous copies (2, the default).  The 22 parameter gradients
    are bit-equal across the three, and so are the activation gradients, which do not depend on the switch.  (v = 2 is compared
    with a second run of itself.)"""
    assert case[:4] in ((7, 3, 77, 96), (33, 2, 200, 2048))
    base = _layer(case, packed, 2)
    got = _layer(case, packed, v, fresh=v == 2)
    names = tuple("d_" + n for n in NAMES) + ACTS
    assert len(names) == 22 + 4
    for n in names:
        assert got[n].dtype == base[n].dtype and got[n].shape == base[n].shape, n
        assert bool(torch.isfinite(got[n].float()).all()), n
        same = torch.equal(got[n].contiguous().view(torch.int32 if got[n].dtype == torch.float32 else torch.int16),
                           base[n].contiguous().view(torch.int32 if got[n].dtype == torch.float32 else torch.int16))
        assert same, f"{n}: decoder_dw_group {v} differs from 2 in {int((got[n] != base[n]).sum())} elements"
    assert float(got["d_ff_w1"].float().abs().max()) > 0 and float(got["d_sa_wk"].float().abs().max()) > 0


# ---- 6: argument checks (return codes only: nothing is launched) ---------------------------------------------------------------------
def _arena():
    """operands large enough for every call below, results sentinel-filled"""
    dev = _dev()
    return torch.zeros(1 << 16, dtype=BF16, device=dev), torch.full((1 << 16,), SENT, dtype=BF16, device=dev)


def test_blocked_gemm_rejects_bad_blocks():
    L = _lib()
    a, c = _arena()
    st = L.stream_ptr(_dev())
    f = L.lib().mpf_small_gemm_bf16_blocked
    p, q = a.data_ptr(), c.data_ptr()
    # the accepted call these are variations of (16 x 64 x 64, blocked contraction and blocked columns)
    assert f(p, 32, 1, 32, 1024, None, p, 64, 1, None, None, 0, q, 64, 64, 2048, None, 16, 64, 64, 0, st) == 0
    torch.cuda.synchronize()
    c.fill_(SENT)
    assert f(p, 48, 1, 48, 1024, None, p, 64, 1, None, None, 0, q, 64, 0, 0, None, 16, 64, 96, 0, st) == E_SHAPE           # a_blk = 48
    assert f(p, 64, 1, 0, 0, None, p, 64, 1, None, None, 0, q, 32, 32, 2048, None, 16, 64, 64, 0, st) == E_SHAPE            # c_blk = 32
    assert f(p, 64, 1, 0, 0, None, p, 64, 1, None, p, 64, q, 64, 64, 2048, None, 16, 64, 64, 0, st) == E_SHAPE              # c_blk with c_in
    assert f(p, 32, 1, 32, 1024, None, p, 40, 1, None, None, 0, q, 64, 0, 0, None, 16, 64, 40, 0, st) == E_SHAPE            # blocked contraction, Kc = 40
    assert "small_gemm" in L.lib().mpf_last_error().decode()
    torch.cuda.synchronize()
    assert bool((c == SENT).all())


def test_group_rejects_mixed_forms_gates_and_counts():
    from mp_former_amd.small_linear import MpfSmallGemmItem
    L = _lib()
    a, c = _arena()
    st = L.stream_ptr(_dev())
    f = L.lib().mpf_small_gemm_bf16_group

    def items(*specs):
        arr = (MpfSmallGemmItem * len(specs))()
        for it, (ct, Kc, gate) in zip(arr, specs):
            it.a, it.gate, it.b, it.c, it.rowsum_a = a.data_ptr(), (a.data_ptr() if gate else None), a.data_ptr(), c.data_ptr(), None
            it.a_rs, it.a_ks, it.b_rs, it.b_ks = (64, 1, 64, 1) if ct else (1, 16, 1, 16)
            it.a_bs, it.ldc, it.a_blk, it.I, it.J, it.Kc = 0, 16, 0, 16, 16, Kc
        return arr

    row, ct = (False, 32, False), (True, 32, False)
    assert f(items(row, row), 2, st) == 0 and f(items(ct, ct), 2, st) == 0          # the accepted calls these are variations of
    torch.cuda.synchronize()
    c.fill_(SENT)
    assert f(items(ct, row), 2, st) == E_SHAPE and f(items(row, ct), 2, st) == E_SHAPE          # mixed operand forms
    assert f(items(ct, (True, 32, True)), 2, st) == E_SHAPE                                     # a gate on a transposed item
    assert f(items(row, (False, 33, False)), 2, st) == E_SHAPE                                  # Kc % 32 disagrees
    assert f(items(ct, (True, 40, False)), 2, st) == E_SHAPE
    assert f(items(*[row] * 9), 9, st) == E_SHAPE                                               # nine items
    torch.cuda.synchronize()
    assert bool((c == SENT).all())


def test_transpose_group_rejects_bad_shapes_and_counts():
    from mp_former_amd.small_linear import MpfTransposeItem
    L = _lib()
    a, c = _arena()
    st = L.stream_ptr(_dev())
    f = L.lib().mpf_transpose_group_bf16

    def items(n, R=8, C=16, ld=16):
        arr = (MpfTransposeItem * n)()
        for it in arr:
            it.src, it.gate, it.dst, it.ld, it.R, it.C = a.data_ptr(), None, c.data_ptr(), ld, R, C
        return arr

    assert f(items(16), 16, 8, st) == 0                 # the accepted call these are variations of
    torch.cuda.synchronize()
    c.fill_(SENT)
    assert f(items(1, R=9), 1, 8, st) == E_SHAPE        # R > Rp
    assert f(items(1, C=12), 1, 8, st) == E_SHAPE
    assert f(items(1), 1, 12, st) == E_SHAPE            # Rp = 12
    assert f(items(17), 17, 8, st) == E_SHAPE           # seventeen items
    torch.cuda.synchronize()
    assert bool((c == SENT).all())


@pytest.mark.parametrize("I,J", [(0, 16), (16, 0), (0, 0)])
def test_empty_problems_return_zero_and_write_nothing(I, J):
    from mp_former_amd.small_linear import MpfSmallGemmItem
    L = _lib()
    a, c = _arena()
    st = L.stream_ptr(_dev())
    p, q = a.data_ptr(), c.data_ptr()
    rs = q + 2 * (1 << 15)
    assert L.lib().mpf_small_gemm_bf16(p, 32, 1, None, p, 32, 1, None, None, 0, q, 16, rs, I, J, 32, 0, st) == 0
    assert L.lib().mpf_small_gemm_bf16_blocked(p, 32, 1, 32, 1024, None, p, 32, 1, None, None, 0, q, 64, 64, 2048, rs, I, J, 32, 0, st) == 0
    items = (MpfSmallGemmItem * 2)()
    for it in items:
        it.a, it.gate, it.b, it.c, it.rowsum_a = p, None, p, q, rs
        it.a_rs, it.a_ks, it.a_bs, it.b_rs, it.b_ks, it.ldc, it.a_blk, it.I, it.J, it.Kc = 1, 16, 0, 1, 16, 16, 0, I, J, 32
    assert L.lib().mpf_small_gemm_bf16_group(items, 2, st) == 0
    torch.cuda.synchronize()
    assert bool((c == SENT).all())
