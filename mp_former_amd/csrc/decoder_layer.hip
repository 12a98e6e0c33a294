// One transformer-decoder layer (cross-attention, self-attention, FFN, post-norm residuals) issued
// from native code: the host side of include/mpformer_hip.h MpfDecoderLayer.  No kernels here — the
// layer is a fixed sequence of the library's own entry points (small_gemm.hip, attn.hip,
// elementwise.hip); what this file removes is the per-kernel cost of a Python autograd node (~20 us of
// host time against 3-6 us of GPU time per launch), which made the decoder launch-bound.
// Reference: mask2former_transformer_decoder.py:1784-1800 (the layer loop), :42-52, :100-112, :165-169.
// The same sequence serves the clip decoder's layer, which adds learned query positions to the query of the cross-attention
// and to the query and key of the self-attention (video_mask2former_transformer_decoder.py:415, :421; MpfDecoderLayerPos, the
// mpf_decoder_layer_pos_* entry points): layer_forward / layer_backward take the position record or nullptr, and without it
// issue exactly the image layer's launches.  The two position kernels are in query_pos.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mpf_common.h"

namespace {

constexpr int kE = 256;
constexpr int kMaxDw = 8;        // weight-gradient problems per layer (6 with packed in-projection gradients — 7 with query positions — 8 without)
constexpr int kMaxOperands = 16;  // their distinct operands (14, 15 with query positions): what one mpf_transpose_group_bf16 launch takes

struct Carve {
    char* p;
    size_t used = 0;
    explicit Carve(void* base) : p(static_cast<char*>(base)) {}
    template <typename T>
    T* take(size_t count)
    {
        T* r = reinterpret_cast<T*>(p + used);
        used += mpf::align256(count * sizeof(T));
        return r;
    }
};

struct FwdScratch {
    void *vT_c, *vT_s, *t;
    float *x1, *x2;
    size_t bytes;
};

FwdScratch fwd_scratch(void* base, int Qt, int N, int S)
{
    Carve c(base);
    FwdScratch f;
    const size_t R = (size_t)Qt * N;
    f.vT_c = c.take<uint16_t>((size_t)N * kE * S);
    f.vT_s = c.take<uint16_t>((size_t)N * kE * Qt);
    f.t = c.take<uint16_t>(R * kE);
    f.x1 = c.take<float>(R * kE);
    f.x2 = c.take<float>(R * kE);
    f.bytes = c.used;
    return f;
}

struct BwdScratch {
    // dt3 / dt2 / dt1: the gradients entering the FFN / self-attention / cross-attention output projections, dq / dq_c the
    // in-projection gradients of the two attentions — each in its own buffer, because the weight gradients that read them
    // are issued together at the end of the layer (one grouped launch)
    void *dt3, *dt2, *dt1, *dxb, *dh, *dout, *dq, *dk_s, *dv_s, *dq_c, *qT, *doT;
    float *ds_a, *ds_b, *delta;
    void* aux;                   // aux operands of the attention dK / dV kernel (mpf_attn_bwd_aux_bytes: the larger of the two attentions)
    size_t aux_bytes;
    uint16_t* tbuf;              // transposed [C, Rp] copies of the weight-gradient operands (2 F + 13 * 256 columns; 14 with positions)
    void* ln_ws;                 // per-workgroup partial sums of the three LayerNorms' parameter gradients, ln_ws_bytes each
    size_t ln_ws_bytes;
    void *dxq0, *dxq1;           // with query positions: the gradients of the operands bf16(x0 + qpos), bf16(x1 + qpos)
    size_t bytes;
};

BwdScratch bwd_scratch(void* base, int Qt, int N, int H, int F, int S, bool pos)
{
    Carve c(base);
    BwdScratch b;
    const size_t R = (size_t)Qt * N;
    const size_t LqP = (size_t)((Qt + 31) / 32 * 32);
    b.dt3 = c.take<uint16_t>(R * kE);
    b.dt2 = c.take<uint16_t>(R * kE);
    b.dt1 = c.take<uint16_t>(R * kE);
    b.dxb = c.take<uint16_t>(R * kE);
    b.dh = c.take<uint16_t>(R * F);
    b.dout = c.take<uint16_t>(R * kE);
    b.dq = c.take<uint16_t>(R * kE);
    b.dk_s = c.take<uint16_t>(R * kE);
    b.dv_s = c.take<uint16_t>(R * kE);
    b.dq_c = c.take<uint16_t>(R * kE);
    b.qT = c.take<uint16_t>((size_t)N * kE * LqP);
    b.doT = c.take<uint16_t>((size_t)N * kE * LqP);
    b.ds_a = c.take<float>(R * kE);
    b.ds_b = c.take<float>(R * kE);
    b.delta = c.take<float>((size_t)N * H * Qt);
    b.aux_bytes = std::max(mpf_attn_bwd_aux_bytes(Qt, S, N, H, N), mpf_attn_bwd_aux_bytes(Qt, Qt, N, H, 1));
    b.aux = c.take<char>(b.aux_bytes);
    b.tbuf = c.take<uint16_t>((size_t)(2 * F + (pos ? 14 : 13) * kE) * ((R + 31) / 32 * 32));
    b.ln_ws_bytes = mpf::align256(mpf_res_ln256_backward_workspace_bytes((int)R));
    b.ln_ws = c.take<char>(3 * b.ln_ws_bytes);
    b.dxq0 = pos ? c.take<uint16_t>(R * kE) : nullptr;       // (behind everything else: the layout without positions is unchanged)
    b.dxq1 = pos ? c.take<uint16_t>(R * kE) : nullptr;
    b.bytes = c.used;
    return b;
}

// P != nullptr: the layer takes query positions (the record is checked here too); xb0 is then not read
int check_layer(const MpfDecoderLayer* L, const char* who, const MpfDecoderLayerPos* P = nullptr, bool backward = false)
{
    if (!L) return mpf::fail(MPF_E_NULL, who);
    if (P && (!P->qpos || !P->xq0 || !P->xq1 || (backward && !P->d_qpos)))
        return mpf::fail(MPF_E_NULL, "decoder_layer: NULL buffer in MpfDecoderLayerPos");
    if (L->Qt <= 0 || L->N <= 0 || L->S <= 0 || L->ffn_dim <= 0 || L->H * 32 != kE || L->ffn_dim % 32)
        return mpf::fail(MPF_E_SHAPE, "decoder_layer: needs H * 32 == 256 channels, positive sizes, ffn_dim % 32 == 0");
    if (mpf::any_null({L->ca_wq, L->ca_bq, L->ca_wo, L->ca_bo, L->ca_gamma, L->ca_beta, L->sa_wq, L->sa_bq, L->sa_wk, L->sa_bk,
                       L->sa_wv, L->sa_bv, L->sa_wo, L->sa_bo, L->sa_gamma, L->sa_beta, L->ff_w1, L->ff_b1, L->ff_w2, L->ff_b2,
                       L->ff_gamma, L->ff_beta, L->x0, P ? L->x0 : L->xb0, L->k_c, L->v_c, L->mask_c, L->q_c, L->kT_c, L->o_c, L->lse_c,
                       L->s1, L->mean1, L->rstd1, L->xb1, L->q_s, L->k_s, L->v_s, L->kT_s, L->o_s, L->lse_s, L->s2, L->mean2,
                       L->rstd2, L->xb2, L->h, L->s3, L->mean3, L->rstd3, L->scratch, L->attn_ws}))
        return mpf::fail(MPF_E_NULL, "decoder_layer: NULL buffer in MpfDecoderLayer");
    return 0;
}

// y[R, J] = x[R, Kc] . w[J, Kc]^T + b (ReLU)
int lin_fwd(const void* x, const void* w, const void* b, void* y, int R, int J, int Kc, int relu, void* st)
{
    return mpf_small_gemm_bf16(x, Kc, 1, nullptr, w, Kc, 1, b, nullptr, 0, y, J, nullptr, R, J, Kc, relu, st);
}

// dx[R, Kin] = (dy[R, J] gated) . w[J, Kin] (+ acc)
int lin_dx(const void* dy, const void* gate, const void* w, const void* acc, void* dx, int R, int J, int Kin, void* st)
{
    return mpf_small_gemm_bf16(dy, J, 1, gate, w, 1, Kin, nullptr, acc, Kin, dx, Kin, nullptr, R, Kin, J, 0, st);
}

// q | k | v of the self-attention stand side by side in memory (packed in_proj weight / bias, the three activation buffers, the
// three gradient buffers, the three weight-gradient destinations): the three GEMMs of each kind become ONE blocked GEMM
bool side_by_side(const void* q, const void* k, const void* v, size_t bytes)
{
    return k == static_cast<const char*>(q) + bytes && v == static_cast<const char*>(q) + 2 * bytes;
}
constexpr size_t kWeightBytes = (size_t)kE * kE * 2, kBiasBytes = (size_t)kE * 2;
size_t act_bytes(int R) { return (size_t)R * kE * 2; }

bool packed_weights(const MpfDecoderLayer* L)
{
    return side_by_side(L->sa_wq, L->sa_wk, L->sa_wv, kWeightBytes) && side_by_side(L->sa_bq, L->sa_bk, L->sa_bv, kBiasBytes);
}
bool packed_acts(const MpfDecoderLayer* L, int R) { return side_by_side(L->q_s, L->k_s, L->v_s, act_bytes(R)); }
bool packed_dw_dst(const MpfDecoderLayerGrad* G)
{
    return side_by_side(G->d_sa_wq, G->d_sa_wk, G->d_sa_wv, kWeightBytes) && side_by_side(G->d_sa_bq, G->d_sa_bk, G->d_sa_bv, kBiasBytes);
}

}  // namespace

namespace {
// A/B switches (mpf_set_option): decoder_dw_group = 0 issues the weight gradients as separate launches (round-1 form), 1 = one grouped
// launch on the row-contiguous operands (round 2), 2 = grouped transposes + one grouped launch on contraction-contiguous copies
int g_dw_group = 2;
// decoder_row_chain = 0: output projection, residual LayerNorm, decoder_norm and the mask_embed layers as separate launches
// (the form of rounds 2-4); 1: the row-local chains of row_chain.hip
int g_row_chain = 1;
}  // namespace

namespace mpf {
int set_decoder_option(const char* key, int v)
{
    if (!strcmp(key, "decoder_dw_group")) { if (v < 0 || v > 2) return -1; g_dw_group = v; return 0; }
    if (!strcmp(key, "decoder_row_chain")) { if (v < 0 || v > 1) return -1; g_row_chain = v; return 0; }
    return 1;
}
}  // namespace mpf

#define MPF_TRY(expr)                \
    do {                             \
        const int rc_ = (expr);      \
        if (rc_ != 0) return rc_;    \
    } while (0)

extern "C" uint64_t mpf_decoder_layer_struct_bytes(int which)
{
    return which == 0 ? sizeof(MpfDecoderLayer) : sizeof(MpfDecoderLayerGrad);
}

extern "C" uint64_t mpf_decoder_layer_scratch_bytes(int Qt, int N, int H, int S, int ffn_dim, int backward)
{
    if (Qt <= 0 || N <= 0 || H <= 0 || S <= 0 || ffn_dim <= 0) return 0;
    return backward ? bwd_scratch(nullptr, Qt, N, H, ffn_dim, S, false).bytes : fwd_scratch(nullptr, Qt, N, S).bytes;
}

extern "C" uint64_t mpf_decoder_layer_pos_struct_bytes(void) { return sizeof(MpfDecoderLayerPos); }

extern "C" uint64_t mpf_decoder_layer_pos_scratch_bytes(int Qt, int N, int H, int S, int ffn_dim, int backward)
{
    if (Qt <= 0 || N <= 0 || H <= 0 || S <= 0 || ffn_dim <= 0) return 0;
    return backward ? bwd_scratch(nullptr, Qt, N, H, ffn_dim, S, true).bytes : fwd_scratch(nullptr, Qt, N, S).bytes;
}

namespace {

// The forward of both forms.  P == nullptr: the image decoder's layer (query, key and value operands are the stream's bf16
// copies xb0 / xb1); P != nullptr: query positions (video_mask2former_transformer_decoder.py:415, :421) — the cross-attention
// query from xq0 = bf16(x0 + qpos), the self-attention query and key from xq1 = bf16(x1 + qpos), its value from xb1.
int layer_forward(const MpfDecoderLayer* L, const MpfDecoderLayerPos* P, void* st)
{
    MPF_TRY(check_layer(L, "decoder_layer_forward: NULL layer", P, false));
    if (!L->x3 && !L->xb3) return mpf::fail(MPF_E_NULL, "decoder_layer_forward: no output buffer");
    const int Qt = L->Qt, N = L->N, H = L->H, S = L->S, F = L->ffn_dim, R = Qt * N;
    const FwdScratch f = fwd_scratch(L->scratch, Qt, N, S);
    if (L->scratch_bytes < f.bytes) return mpf::fail(MPF_E_SHAPE, "decoder_layer_forward: scratch too small");
    const float scale = 0.17677669529663687f;       // 1 / sqrt(32)
    // output projection + residual LayerNorm of an attention block: the row-local chain of row_chain.hip, or two launches
    const auto proj_ln = [&](auto o, auto wo, auto bo, auto x_in, auto gamma, auto beta, auto s, auto x_out, auto xb, auto mean, auto rstd) {
        if (g_row_chain) return mpf_lin256_res_ln_forward(o, wo, bo, x_in, gamma, beta, s, x_out, xb, mean, rstd, R, L->eps, st);
        MPF_TRY(lin_fwd(o, wo, bo, f.t, R, kE, kE, 0, st));
        return mpf_res_ln256_forward(x_in, f.t, MPF_BF16, gamma, beta, s, x_out, xb, mean, rstd, R, L->eps, nullptr, 0, nullptr, st);
    };
    // cross-attention (:1784-1789) + post-norm
    if (P) MPF_TRY(mpf_qpos_operand_forward(L->x0, P->qpos, P->xq0, Qt, N, st));
    MPF_TRY(lin_fwd(P ? P->xq0 : L->xb0, L->ca_wq, L->ca_bq, L->q_c, R, kE, kE, 0, st));
    MPF_TRY(mpf_attn_transpose2_strided(L->k_c, L->v_c, L->kv_row_stride, L->kv_img_stride, L->kT_c, f.vT_c, S, S, N, kE, st));
    MPF_TRY(mpf_attn_forward_kv(L->q_c, L->k_c, L->kv_row_stride, L->kv_img_stride, f.vT_c, L->mask_c, 1, L->o_c, L->lse_c, Qt, S, N,
                                H, 32, scale, L->attn_ws, L->attn_ws_bytes, st));
    MPF_TRY(proj_ln(L->o_c, L->ca_wo, L->ca_bo, L->x0, L->ca_gamma, L->ca_beta, L->s1, f.x1, L->xb1, L->mean1, L->rstd1));
    // self-attention (:1791-1795) + post-norm
    const bool packed = packed_weights(L) && packed_acts(L, R);
    const void* xqk = L->xb1;                        // operand of the query and key projections
    if (P) {
        MPF_TRY(mpf_qpos_operand_forward(f.x1, P->qpos, P->xq1, Qt, N, st));
        xqk = P->xq1;
    }
    if (packed) {
        // [q_s | k_s | v_s] = xb1 . W_in^T as one blocked GEMM; with positions [q_s | k_s] = xq1 . [Wq | Wk]^T, v_s = xb1 . Wv^T
        MPF_TRY(mpf_small_gemm_bf16_blocked(xqk, kE, 1, 0, 0, nullptr, L->sa_wq, kE, 1, L->sa_bq, nullptr, 0, L->q_s, kE, kE,
                                            (int64_t)R * kE, nullptr, R, (P ? 2 : 3) * kE, kE, 0, st));
        if (P) MPF_TRY(lin_fwd(L->xb1, L->sa_wv, L->sa_bv, L->v_s, R, kE, kE, 0, st));
    } else {
        MPF_TRY(lin_fwd(xqk, L->sa_wq, L->sa_bq, L->q_s, R, kE, kE, 0, st));
        MPF_TRY(lin_fwd(xqk, L->sa_wk, L->sa_bk, L->k_s, R, kE, kE, 0, st));
        MPF_TRY(lin_fwd(L->xb1, L->sa_wv, L->sa_bv, L->v_s, R, kE, kE, 0, st));
    }
    MPF_TRY(mpf_attn_transpose2(L->k_s, L->v_s, L->kT_s, f.vT_s, Qt, Qt, N, kE, st));
    MPF_TRY(mpf_attn_forward(L->q_s, L->k_s, f.vT_s, L->mask_s, 0, L->o_s, L->lse_s, Qt, Qt, N, H, 32, scale, L->attn_ws,
                             L->attn_ws_bytes, st));
    MPF_TRY(proj_ln(L->o_s, L->sa_wo, L->sa_bo, f.x1, L->sa_gamma, L->sa_beta, L->s2, f.x2, L->xb2, L->mean2, L->rstd2));
    // FFN (:1798-1800) + post-norm
    MPF_TRY(lin_fwd(L->xb2, L->ff_w1, L->ff_b1, L->h, R, F, kE, 1, st));
    MPF_TRY(lin_fwd(L->h, L->ff_w2, L->ff_b2, f.t, R, kE, F, 0, st));
    MPF_TRY(mpf_res_ln256_forward(f.x2, f.t, MPF_BF16, L->ff_gamma, L->ff_beta, L->s3, L->x3, L->xb3, L->mean3, L->rstd3, R,
                                  L->eps, nullptr, 0, nullptr, st));
    return 0;
}

// The weight gradients of a layer, stated once along the backward chain: the distinct [R, C] operands, in the order of their
// transposed copies, and one problem per gradient,  dw[J, Kin] = (dy gated)^T . x,  db[J] = column sums of (dy gated).  They depend
// only on buffers that the chain leaves alone (each dY in its own scratch buffer), so issue() runs after the chain.
struct DwList {
    struct Operand { const void *src, *gate; int C; } op[kMaxOperands];
    struct Problem { int dy, x; void *dw, *db; int J, Kin, blocks; } pr[kMaxDw];
    int nop = 0, npr = 0, lost = 0;          // lost: an operand or a problem that did not fit (refused by issue())
    int operand(const void* src, int C = kE, const void* gate = nullptr) { if (nop == kMaxOperands) return lost = 1, 0; op[nop] = {src, gate, C}; return nop++; }
    // blocks > 1: dy is that many [R, 256] operands stated one after the other, their buffers R * 256 elements apart, and dw / db
    // the packed [blocks * 256, Kin] / [blocks * 256] destination
    void add(int dy, int x, void* dw, void* db, int blocks = 1)
    {
        if (npr == kMaxDw) lost = 1;
        else pr[npr++] = {dy, x, dw, db, blocks * op[dy].C, op[x].C, blocks};
    }

    // form = decoder_dw_group.  0: one launch per problem and 1: one grouped launch, both on the operands as they lie (both
    // row-contiguous); 2: the weight gradients contract over the ROWS of dY and x: on transposed [C, Rp] copies (one grouped launch)
    // both operands are contraction-contiguous, i.e. 16-byte fragment loads instead of eight 2-byte ones per fragment; same 32-row
    // contraction steps on the same waves, zero padding: bit-identical to the row-contiguous form.  The copies of a blocked dy are
    // adjacent [256, Rp] blocks by construction, one [blocks * 256, Rp] operand.
    int issue(int form, int R, uint16_t* tbuf, void* st) const
    {
        if (lost) return mpf::fail(MPF_E_SHAPE, "decoder_layer_backward: more weight-gradient operands or problems than one launch takes");
        const int Rp = (R + 31) / 32 * 32;
        const uint16_t* copy[kMaxOperands];
        if (form == 2) {
            MpfTransposeItem tr[kMaxOperands];
            for (int t = 0; t < nop; ++t) {
                tr[t].src = op[t].src; tr[t].gate = op[t].gate; tr[t].dst = tbuf; tr[t].ld = op[t].C; tr[t].R = R; tr[t].C = op[t].C;
                copy[t] = tbuf;
                tbuf += (size_t)op[t].C * Rp;
            }
            MPF_TRY(mpf_transpose_group_bf16(tr, nop, Rp, st));
        }
        MpfSmallGemmItem it[kMaxDw];
        for (int t = 0; t < npr; ++t) {
            const Problem& p = pr[t];
            MpfSmallGemmItem& m = it[t];
            m.c = p.dw; m.rowsum_a = p.db; m.ldc = p.Kin; m.I = p.J; m.J = p.Kin;
            if (form == 2) {
                m.a = copy[p.dy]; m.gate = nullptr; m.b = copy[p.x];
                m.a_rs = Rp; m.a_ks = 1; m.a_bs = 0; m.b_rs = Rp; m.b_ks = 1; m.a_blk = 0; m.Kc = Rp;
            } else {
                m.a = op[p.dy].src; m.gate = op[p.dy].gate; m.b = op[p.x].src;
                m.a_rs = 1; m.a_ks = op[p.dy].C; m.a_bs = p.blocks > 1 ? (int64_t)R * kE : 0; m.b_rs = 1; m.b_ks = p.Kin;
                m.a_blk = p.blocks > 1 ? kE : 0; m.Kc = R;
            }
        }
        if (form) return mpf_small_gemm_bf16_group(it, npr, st);
        for (int t = 0; t < npr; ++t)
            MPF_TRY(mpf_small_gemm_bf16_blocked(it[t].a, it[t].a_rs, it[t].a_ks, it[t].a_blk, it[t].a_bs, it[t].gate, it[t].b, it[t].b_rs,
                                                it[t].b_ks, nullptr, nullptr, 0, it[t].c, it[t].ldc, 0, 0, it[t].rowsum_a, it[t].I,
                                                it[t].J, it[t].Kc, 0, st));
        return 0;
    }
};

// The backward of both forms (P as in layer_forward).
int layer_backward(const MpfDecoderLayer* L, const MpfDecoderLayerPos* P, const MpfDecoderLayerGrad* G, void* st)
{
    MPF_TRY(check_layer(L, "decoder_layer_backward: NULL layer", P, true));
    if (!G) return mpf::fail(MPF_E_NULL, "decoder_layer_backward: NULL grad");
    if (!G->g_x3 && !G->g_xb3) return mpf::fail(MPF_E_NULL, "decoder_layer_backward: no upstream gradient");
    if (mpf::any_null({G->d_x0, P ? (const void*)G->d_x0 : G->d_xb0,         // (d_xb0: no reader, no gradient with positions)
                       G->d_k_c, G->d_v_c, G->d_ca_wq, G->d_ca_bq, G->d_ca_wo, G->d_ca_bo, G->d_sa_wq, G->d_sa_bq, G->d_sa_wk, G->d_sa_bk,
                       G->d_sa_wv, G->d_sa_bv, G->d_sa_wo, G->d_sa_bo, G->d_ff_w1, G->d_ff_b1, G->d_ff_w2, G->d_ff_b2, G->d_ln}))
        return mpf::fail(MPF_E_NULL, "decoder_layer_backward: NULL buffer in MpfDecoderLayerGrad");
    const int Qt = L->Qt, N = L->N, H = L->H, S = L->S, F = L->ffn_dim, R = Qt * N;
    const int LqP = (Qt + 31) / 32 * 32;
    const BwdScratch b = bwd_scratch(L->scratch, Qt, N, H, F, S, P != nullptr);
    if (L->scratch_bytes < b.bytes) return mpf::fail(MPF_E_SHAPE, "decoder_layer_backward: scratch too small");
    const float scale = 0.17677669529663687f;
    // q | k | v as one problem.  dX needs the packed weight and adjacent gradient buffers.  dW needs adjacent destinations, and
    // adjacent gradient buffers where it reads them as they lie (the transposed copies of dq | dk | dv are adjacent by construction)
    const bool grads_packed = side_by_side(b.dq, b.dk_s, b.dv_s, act_bytes(R));
    const bool dx_packed = packed_weights(L) && grads_packed;
    const bool dw_packed = packed_dw_dst(G) && (g_dw_group == 2 || grads_packed);
    // LayerNorm parameter gradients: the three backward launches leave per-workgroup partial sums, ONE launch at the end of the
    // layer reduces them in a fixed order (no float atomics, nothing to zero)
    char* ln_part = static_cast<char*>(b.ln_ws);
    DwList W;
    // FFN block: x3 = LN(x2 + W2 relu(W1 xb2))
    if (G->g_x3_plus && !G->g_x3) return mpf::fail(MPF_E_NULL, "decoder_layer_backward: g_x3_plus without g_x3");
    MPF_TRY(mpf_res_ln256_backward_partial(L->s3, L->mean3, L->rstd3, L->ff_gamma, G->g_x3, G->g_xb3, G->g_x3_plus, b.ds_a, b.dt3, R,
                                           ln_part + 2 * b.ln_ws_bytes, b.ln_ws_bytes, st));
    MPF_TRY(lin_dx(b.dt3, nullptr, L->ff_w2, nullptr, b.dh, R, kE, F, st));
    const int dt3 = W.operand(b.dt3), h = W.operand(L->h, F);
    W.add(dt3, h, G->d_ff_w2, G->d_ff_b2);
    MPF_TRY(lin_dx(b.dh, L->h, L->ff_w1, nullptr, b.dxb, R, F, kE, st));
    const int dh = W.operand(b.dh, F, L->h), xb2 = W.operand(L->xb2);
    W.add(dh, xb2, G->d_ff_w1, G->d_ff_b1);
    // self-attention block: x2 = LN(x1 + Wo attn(Wq xb1, Wk xb1, Wv xb1))
    MPF_TRY(mpf_res_ln256_backward_partial(L->s2, L->mean2, L->rstd2, L->sa_gamma, b.ds_a, b.dxb, nullptr, b.ds_b, b.dt2, R,
                                           ln_part + b.ln_ws_bytes, b.ln_ws_bytes, st));
    MPF_TRY(lin_dx(b.dt2, nullptr, L->sa_wo, nullptr, b.dout, R, kE, kE, st));
    const int dt2 = W.operand(b.dt2), o_s = W.operand(L->o_s);
    W.add(dt2, o_s, G->d_sa_wo, G->d_sa_bo);
    MPF_TRY(mpf_attn_bwd_prep_aux(L->q_s, b.dout, L->o_s, L->lse_s, L->mask_s, 0, Qt, b.qT, b.doT, b.delta, b.aux, b.aux_bytes, Qt, LqP,
                                  N, H, st));
    MPF_TRY(mpf_attn_backward_kv_aux(L->q_s, L->k_s, L->v_s, 0, 0, L->kT_s, b.qT, b.dout, b.doT, L->mask_s, 0, L->lse_s, b.delta, b.dq,
                                     b.dk_s, b.dv_s, 0, 0, Qt, LqP, Qt, N, H, 32, scale, L->attn_ws, L->attn_ws_bytes, b.aux, st));
    void* dxqk = P ? b.dxq1 : b.dxb;                      // gradient of the operand of the query and key projections
    if (dx_packed) {
        // dxb = [dq | dk | dv] . W_in (contraction over the 768 packed outputs, blocked over the three buffers); with positions
        // dxq1 = [dq | dk] . [Wq | Wk] (contraction over 512), dxb = dv . Wv
        MPF_TRY(mpf_small_gemm_bf16_blocked(b.dq, kE, 1, kE, (int64_t)R * kE, nullptr, L->sa_wq, 1, kE, nullptr, nullptr, 0, dxqk, kE,
                                            0, 0, nullptr, R, kE, (P ? 2 : 3) * kE, 0, st));
        if (P) MPF_TRY(lin_dx(b.dv_s, nullptr, L->sa_wv, nullptr, b.dxb, R, kE, kE, st));
    } else {
        MPF_TRY(lin_dx(b.dq, nullptr, L->sa_wq, nullptr, dxqk, R, kE, kE, st));
        MPF_TRY(lin_dx(b.dk_s, nullptr, L->sa_wk, dxqk, dxqk, R, kE, kE, st));
        MPF_TRY(lin_dx(b.dv_s, nullptr, L->sa_wv, P ? nullptr : b.dxb, b.dxb, R, kE, kE, st));
    }
    const int dq = W.operand(b.dq), dk = W.operand(b.dk_s), dv = W.operand(b.dv_s), xb1 = W.operand(L->xb1);
    const int xqk = P ? W.operand(P->xq1) : xb1;          // operand of the query and key projections
    if (dw_packed && !P) {
        // dW_in [768, 256] = [dq | dk | dv]^T . xb1 and its 768 bias gradients as one problem
        W.add(dq, xb1, G->d_sa_wq, G->d_sa_bq, 3);
    } else if (dw_packed) {
        // [dWq | dWk] [512, 256] = [dq | dk]^T . xq1 as one problem, dWv = dv^T . xb1
        W.add(dq, xqk, G->d_sa_wq, G->d_sa_bq, 2);
        W.add(dv, xb1, G->d_sa_wv, G->d_sa_bv);
    } else {
        W.add(dq, xqk, G->d_sa_wq, G->d_sa_bq);
        W.add(dk, xqk, G->d_sa_wk, G->d_sa_bk);
        W.add(dv, xb1, G->d_sa_wv, G->d_sa_bv);
    }
    // cross-attention block: x1 = LN(x0 + Wo attn(Wq xb0, k_c, v_c)); with positions the gradient of bf16(x1 + qpos) joins the
    // fp32 gradient of x1 first (the sum autograd forms for the stream's two consumers)
    if (P) MPF_TRY(mpf::bf16_rows_add256(b.dxq1, b.ds_b, R, st));
    MPF_TRY(mpf_res_ln256_backward_partial(L->s1, L->mean1, L->rstd1, L->ca_gamma, b.ds_b, b.dxb, nullptr, G->d_x0, b.dt1, R, ln_part,
                                           b.ln_ws_bytes, st));
    MPF_TRY(mpf_ln_partial_reduce(ln_part, b.ln_ws_bytes, R, 3, G->d_ln, st));      // d_ln = [ca | sa | ff] x (dgamma, dbeta)
    MPF_TRY(lin_dx(b.dt1, nullptr, L->ca_wo, nullptr, b.dout, R, kE, kE, st));
    const int dt1 = W.operand(b.dt1), o_c = W.operand(L->o_c);
    W.add(dt1, o_c, G->d_ca_wo, G->d_ca_bo);
    MPF_TRY(mpf_attn_bwd_prep_aux(L->q_c, b.dout, L->o_c, L->lse_c, L->mask_c, 1, S, b.qT, b.doT, b.delta, b.aux, b.aux_bytes, Qt, LqP, N,
                                  H, st));
    MPF_TRY(mpf_attn_backward_kv_aux(L->q_c, L->k_c, L->v_c, L->kv_row_stride, L->kv_img_stride, L->kT_c, b.qT, b.dout, b.doT, L->mask_c,
                                     1, L->lse_c, b.delta, b.dq_c, G->d_k_c, G->d_v_c, G->dkv_row_stride, G->dkv_img_stride, Qt, LqP, S,
                                     N, H, 32, scale, L->attn_ws, L->attn_ws_bytes, b.aux, st));
    MPF_TRY(lin_dx(b.dq_c, nullptr, L->ca_wq, nullptr, P ? b.dxq0 : G->d_xb0, R, kE, kE, st));
    // the gradient of bf16(x0 + qpos) goes to the fp32 stream, and with that of bf16(x1 + qpos) to the positions
    if (P) MPF_TRY(mpf_qpos_backward(b.dxq0, b.dxq1, G->d_x0, P->d_qpos, Qt, N, st));
    const int dq_c = W.operand(b.dq_c), xq_c = W.operand(P ? P->xq0 : L->xb0);      // (the operand of the cross-attention's query projection)
    W.add(dq_c, xq_c, G->d_ca_wq, G->d_ca_bq);
    return W.issue(g_dw_group, R, b.tbuf, st);
}

}  // namespace

extern "C" int mpf_decoder_layer_forward(const MpfDecoderLayer* L, void* st) { return layer_forward(L, nullptr, st); }

extern "C" int mpf_decoder_layer_backward(const MpfDecoderLayer* L, const MpfDecoderLayerGrad* G, void* st) { return layer_backward(L, nullptr, G, st); }

extern "C" int mpf_decoder_layer_pos_forward(const MpfDecoderLayer* L, const MpfDecoderLayerPos* P, void* st)
{
    return P ? layer_forward(L, P, st) : mpf::fail(MPF_E_NULL, "decoder_layer_pos_forward: NULL position record");
}

extern "C" int mpf_decoder_layer_pos_backward(const MpfDecoderLayer* L, const MpfDecoderLayerPos* P, const MpfDecoderLayerGrad* G, void* st)
{
    return P ? layer_backward(L, P, G, st) : mpf::fail(MPF_E_NULL, "decoder_layer_pos_backward: NULL position record");
}

// The attention mask of the NEXT layer from this layer's residual stream (mask2former_transformer_decoder.py:1869-1875 with the
// prediction-head part of :1859-1866, detached as the reference detaches it): decoder_norm -> mask_embed MLP (ReLU after the first
// two layers) -> sign of the product with the features pooled to the level grid, MP rows and the all-masked-row rule applied by
// the mask-head kernel.  Five launches issued from one call: the python glue around them (five autograd-free ops, ten times per
// step) was 0.5 ms of launch-thread time at the one place of the step where the device waits for every launch.
extern "C" size_t mpf_next_attn_mask_scratch_bytes(int N, int Q)
{
    if (N <= 0 || Q <= 0) return 0;
    const size_t rows = (size_t)N * Q;
    return 3 * mpf::align256(rows * kE * 2) + 2 * mpf::align256(rows * 4);
}

extern "C" int mpf_next_attn_mask(const MpfNextMask* m, void* st)
{
    if (!m || mpf::any_null({m->x, m->ln_gamma, m->ln_beta, m->w0, m->w1, m->w2, m->pooled, m->out, m->flags, m->scratch}))
        return mpf::fail(MPF_E_NULL, "next_attn_mask: NULL buffer");
    if (m->N <= 0 || m->Q <= 0 || m->HW <= 0 || m->pad < 0) return mpf::fail(MPF_E_SHAPE, "next_attn_mask: bad sizes");
    if (m->scratch_bytes < mpf_next_attn_mask_scratch_bytes(m->N, m->Q)) return mpf::fail(MPF_E_SHAPE, "next_attn_mask: scratch too small");
    const int rows = m->N * m->Q;
    const size_t act = mpf::align256((size_t)rows * kE * 2), vec = mpf::align256((size_t)rows * 4);
    char* sc = static_cast<char*>(m->scratch);
    void* d16 = sc;                 // decoder_norm(x) in bf16; reused for the third layer's result
    void* e1 = sc + act;
    void* e2 = sc + 2 * act;
    float* mean = reinterpret_cast<float*>(sc + 3 * act);
    float* rstd = reinterpret_cast<float*>(sc + 3 * act + vec);
    if (g_row_chain && m->b0 && m->b1 && m->b2) {
        MPF_TRY(mpf_ln256_mlp3_forward(m->x, m->ln_gamma, m->ln_beta, m->w0, m->b0, m->w1, m->b1, m->w2, m->b2, d16, rows, m->eps, st));
    } else {
        MPF_TRY(mpf_res_ln256_forward(m->x, nullptr, 0, m->ln_gamma, m->ln_beta, nullptr, nullptr, d16, mean, rstd, rows, m->eps, nullptr, 0,
                                      nullptr, st));
        MPF_TRY(mpf_small_gemm_bf16(d16, kE, 1, nullptr, m->w0, kE, 1, m->b0, nullptr, 0, e1, kE, nullptr, rows, kE, kE, 1, st));
        MPF_TRY(mpf_small_gemm_bf16(e1, kE, 1, nullptr, m->w1, kE, 1, m->b1, nullptr, 0, e2, kE, nullptr, rows, kE, kE, 1, st));
        MPF_TRY(mpf_small_gemm_bf16(e2, kE, 1, nullptr, m->w2, kE, 1, m->b2, nullptr, 0, d16, kE, nullptr, rows, kE, kE, 0, st));
    }
    // mask_embed is sequence-first [Q, N, 256]: image stride 256, query stride N * 256
    return mpf_mask_head_bits(d16, kE, (int64_t)m->N * kE, m->pooled, m->mp_rows, m->pad, m->out, m->flags, m->N, m->Q, m->HW, st);
}
