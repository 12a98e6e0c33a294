// Host-side records of the small-row GEMM family.  small_gemm.hip holds the kernels and the five entry points: each fills one record,
// checks it and launches with the geometry the record names.  Every rule, tile count, grid and algorithmic-bytes formula of the family
// is written here, once, in 64-bit arithmetic; nothing here touches a device.  DESIGN.md ("Small-row GEMM host layer") has the table
// entry x condition -> kernel.
#pragma once
#include <stdint.h>

#include "mpf_common.h"

constexpr int kSgGroupMax = 8, kSgTrMax = 16;                // problems per grouped launch, matrices per transpose launch
constexpr int kSgFillBlocks = 256;                           // a launch of this many blocks fills the chip
constexpr int64_t kSgGridX = 0x7fffffff, kSgGridY = 65535;   // what a launch takes on x and on y

inline int64_t sg_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the widest tile (16 rows x 16 nj columns) that still gives the chip kSgFillBlocks blocks, else the narrowest
inline int small_gemm_tile_width(int64_t n_it, int64_t J)
{
    for (int nj : {4, 2})
        if (n_it * sg_ceil_div(J, 16 * nj) >= kSgFillBlocks) return nj;
    return 1;
}

// one call of mpf_small_gemm_bf16_blocked (an aggregate: the entries fill it in the order of the fields)
struct SmallGemmProblem {
    const void *a = nullptr, *gate = nullptr, *b = nullptr, *bias = nullptr, *c_in = nullptr;
    void *c = nullptr, *rowsum_a = nullptr;
    int64_t a_rs = 0, a_ks = 0, a_bs = 0, b_rs = 0, b_ks = 0, ldcin = 0, ldc = 0, c_bs = 0;
    int a_blk = 0, c_blk = 0, I = 0, J = 0, Kc = 0, relu = 0;

    // an item of the grouped launch: no bias, addend, column blocks or ReLU
    static SmallGemmProblem of(const MpfSmallGemmItem& m)
    {
        return {m.a, m.gate, m.b, nullptr, nullptr, m.c, m.rowsum_a, m.a_rs, m.a_ks, m.a_bs, m.b_rs, m.b_ks, 0, m.ldc, 0, m.a_blk, 0, m.I, m.J, m.Kc, 0};
    }
    bool ac() const { return a_ks == 1; }                 // contraction-contiguous operands
    bool bc() const { return b_ks == 1; }
    bool gated() const { return gate != nullptr; }
    bool masked() const { return (Kc & 31) != 0; }        // the last 32-wide contraction step is partial
    bool empty() const { return I == 0 || J == 0; }
    int64_t n_it() const { return sg_ceil_div(I, 16); }
    int nj() const { return small_gemm_tile_width(n_it(), J); }
    int64_t tiles_j() const { return sg_ceil_div(J, 16 * nj()); }
    int64_t n_waves() const { return n_it() * tiles_j(); }          // blocks of the launch
    double bytes() const { return 2.0 * ((double)I * Kc * (gate ? 2 : 1) + (double)J * Kc + (double)I * J); }
};

inline bool sg_misaligned(const void* p, uintptr_t mask) { return ((uintptr_t)p & mask) != 0; }

// Order: blocked-form rule, negative size, empty (accepted: nothing to check), NULL, empty contraction, unit stride, 16-byte rule,
// 8-byte-store rule, launch size.
inline int small_gemm_check(const SmallGemmProblem& p)
{
    if (p.a_blk < 0 || p.c_blk < 0 || (p.a_blk && p.a_blk % 32) || (p.c_blk && p.c_blk % 64) || (p.a_blk && p.ac() && p.Kc % 32) ||
        (p.c_blk && p.c_in))
        return mpf::fail(MPF_E_SHAPE, "small_gemm_blocked: a_blk % 32, c_blk % 64 (and Kc % 32 for a blocked contraction) must be 0");
    if (p.I < 0 || p.J < 0 || p.Kc < 0) return mpf::fail(MPF_E_SHAPE, "small_gemm: negative size");
    if (p.empty()) return 0;
    if (!p.a || !p.b || !p.c) return mpf::fail(MPF_E_NULL, "small_gemm: a, b, c must not be null");
    if (p.Kc == 0) return mpf::fail(MPF_E_SHAPE, "small_gemm: empty contraction");
    if ((!p.ac() && p.a_rs != 1) || (!p.bc() && p.b_rs != 1))
        return mpf::fail(MPF_E_SHAPE, "small_gemm: each operand needs a unit row or contraction stride");
    if ((p.ac() && (p.Kc % 8 || p.a_rs % 8 || sg_misaligned(p.a, 15) || (p.gate && sg_misaligned(p.gate, 15)))) ||
        (p.bc() && (p.Kc % 8 || p.b_rs % 8 || sg_misaligned(p.b, 15))))
        return mpf::fail(MPF_E_SHAPE, "small_gemm: contraction-contiguous operands need 16-B aligned rows, Kc % 8 == 0");
    if (p.J % 4 || p.ldc % 4 || sg_misaligned(p.c, 7) || (p.bias && sg_misaligned(p.bias, 7)) ||
        (p.c_in && (p.ldcin % 4 || sg_misaligned(p.c_in, 7))))
        return mpf::fail(MPF_E_SHAPE, "small_gemm: J and ldc must be multiples of 4 (8-B stores)");
    if (p.n_waves() > kSgGridX) return mpf::fail(MPF_E_TOO_LARGE, "small_gemm: more than 2^31 - 1 tiles");
    return 0;
}

// The problems of one grouped launch: the non-empty items in order, block ranges [first[t], first[t + 1]), first[n] = the grid.
// n == 0: nothing to launch.  The unused slots repeat problem 0 with an empty block range.
struct SmallGemmGroupPlan {
    SmallGemmProblem it[kSgGroupMax];
    int64_t first[kSgGroupMax + 1] = {};
    int nj[kSgGroupMax] = {};
    int n = 0;
    bool masked = false, contig = false;      // the group's contraction tail; both operands of every item contraction-contiguous
    double bytes = 0.0;
};

// Order: count, zero items (accepted), NULL items; per item its operand form, one form per group, no gate on contiguous operands, the
// item's own check, Kc % 32 in agreement with the non-empty items before it; then the launch size.
inline int small_gemm_group_plan(SmallGemmGroupPlan& g, const MpfSmallGemmItem* items, int n_items)
{
    if (n_items < 0 || n_items > kSgGroupMax) return mpf::fail(MPF_E_SHAPE, "small_gemm_group: at most 8 problems per launch");
    if (n_items == 0) return 0;
    if (!items) return mpf::fail(MPF_E_NULL, "small_gemm_group: NULL items");
    for (int t = 0; t < n_items; ++t) {
        const SmallGemmProblem p = SmallGemmProblem::of(items[t]);
        const bool contig = p.ac() && p.bc();
        if (!contig && (p.a_rs != 1 || p.b_rs != 1))
            return mpf::fail(MPF_E_SHAPE, "small_gemm_group: both operands row-contiguous (the weight-gradient form) or both contraction-contiguous");
        if (t > 0 && contig != g.contig) return mpf::fail(MPF_E_SHAPE, "small_gemm_group: one operand form per group");
        g.contig = contig;
        if (contig && p.gate) return mpf::fail(MPF_E_SHAPE, "small_gemm_group: the gate belongs into the transposed copy (mpf_transpose_group_bf16)");
        if (int e = small_gemm_check(p)) return e;
        if (p.empty()) continue;
        if (g.n > 0 && p.masked() != g.masked) return mpf::fail(MPF_E_SHAPE, "small_gemm_group: Kc % 32 must agree across the group");
        g.masked = p.masked();
        g.it[g.n] = p;
        g.nj[g.n] = p.nj();
        g.first[g.n + 1] = g.first[g.n] + p.n_waves();
        g.bytes += p.bytes();
        ++g.n;
    }
    if (g.first[g.n] > kSgGridX) return mpf::fail(MPF_E_TOO_LARGE, "small_gemm_group: more than 2^31 - 1 tiles");
    for (int t = g.n; t < kSgGroupMax && g.n > 0; ++t) { g.first[t + 1] = g.first[g.n]; g.nj[t] = 1; g.it[t] = g.it[0]; }
    return 0;
}

// The matrices of one transpose launch: 64 x 64 tiles, tiles_r of them along the Rp padded rows; matrix t owns the blocks
// [first[t], first[t + 1]), first[n] = the grid.  n == 0: nothing to launch.
struct TransposeGroupPlan {
    int64_t first[kSgTrMax + 1] = {};
    int64_t tiles_r = 0;
    int n = 0;
    int64_t blocks() const { return first[n]; }
};

// Order: count, zero items (accepted), NULL items, Rp; per item NULL matrices, then its shape and alignment; then the launch size.
inline int transpose_group_plan(TransposeGroupPlan& g, const MpfTransposeItem* items, int n_items, int Rp)
{
    if (n_items < 0 || n_items > kSgTrMax) return mpf::fail(MPF_E_SHAPE, "transpose_group: at most 16 matrices per launch");
    if (n_items == 0) return 0;
    if (!items) return mpf::fail(MPF_E_NULL, "transpose_group: NULL items");
    if (Rp <= 0 || Rp % 8) return mpf::fail(MPF_E_SHAPE, "transpose_group: Rp must be a positive multiple of 8");
    g.tiles_r = sg_ceil_div(Rp, 64);
    for (int t = 0; t < n_items; ++t) {
        const MpfTransposeItem& m = items[t];
        if (!m.src || !m.dst) return mpf::fail(MPF_E_NULL, "transpose_group: NULL matrix");
        if (m.R <= 0 || m.R > Rp || m.C <= 0 || m.C % 8 || m.ld % 8 || sg_misaligned(m.src, 15) || sg_misaligned(m.dst, 15) ||
            (m.gate && sg_misaligned(m.gate, 15)))
            return mpf::fail(MPF_E_SHAPE, "transpose_group: 0 < R <= Rp, C % 8 == 0, 16-byte aligned rows");
        g.first[t + 1] = g.first[t] + g.tiles_r * sg_ceil_div(m.C, 64);
    }
    if (g.first[n_items] > kSgGridX) return mpf::fail(MPF_E_TOO_LARGE, "transpose_group: more than 2^31 - 1 tiles");
    g.n = n_items;
    return 0;
}

// How one call of mpf_tall_gemm_bf16 is launched.  ws: the weight-stationary kernel tall_ws_bf16_kernel<KS, NB, MB, NBUF> on a grid of
// gx column groups x gy workgroups that walk the ntiles row tiles; else the fragment-per-wave kernel on 128 x 128 tiles.
struct TallRoute {
    bool ws = false;
    int KS = 0, NB = 0, MB = 0, NBUF = 0;
    int64_t ntiles = 0, gx = 0, gy = 0;
    size_t lds = 0;
    // the y dimension can exceed what a launch takes under a tall_ws_wgs override
    int check() const { return gy > kSgGridY ? mpf::fail(MPF_E_TOO_LARGE, "tall_gemm_bf16: more than 65 535 workgroups on grid.y (tall_ws_wgs)") : 0; }
};

struct TallGemmProblem {
    const void *a = nullptr, *b = nullptr, *bias = nullptr;
    void* c = nullptr;
    int64_t lda = 0, ldb = 0, ldc = 0;
    int M = 0, N = 0, K = 0;

    bool empty() const { return M == 0 || N == 0; }       // asked before the check: an empty call returns 0 whatever else it holds
    bool weight_stationary(bool tall_ws) const { return tall_ws && M >= 1024 && (K == 256 || K == 768); }
    // cus: compute units of the device; wgs: the tall_ws_wgs override (0: one residency; read as unsigned).  Both only matter to
    // the weight-stationary route.
    TallRoute route(bool tall_ws, int cus, int wgs) const
    {
        TallRoute r;
        r.ws = weight_stationary(tall_ws);
        if (!r.ws) {
            r.gx = sg_ceil_div(N, 128);
            r.ntiles = r.gy = sg_ceil_div(M, 128);
            return r;
        }
        // (measured at 32 768 rows: 64-row tiles x 2 buffers, 32-row tiles x 3 or 4 buffers all give 29-30 us for K = 256 and
        // 35-38 us for K = 768: the copies are not what the kernel waits for — ablations: result stores 9 us of HBM write time,
        // copies 3-8, MFMA phase 3 (K = 256) / 15 (K = 768: one 16-column block per wave reads the whole X tile from LDS))
        r.KS = K / 32; r.NB = K == 256 ? 2 : 1; r.MB = K == 256 ? 4 : 2; r.NBUF = 2;
        r.ntiles = sg_ceil_div(M, r.MB * 16);
        r.gx = sg_ceil_div(N, 64 * r.NB);
        r.lds = (size_t)r.MB * 16 * r.KS * 64 * r.NBUF;
        // the grid is exactly one residency (LDS: 160 KB per CU; registers: two workgroups), so that no workgroup starts after the
        // others have walked their tiles
        const int64_t per_cu = r.lds > 80 * 1024 ? 1 : 2;
        const int64_t gy = (wgs ? (int64_t)(unsigned)wgs : cus * per_cu) / r.gx;
        r.gy = gy < 1 ? 1 : (gy > r.ntiles ? r.ntiles : gy);
        return r;
    }
    double bytes() const { return 2.0 * ((double)M * K + (double)N * K + (double)M * N); }
    double flops() const { return 2.0 * M * (double)N * K; }
};

// Order: NULL buffers, sizes, alignment, row tiles.  (The row-tile rule counts 128-row tiles for both routes.)
inline int tall_gemm_check(const TallGemmProblem& p)
{
    if (!p.a || !p.b || !p.c) return mpf::fail(MPF_E_NULL, "tall_gemm_bf16: NULL buffer");
    if (p.M < 0 || p.N < 0 || p.K <= 0 || (p.K & 31)) return mpf::fail(MPF_E_SHAPE, "tall_gemm_bf16: K must be a positive multiple of 32");
    if ((p.lda & 7) || (p.ldb & 7) || (p.ldc & 3) || sg_misaligned(p.a, 15) || sg_misaligned(p.b, 15) || sg_misaligned(p.c, 7))
        return mpf::fail(MPF_E_SHAPE, "tall_gemm_bf16: 16-byte aligned operand rows, 8-byte aligned result rows");
    if (sg_ceil_div(p.M, 128) > kSgGridY) return mpf::fail(MPF_E_TOO_LARGE, "tall_gemm_bf16: more than 65 535 row tiles");
    return 0;
}
