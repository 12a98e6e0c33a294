// Host-side record of the fused mask product family.  mask_fused.hip holds the kernels and the seven entry points: each of the four
// launching entries fills one MaskFusedProblem, checks it (mask_fused_check) and launches its kernels with the grids, LDS size and
// workspace parts the record names; the three size queries read the same workspace layouts.  Every size, limit, grid, layout and
// algorithmic-bytes formula of the family is written here, once, in 64-bit arithmetic.  DESIGN.md ("Fused mask product host
// layer") has the table entry x condition -> kernel.
#pragma once
#include <algorithm>

#include "mpf_common.h"

constexpr int kC = 256, kT = 256;             // mask dimension (contraction length of the product); threads of every kernel of the family
constexpr int kMP = 32, kMQ = 128;            // cost: points per tile, queries per workgroup (8 row tiles)
// LDS of the cost kernel: [0, 16K) interpolated features, high planes [32 pt][512 B]; [16K, 32K) low planes; then X [128][33] f32;
// then TV [32 points][2 TCH] f32
constexpr int kOffLo = kMP * 512, kOffX = 2 * kMP * 512, kOffTV = kOffX + kMQ * 33 * 4;
// cost: two workgroups fit a CU (208 VGPRs): ONE full round of 512 (768 workgroups = 1.5 rounds measured 8 % slower); the pair
// backward fills the chip with as many
constexpr int kRound = 512;
constexpr int kMaxT = 128, kMaxKS = 64, kGridYZ = 65535;          // cost: target columns (2 x the widest chunk); d E: partial planes
// pixels per workgroup of the forward and of d F (the backward takes whole tiles only); d E: a pixel chunk is a multiple of kPxStep,
// a workgroup takes kSlotGroup slots
constexpr int kPxTile = 128, kPxStep = 64, kSlotGroup = 128;

enum class MaskFusedEntry { cost, cost_clip, planes_fwd, planes_bwd };

// parts of a workspace: byte offsets (the first part is at 0) and the total; all zero when there is nothing to size
struct CostWs { size_t part_q = 0, tsum = 0, total = 0; };                // part_qt [nwg][G][Q][Tmax][2] | part_q [nwg][G][Q][2] | tsum [rows]
struct PairBwdWs { size_t part = 0, valid = 0, total = 0; };              // Et [N][256][KP] bf16 | part [KS][slots][256] f32 | valid [slots]

struct MaskFusedProblem {
    MaskFusedEntry entry;
    // what only some entries have keeps a value that passes every rule
    int channels = kC, G = 1, Q = 1, Tmax = 1, P = 1, F = 1, h = 1, w = 1, tsamp_rows = 1;          // cost: F frames (1: image form)
    int N = 1, HW = kPxTile, total_slots = 1, max_count = 1, d_embed_dtype = MPF_BF16;            // pair planes
    int64_t embed_row_stride = 0, feat_stride = 0, feat_frame_stride = 0, dfeat_stride = 0;
    bool d_features = false, d_embed = false;                                                     // pair backward: the gradients asked for

    static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }
    bool clip() const { return entry == MaskFusedEntry::cost_clip; }
    bool is_cost() const { return entry == MaskFusedEntry::cost || clip(); }

    // ---- cost: the F * ceil(P / 32) tiles of all frames are dealt to nwg workgroups per (group, 128 queries) in runs of tiles_per_wg
    int64_t samples() const { return (int64_t)F * P; }                             // of a target row
    int64_t cells() const { return (int64_t)G * Q * Tmax; }
    int64_t ntiles() const { return F * ceil_div(P, kMP); }
    int64_t qgroups() const { return ceil_div(Q, kMQ); }
    int64_t tiles_per_wg() const { return ceil_div(ntiles(), std::max<int64_t>(1, kRound / std::max<int64_t>(1, G * qgroups()))); }
    int64_t nwg() const { return ceil_div(ntiles(), tiles_per_wg()); }
    // target-chunk width: two chunks hold Tmax
    int tch() const { for (int t : {4, 8, 12, 16, 24, 32}) if (ceil_div(Tmax, 2) <= t) return t; return 64; }
    size_t cost_lds() const { return kOffTV + (size_t)kMP * 2 * tch() * 4; }        // 50 688 (TCH = 4) .. 66 048 bytes (TCH = 64)
    dim3 rowsum_grid() const { return dim3(tsamp_rows); }
    dim3 cost_grid() const { return dim3((unsigned)nwg(), G, (unsigned)qgroups()); }
    dim3 fold_grid() const { return dim3((unsigned)ceil_div(cells(), kT)); }
    CostWs cost_ws() const
    {
        if (G <= 0 || Q <= 0 || Tmax <= 0 || P <= 0 || F <= 0 || tsamp_rows < 0 || samples() >= (1ll << 31)) return {};
        const size_t rows = (size_t)nwg() * G * Q, a = mpf::align256(rows * Tmax * 2 * 4), b = a + mpf::align256(rows * 2 * 4);
        return {a, b, b + mpf::align256((size_t)tsamp_rows * 4)};
    }

    // ---- pair backward: Et rows padded to KP slots, mgroups groups of 128 slots, KS pixel chunks of px_per_chunk
    int64_t KP() const { return std::max<int64_t>(64, ceil_div(max_count, 64) * 64); }
    int64_t mgroups() const { return std::max<int64_t>(1, ceil_div(max_count, kSlotGroup)); }
    // pixel chunks: enough workgroups to fill the chip, at most 64 partial planes; a chunk is a multiple of 64 pixels
    int64_t want_chunks() const { return std::max<int64_t>(1, std::min<int64_t>(kMaxKS, kRound / std::max<int64_t>(1, N * mgroups()))); }
    int KS() const { int ks = (int)want_chunks(); while (ks > 1 && (HW % (ks * kPxStep))) --ks; return ks; }
    int px_per_chunk() const { return HW / KS(); }
    dim3 fwd_grid() const { return dim3((unsigned)ceil_div(HW, kPxTile), N); }
    dim3 transpose_grid() const { return dim3((unsigned)(KP() / 32), N); }
    dim3 dfeat_grid() const { return dim3(HW / kPxTile, N); }
    dim3 valid_grid() const { return dim3((unsigned)ceil_div(total_slots, kT)); }
    dim3 dembed_grid() const { return dim3(KS(), (unsigned)mgroups(), N); }
    dim3 reduce_grid() const { return dim3(total_slots); }
    PairBwdWs pair_bwd_ws() const
    {
        if (N <= 0 || HW <= 0 || total_slots <= 0 || max_count <= 0) return {};
        const size_t a = mpf::align256((size_t)N * kC * KP() * 2), b = a + mpf::align256((size_t)KS() * total_slots * kC * 4);
        return {a, b, b + mpf::align256((size_t)total_slots * 4)};
    }

    size_t workspace_bytes() const { return is_cost() ? cost_ws().total : entry == MaskFusedEntry::planes_bwd ? pair_bwd_ws().total : 0; }

    // algorithmic bytes and flops handed to the profiler.  cost: the gathers, 4 corner rows of 512 B per point, and the two-plane product
    double cost_bytes() const { return (double)G * qgroups() * F * P * 2048.0 + (double)tsamp_rows * F * P * 4.0; }
    double cost_flops() const { return 2.0 * 2.0 * (double)G * Q * F * P * kC; }
    double fwd_bytes() const { return 2.0 * (double)N * HW * kC; }
    double dfeat_bytes() const { return 2.0 * (double)N * HW * kC + 2.0 * (double)total_slots * HW; }
    double dembed_bytes() const { return 2.0 * (double)N * HW * kC * mgroups() + 2.0 * (double)total_slots * HW; }
    double bwd_flops() const { return 2.0 * (double)total_slots * HW * kC; }
};

// `who` is the entry's symbol; the texts name it without the "mpf_".  Order: NULL buffers, channels, sizes, the limits of the entry
// (128 targets, 65 535 on grid.y / grid.z, the 2^31 products), alignment of strides and pixel counts, overlapping frames, gradient
// dtype, NULL or short workspace.  The pair entries answer their limits and alignment as sizes, with one text.
inline int mask_fused_check(const char* who, const MaskFusedProblem& p, std::initializer_list<const void*> bufs, const void* workspace = nullptr,
                            size_t workspace_bytes = 0)
{
    const auto fail = [&](int code, const char* what) { return mpf::failf(code, who + 4, what); };
    const char* sizes = p.entry == MaskFusedEntry::planes_bwd ? "bad sizes (HW must be a multiple of 128)" : "bad sizes";
    if (mpf::any_null(bufs)) return fail(MPF_E_NULL, "NULL buffer");
    if (p.channels != kC) return fail(MPF_E_SHAPE, "256 channels only");
    if (std::min({p.G, p.Q, p.Tmax, p.P, p.F, p.h, p.w, p.tsamp_rows, p.N, p.HW, p.total_slots, p.max_count}) <= 0 || p.N > kGridYZ)
        return fail(MPF_E_SHAPE, sizes);
    if (p.Tmax > kMaxT) return fail(MPF_E_SHAPE, p.clip() ? "at most 128 tubes per clip" : "at most 128 targets per image");
    if (p.G > kGridYZ || p.F > kGridYZ || std::max(p.cells(), p.samples()) >= (1ll << 31))
        return fail(MPF_E_TOO_LARGE, p.clip() ? "too many groups, frames or samples" : "too many groups");
    if ((p.embed_row_stride % 8) || (p.feat_stride % 8) || (p.feat_frame_stride % 8) || (p.dfeat_stride % 8)
        || p.HW % (p.entry == MaskFusedEntry::planes_fwd ? 4 : kPxTile))
        return fail(MPF_E_SHAPE, p.is_cost() ? "rows must be 16-byte aligned" : sizes);
    // (stride < h * w * 256, as a quotient: the product of two INT_MAX and 256 is past 64 bits)
    if (p.clip() && p.feat_frame_stride / kC < (int64_t)p.h * p.w) return fail(MPF_E_SHAPE, "frames overlap");
    if (p.d_embed && p.d_embed_dtype != MPF_BF16 && p.d_embed_dtype != MPF_F32) return fail(MPF_E_DTYPE, "d_embed bf16 or f32");
    if (p.entry == MaskFusedEntry::planes_fwd) return 0;
    if (!workspace) return fail(MPF_E_NULL, "NULL buffer");
    return workspace_bytes < p.workspace_bytes() ? fail(MPF_E_SHAPE, "workspace too small") : 0;
}
