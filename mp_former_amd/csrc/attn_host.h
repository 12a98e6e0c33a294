// Host-side records of the masked attention family ("Attention host layer").  attn.hip holds the kernels, two launchers and the
// ten entry points: each fills one AttnProblem, the only place where the family's sizes, offsets and grids are written, and checks once.
#pragma once
#include "mpf_common.h"

constexpr int kAttnHD = 32;         // head dim
constexpr int kAttnMaxNW = 8;       // waves per workgroup of the forward / dQ kernels

struct AttnProblem {
    int Lq, LqP, Lk, N, H;        // queries, queries padded for the transposed operands (round32), keys, images, heads
    int mask_images;              // N: one mask per image; 1: one for all images; 0: no mask
    static int round32(int x) { return (x + 31) / 32 * 32; }
    static int images(const void* mask, int mask_per_image, int N) { return mask ? (mask_per_image ? N : 1) : 0; }
    int E() const { return H * kAttnHD; }
    int q_tiles() const { return round32(Lq) / 32; }                   // 32 queries per wave of the forward / dQ kernels
    int64_t rows() const { return (int64_t)N * H * Lq; }               // (image, head, query): lse, delta, one partial each
    bool sizes_ok() const { return Lq > 0 && Lk > 0 && N > 0 && H > 0; }
    // workspace = [splits, N, H, Lq, 32] partial O (or dQ), [splits, N, H, Lq, 2] (max, sum), rounded up to 256 bytes | aux, when none is handed in
    size_t part_bytes(int splits) const { return mpf::align256((size_t)splits * N * H * Lq * (kAttnHD + 2) * sizeof(float)); }
    // aux = [N, H, LqP] (lse, delta) pairs, rounded up to 256 bytes | maskT: [mask_images, Lk, LqP] bytes, the mask transposed
    size_t ld2_bytes() const { return mpf::align256((size_t)N * H * LqP * sizeof(float2)); }
    size_t aux_bytes() const { return ld2_bytes() + (size_t)mask_images * Lk * LqP; }
    uint8_t* maskT_at(const void* aux) const { return (uint8_t*)aux + ld2_bytes(); }
    // blocks of the prep launches: 64 x 64 tiles of q / dout and of the mask, 256 delta products, 256 (lse, delta) pairs
    int tiles_q() const { return (LqP + 63) / 64; }
    int tiles_k() const { return (Lk + 63) / 64; }
    int transpose_tiles() const { return tiles_q() * ((N * E() + 63) / 64); }
    int delta_blocks() const { return (Lq * N * E() + 255) / 256; }
    int ld2_blocks() const { return (N * H * Lq + 255) / 256; }
    int mask_blocks() const { return mask_images * tiles_q() * tiles_k(); }
    // profiler records.  Forward: K, V^T, q, out, the mask; each backward kernel: half of the pair's 8 [Lk, N, E] and 8 [Lq, N, E] operands, the mask
    double forward_bytes() const { return 2.0 * ((double)Lk * N * E() * 2 + (double)Lq * N * E()) + (mask_images ? (double)N * Lq * Lk : 0.0); }
    double backward_bytes() const { return forward_bytes() + 2.0 * ((double)Lq * N * E()); }
    double flops(int products) const { return 2.0 * products * Lq * (double)Lk * E() * N; }     // products of Lq x Lk x 32 per head
};

// Element strides of a [L, N, E] operand between sequence positions / images, from the ABI's pair: 0, 0 = dense
struct AttnKV {
    int64_t row, img;
    AttnKV(int64_t row_stride, int64_t img_stride, int N, int E) : row(row_stride ? row_stride : (int64_t)N * E), img(row_stride ? img_stride : E) {}
};

// Key splits of the forward / dQ kernels: one WAVE per (32 queries, head, image, split) and each wave walks its keys in
// 32-key steps of ~2 us, so short waves are what makes these kernels fast: 128 keys per wave (64 for key axes up to 256),
// doubled while that would mean more than ~4 096 waves (measured at config B, Lq = 120: level 1 (Lk = 4 096) 16 + 8 us with
// 128 keys per wave against 24 + 5 with 256, level 2 (Lk = 16 384) 58 + 8 against 49 + 5).  Up to kMaxNW = 8 waves form the
// workgroup of a query tile and merge through LDS — key axes up to 1 024 need no second pass; beyond that the workgroups'
// partials go through the workspace and the combine / sum kernels.
struct AttnSplit {
    int keys_per_wave, nw, wg_splits;
    template <class P> void fill(P& p) const { p.splits = wg_splits; p.nw = nw; p.keys_per_split = keys_per_wave; }
};
namespace mpf {
inline int g_attn_occ = 4;      // mpf_set_option attn_occ (2 | 4): forward, aligned forms
inline int g_attn_nw = kAttnMaxNW, g_attn_kpw = 0;     // A/B switches (mpf_set_option attn_nw / attn_kpw; 0 = the policy above)
inline AttnSplit attn_split(const AttnProblem& p)
{
    AttnSplit a;
    int kpw = g_attn_kpw;
    if (!kpw) {
        const int64_t tiles = (int64_t)p.q_tiles() * p.N * p.H;
        kpw = p.Lk <= 256 ? 64 : 128;
        while (kpw < 512 && tiles * ((p.Lk + kpw - 1) / kpw) > 4096) kpw *= 2;
    }
    const int waves = (p.Lk + kpw - 1) / kpw;
    a.keys_per_wave = kpw;
    a.nw = waves < g_attn_nw ? waves : g_attn_nw;
    a.wg_splits = (waves + a.nw - 1) / a.nw;
    return a;
}

inline bool attn_layout_ok(std::initializer_list<int64_t> strides, std::initializer_list<const void*> buffers)
{   // strides: non-negative multiples of 8 elements; buffers: 16-byte aligned
    int64_t s = 0; uintptr_t b = 0;         // (a negative stride leaves the sign bit set)
    for (int64_t v : strides) s |= v;
    for (const void* p : buffers) b |= (uintptr_t)p;
    return s >= 0 && s % 8 == 0 && (b & 15) == 0;
}
// The check of the forward and backward entries.  The workspace holds the partials and `aux_in_workspace` bytes; aligned16: the backward's buffers
inline int attn_check(const char* who, const AttnProblem& p, std::initializer_list<const void*> required, std::initializer_list<int64_t> strides,
                      std::initializer_list<const void*> kv_buffers, const char* kv_rule, int head_dim, size_t workspace_bytes,
                      size_t aux_in_workspace, std::initializer_list<const void*> aligned16)
{
    if (any_null(required)) return failf(MPF_E_NULL, who, "NULL buffer");
    if (p.LqP != AttnProblem::round32(p.Lq)) return failf(MPF_E_SHAPE, who, "LqP must be Lq rounded up to a multiple of 32");
    if (!attn_layout_ok(strides, kv_buffers)) return failf(MPF_E_SHAPE, who, kv_rule);
    if (head_dim != kAttnHD) return failf(MPF_E_SHAPE, who, "head_dim must be 32");
    if (!p.sizes_ok()) return failf(MPF_E_SHAPE, who, "bad sizes");
    if (workspace_bytes < p.part_bytes(attn_split(p).wg_splits) + aux_in_workspace) return failf(MPF_E_SHAPE, who, "workspace too small");
    return attn_layout_ok({}, aligned16) ? 0 : failf(MPF_E_SHAPE, who, "workspace / aux must be 16-byte aligned");
}
}  // namespace mpf
