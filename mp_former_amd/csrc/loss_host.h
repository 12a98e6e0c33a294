// Host-side record of the point-sampled loss family.  loss.hip holds the kernels and the ten entry points: each entry fills one
// LossProblem, checks it (loss_check), asks for a route (mask_loss_fwd_route / match_cost_route / sample_select_pt) and launches
// the kernel of that route, the ones with dynamic LDS through launch_lds.  Every size, limit, grid and algorithmic-bytes formula of
// the family is written here, once.  DESIGN.md ("Loss host layer") has the table entry x condition -> kernel.
#pragma once
#include <hip/hip_bf16.h>

#include "mpf_common.h"

// workgroup shapes the kernels of loss.hip are written for
constexpr int kThreads = 256;             // the per-point kernels
constexpr int kSelThreads = 1024;         // select_uncertain_kernel
constexpr int kMcThreads = 1024;          // mask_loss_fwd_lds_kernel, sample_select_kernel: one workgroup per staged plane
constexpr int kBandThreads = 1024;        // mask_loss_bwd_band_kernel
// match_cost_lds_kernel: 512 threads x 25 points keep the samples of 2 rows in registers without spilling (1024 threads leave 128
// VGPRs per lane: 180 spilled registers and 2.6x the time; 4 rows would need ~300 registers per lane); it reduces
// 2 * rows * 4 + 4 sums per pass of 4 targets
constexpr int kCostThreads = 512, kCostPT = 25, kCostRows = 2, kCostSums = 2 * kCostRows * 4 + 4;

// LDS of a workgroup: 160 KiB.  A bf16 plane is staged whole when its size is a multiple of 16 bytes (copy_plane_to_lds moves uint4) and at most
constexpr int64_t kPlaneLds = 128 * 1024;         // sample_select_kernel adds up to 6 176 bytes of histogram and counts (40 keys per thread),
                                                  // mask_loss_fwd_lds_kernel 256 of sums; the clip cost was written and tested to this limit only;
                                                  // also the band of accumulators of the dense backward
constexpr int64_t kPlaneLdsCost = 136 * 1024;     // image cost: match_cost_lds_kernel adds 640 bytes of sums only
constexpr size_t kXsLds = 150 * 1024;             // match_cost_kernel keeps the P logits of a row (of one frame) in LDS: 38 400 points
constexpr size_t kDefaultLds = 32 * 1024;         // match_cost_kernel asks for a higher dynamic-LDS limit only above this
constexpr int kGridY = 65535;

// floats per (row, frame) of the clip cost's workspace: {softplus, sigmoid, then (x t, s t, t) per target}
// (the kernels take it of an int, the host sizes of an int64_t)
template <class I>
__host__ __device__ __forceinline__ I clip_partial_floats(I Tmax) { return 2 + 3 * Tmax; }

enum class LossEntry { point_sample, forward, backward, backward_dense, select, sample_select, cost, cost_clip };
enum class LossRoute { generic, lds };

struct LossProblem {
    LossEntry entry;
    int dtype = MPF_BF16, h = 1, w = 1;       // the maps that are sampled
    int n = 0, P = 1;                         // rows (pairs, cost rows) and points per row (clip: per frame)
    // what only some entries have keeps a value that passes every rule
    int H = 1, W = 1, gt_dtype = MPF_U8;      // ground-truth planes
    int grad_dtype = MPF_BF16, chunks = 1;    // dense backward; forward
    int M = 1, k = 1, P_out = 1;              // selection: candidates, kept, row pitch of the output
    int F = 0, Tmax = 1, G = 1;               // cost: frames (0: image form), target columns, rows per group
    int64_t stride_f = 0;

    LossProblem(LossEntry e, int dtype_, int h_, int w_, int n_, int P_ = 1) : entry(e), dtype(dtype_), h(h_), w(w_), n(n_), P(P_) {}
    static int ceil_div(int a, int b) { return (int)(((int64_t)a + b - 1) / b); }
    bool bits() const { return gt_dtype == MPF_BITS; }
    bool empty() const { return n == 0 || k == 0; }
    const char* pick(const char* f32, const char* bf16) const { return dtype == MPF_F32 ? f32 : bf16; }

    // LDS staging of a bf16 plane
    int64_t plane_bytes() const { return (int64_t)h * w * 2; }
    bool fits_lds(int64_t limit) const { return plane_bytes() % 16 == 0 && plane_bytes() <= limit; }
    size_t fwd_lds() const { return (size_t)plane_bytes() + (kMcThreads / 64) * 4 * sizeof(float); }
    size_t cost_lds() const { return (size_t)plane_bytes() + (kCostThreads / 64) * kCostSums * sizeof(float); }
    size_t select_lds(int PT) const { return (size_t)plane_bytes() + (256 + 2 * PT * 16 + 8) * sizeof(int); }
    size_t xs_bytes() const { return (size_t)P * 4; }

    // dense backward: horizontal bands of at most kPlaneLds of 32-bit accumulators, of equal height
    int max_rows() const { return (int)(kPlaneLds / (4 * (int64_t)w)); }
    int nb() const { return ceil_div(h, max_rows()); }
    int band_rows() const { return ceil_div(h, nb()); }
    size_t band_lds() const { return (size_t)band_rows() * w * 4; }

    dim3 sample_grid() const { return dim3(ceil_div(P, kThreads), n); }
    dim3 fwd_grid() const { return dim3(chunks, n); }
    dim3 bwd_grid() const { return dim3(ceil_div(P, kThreads * 4), n); }
    dim3 band_grid() const { return dim3(nb(), n); }
    dim3 cost_grid() const { return F ? dim3(n, F) : dim3(n); }
    // LDS cost: the image form takes kCostRows rows per workgroup; the clip form cuts every run of G rows into ceil(G / kCostRows)
    dim3 cost_lds_grid() const { return F ? dim3((n / G) * ceil_div(G, kCostRows), F) : dim3(n / kCostRows); }
    int64_t cells() const { return (int64_t)n * Tmax; }
    dim3 fold_grid() const { return dim3((unsigned)((cells() + kThreads - 1) / kThreads)); }      // (cells() <= kThreads * INT_MAX: loss_check)
    size_t workspace_bytes() const { return n <= 0 || F <= 0 || Tmax <= 0 ? 0 : (size_t)n * F * clip_partial_floats((int64_t)Tmax) * sizeof(float); }

    // algorithmic bytes handed to the profiler
    double bytes(LossRoute r = LossRoute::generic) const
    {
        const bool lds = r == LossRoute::lds;
        switch (entry) {
        case LossEntry::point_sample: return (double)n * P * (8.0 + 4.0 + 16.0);
        case LossEntry::forward: return lds ? (double)n * ((double)h * w * 2.0 + P * (8.0 + 4.0)) : (double)n * P * (8.0 + 16.0 + 4.0);
        case LossEntry::backward: return (double)n * P * (8.0 + 16.0 + 4.0 + 32.0);
        case LossEntry::backward_dense: return (double)n * P * (8.0 + 16.0 + 4.0) + (double)n * h * w * 2.0;
        case LossEntry::select: return (double)n * M * 12.0 * 2 + (double)n * k * 8.0;
        case LossEntry::sample_select: return (double)n * ((double)plane_bytes() + M * 8.0 + k * 16.0);
        case LossEntry::cost:
            return lds ? (double)n * ((double)h * w * 2.0 + P * 8.0 / 4 + P * 4.0 * Tmax / 4) : (double)n * P * (8.0 + 16.0 + 4.0 * Tmax);
        case LossEntry::cost_clip: return (double)n * F * ((double)h * w * 2.0 + P * 8.0 / 2 + P * 4.0 * Tmax / 2);
        }
        return 0.0;
    }
};

// `who` is the entry's symbol; most texts name it without the "mpf_".  `sampler`: the buffers every entry built on the point sampler
// has (answered for as "point-sample", sizes included), or all buffers of the other entries; `own`: the rest.  Order: NULL, sizes,
// overlapping frames, dtypes (gradient, ground truth, maps), the limits of the entry, workspace.  "Nothing to do" (p.empty()) is the
// caller's next line: a call that is both empty and at fault is at fault.
inline int loss_check(const char* who, const LossProblem& p, std::initializer_list<const void*> sampler,
                      std::initializer_list<const void*> own = {}, const void* workspace = nullptr, size_t workspace_bytes = 0)
{
    using E = LossEntry;
    const E e = p.entry;
    const char* name = who + 4;
    const auto fail = [&](int code, const char* what) { return mpf::failf(code, name, what); };
    const bool pairs = e == E::point_sample || e == E::forward || e == E::backward || e == E::backward_dense;
    const bool map_sizes_bad = p.n < 0 || p.P <= 0 || p.h <= 0 || p.w <= 0, pred = p.dtype == MPF_F32 || p.dtype == MPF_BF16;
    if (mpf::any_null(sampler)) return mpf::failf(MPF_E_NULL, pairs ? "point-sample" : name, "NULL buffer");
    if (pairs && map_sizes_bad) return mpf::failf(MPF_E_SHAPE, "point-sample", "bad sizes");
    if (mpf::any_null(own)) return fail(MPF_E_NULL, "NULL buffer");
    if (map_sizes_bad || p.chunks <= 0 || p.Tmax <= 0 || p.M <= 0 || p.k < 0 || p.k > p.M || p.P_out < p.k || (e == E::cost_clip && (p.F <= 0 || p.G <= 0))
        || (e != E::backward_dense && (p.H <= 0 || p.W <= 0)))          // (the dense backward has never looked at H and W)
        return fail(MPF_E_SHAPE, "bad sizes");
    if (p.F > 1 && p.stride_f < (int64_t)p.h * p.w) return fail(MPF_E_SHAPE, "the frames of a row overlap (stride_f < h * w)");
    if (e == E::backward_dense && p.grad_dtype != p.dtype) return fail(MPF_E_DTYPE, "gradient dtype must equal the map dtype");
    if (p.gt_dtype != MPF_U8 && !p.bits()) return fail(MPF_E_DTYPE, "gt dtype must be MPF_U8 or MPF_BITS");
    if (p.bits() && ((int64_t)p.H * p.W) % 32 != 0) return fail(MPF_E_SHAPE, "bit-packed masks need H*W % 32 == 0");
    if (e == E::point_sample && !pred && p.dtype != MPF_U8 && p.dtype != MPF_BITS)
        return mpf::failf(MPF_E_DTYPE, who, "dtype must be MPF_F32, MPF_BF16, MPF_U8 or MPF_BITS");
    if (e == E::sample_select && p.dtype != MPF_BF16) return fail(MPF_E_DTYPE, "bf16 maps only (use mpf_point_sample + mpf_select_uncertain)");
    if (e != E::point_sample && e != E::select && !pred) return mpf::failf(MPF_E_DTYPE, who, "pred dtype must be MPF_F32 or MPF_BF16");
    if (e == E::backward_dense && p.max_rows() < 2) return fail(MPF_E_TOO_LARGE, "plane rows wider than 16384");
    if ((e == E::cost || e == E::cost_clip) && p.xs_bytes() > kXsLds)
        return fail(MPF_E_TOO_LARGE, p.F ? "more than 38400 points per frame" : "more than 38400 points per row");
    if (p.F > kGridY) return fail(MPF_E_TOO_LARGE, "more than 65535 frames (grid.y)");
    if (e == E::cost_clip && p.cells() > (int64_t)kThreads * 0x7fffffff) return fail(MPF_E_TOO_LARGE, "cost matrix too large");
    if (pairs && p.n > kGridY) return mpf::fail(MPF_E_TOO_LARGE, "loss kernels: more than 65535 rows in one launch (grid.y)");
    if (e == E::sample_select && (!p.fits_lds(kPlaneLds) || p.M > 40 * kMcThreads))
        return fail(MPF_E_TOO_LARGE, "plane larger than 128 KiB or more than 40960 candidates");
    if (p.workspace_bytes() && !workspace) return fail(MPF_E_NULL, "NULL workspace");
    return workspace_bytes < p.workspace_bytes() ? fail(MPF_E_SHAPE, "workspace too small (mpf_match_cost_clip_workspace_bytes)") : 0;
}

// ---- routes: pure functions of the record ------------------------------------------------------------------------------------------
// mask_loss_fwd_lds_kernel: one workgroup per pair writes all `chunks` slots of its row, one thread per float
inline LossRoute mask_loss_fwd_route(const LossProblem& p)
{
    return p.dtype == MPF_BF16 && p.fits_lds(kPlaneLds) && p.chunks <= kMcThreads / 4 ? LossRoute::lds : LossRoute::generic;
}

// match_cost_lds_kernel, image (F == 0) and clip: G consecutive rows share their point set and targets.  The image form walks the
// rows in pairs, so groups and the row count must be even; the clip form gives the tail of a run a workgroup of its own, so any
// G >= 2 that divides the rows will do
inline LossRoute match_cost_route(const LossProblem& p)
{
    if (p.dtype != MPF_BF16 || p.P > kCostPT * kCostThreads || p.G < 2) return LossRoute::generic;
    const bool rows_ok = p.F ? p.n % p.G == 0 : (p.G % kCostRows == 0 && p.n % kCostRows == 0);
    return rows_ok && p.fits_lds(p.F ? kPlaneLds : kPlaneLdsCost) ? LossRoute::lds : LossRoute::generic;
}

// keys per thread of sample_select_kernel: 37 covers the shipped 3 x 12544 candidates without register spills; 40 is the cap
inline int sample_select_pt(int M) { return M <= 16 * kMcThreads ? 16 : (M <= 37 * kMcThreads ? 37 : 40); }

// ---- launch ------------------------------------------------------------------------------------------------------------------------
template <class T>
struct MapType { using type = T; };
// f(MapType<T>{}) for the element type of the maps; kU8: byte maps too (mpf_point_sample)
template <bool kU8 = false, class F>
void with_map_type(int dtype, F&& f)
{
    if (dtype == MPF_F32) f(MapType<float>{});
    else if (dtype == MPF_BF16 || !kU8) f(MapType<__hip_bfloat16>{});
    else if constexpr (kU8) f(MapType<uint8_t>{});
}

// Launch of kernel K with `lds` bytes of dynamic LDS.  The limit of K is raised through mpf::ensure_dynamic_lds, i.e. once per
// device and high-water size (one LdsAttr per instantiation of this template = per kernel), when lds is above kRaiseAbove.
template <auto K, size_t kRaiseAbove = 0, class... A>
int launch_lds(dim3 grid, int threads, size_t lds, hipStream_t st, A... args)
{
    static mpf::LdsAttr attr;
    if (lds > kRaiseAbove)
        if (int e = mpf::ensure_dynamic_lds((const void*)K, lds, attr)) return e;
    hipLaunchKernelGGL(K, grid, dim3(threads), lds, st, args...);
    return 0;
}
