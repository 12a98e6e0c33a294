// Host-side records of the multi-scale deformable attention (MSDA) family.  msda_entry.hip holds the ten op entry points: each
// fills one MsdaProblem and one MsdaOperands, checks them (msda_check), asks for a route (msda_forward_route /
// msda_backward_route) and calls the launcher of that route in msda.hip, msda_block.hip or msda_bwd_binned.hip.
#pragma once
#include "mpf_common.h"

struct MsdaProblem {
    int N, S, M, D, L, Lq, P, dtype;      // batch, spatial_size, num_heads, channels, num_levels, num_query, num_point, MPF_F32 / MPF_F64
    size_t esz() const { return dtype == MPF_F32 ? 4 : 8; }
    int64_t n_value() const { return (int64_t)N * S * M * D; }             // elements of value / grad_value
    int64_t n_samples() const { return (int64_t)N * Lq * M * L * P; }      // sampling points: attn has one word each, loc two
    int64_t n_rows() const { return (int64_t)N * Lq * M * D; }             // elements of output / grad_output
    // algorithmic bytes.  Forward: value + loc + attn read once, out written once; the fused raw form
    // also WRITES loc / attn for the backward (the traffic of the prep launch it replaces).
    double forward_bytes(bool rw = false) const { return (double)esz() * ((double)n_value() + (double)n_samples() * 3 * (rw ? 2 : 1) + (double)n_rows()); }
    // backward: value, loc, attn, grad_out read once; the three gradients written once
    double backward_bytes() const { return (double)esz() * (2.0 * n_value() + 2.0 * n_samples() * 3 + (double)n_rows()); }
    // the blocked backward's pair (1344 e S N) is split as: bin = loc in; tile = the rest
    double bin_bytes() const { return 4.0 * n_samples() * 2; }
    double tile_bytes() const { return 4.0 * ((double)n_value() * 2 + (double)n_rows() + (double)n_samples() * 4); }
};

// Every pointer an entry point can be given; the ones an entry does not have stay NULL.
struct MsdaOperands {
    const void* value = nullptr;
    const int64_t *shapes = nullptr, *lsi = nullptr;       // device: [L][2] (H, W) and [L] level starts
    const int64_t* host_shapes = nullptr;                  // host copy of `shapes`, levels stored back to back (optional)
    const void *loc = nullptr, *attn = nullptr;            // inputs; the raw forward WRITES them
    const void *raw = nullptr, *ref = nullptr;             // raw forward: projection output and reference points
    void* out = nullptr;                                   // forward result
    const void* grad_out = nullptr;
    void *grad_value = nullptr, *grad_loc = nullptr, *grad_attn = nullptr, *grad_raw = nullptr;
    const void* fwd_out = nullptr;                         // raw backward: the forward result
    float *graw_amax = nullptr, *gv_amax = nullptr;        // amax slots of grad_raw / grad_value (optional)
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
    hipStream_t stream = nullptr;
};

enum class MsdaFamily { blocked, blocked_raw, blocked_dev, tiled, generic, binned };

struct MsdaRoute {
    MsdaFamily family;
    int V = 0;                    // tiled: channels per lane of msda_*_tiled_f32<32, V>
    bool prep = false;            // msda_prep_kernel runs first (raw forward)
    bool records_amax = false;    // the kernels fill the amax slots themselves; otherwise the entry runs the amax passes
};

// What the blocked kernels (msda_block.hip) need to know about one call, built once per call.  `applies` is the answer to
// "are these your shapes": the launch calls take a plan that applies and cannot decline.
struct MsdaBlockPlan {
    bool applies = false;
    bool fuse_prep = false;                 // the raw forward may do the softmax / location arithmetic inside the forward kernel
    size_t workspace_bytes = 0;             // of the backward
    alignas(8) unsigned char geom[768];     // the kernels' geometry record (GeomB)
};

// the *_dev forms: geometry built on the device, buffers sized from (N, S, M, L, Lq) alone
struct MsdaDevPlan {
    bool applies = false;                   // ... and the runs and counters stay within 32-bit indexing
    int64_t tiles_bm = 0, ent_bm = 0;       // capacity per (image, head) of the tile counters / entry runs
    int blk_grid = 0, tile_grid = 0;        // launch sizes (multiples of 8) of the query-block kernels / the tile kernel
    size_t off_count = 0, off_ovf_count = 0, off_entries = 0, off_ovf = 0, total = 0;      // (the geometry record is at offset 0)
};

namespace mpf {
// msda.hip: first-generation kernels.  V = 4, 2, 1: msda_*_tiled_f32<32, V>; V = 0: msda_*_generic<T>
int msda_fwd_variant();
int msda_bwd_variant();
bool msda_tiled_ok(const MsdaProblem& p, int V);
void msda_launch_prep(const MsdaProblem& p, const MsdaOperands& o);
int msda_launch_forward(const MsdaProblem& p, const MsdaOperands& o, int V, const char* who);
int msda_launch_backward(const MsdaProblem& p, const MsdaOperands& o, int V);

// msda_block.hip: spatially blocked kernels
MsdaBlockPlan msda_block_plan(const MsdaProblem& p, const int64_t* host_shapes);
int msda_block_forward(const MsdaProblem& p, const MsdaOperands& o, const MsdaBlockPlan& plan, bool raw);
int msda_block_backward(const MsdaProblem& p, const MsdaOperands& o, const MsdaBlockPlan& plan);
size_t msda_block_workspace_bytes(const int64_t* host_shapes, int N, int M, int L, int Lq, int P);
MsdaDevPlan msda_block_dev_plan(const MsdaProblem& p, bool backward);
int msda_block_forward_dev(const MsdaProblem& p, const MsdaOperands& o, const MsdaDevPlan& plan);
int msda_block_backward_dev(const MsdaProblem& p, const MsdaOperands& o, const MsdaDevPlan& plan);

// msda_bwd_binned.hip: push + fill + pull
int msda_binned_backward(const MsdaProblem& p, const MsdaOperands& o);
}  // namespace mpf
