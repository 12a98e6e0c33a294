// bf16 weight gradients of a backbone stage's stride-1 convolutions as grouped launches — included at the end of gemm3.hip.
//
//   dW_i[co][tap * Cin + ci] = sum_r dY_i[r][co] * X_i[r shifted by the tap][ci]        (1x1: one tap, no shift)
//
// Every item is a problem of gemm3_nt_tile<128, BF = true> (one bf16 plane, one product, fp32 accumulator): 1x1 items in its plain
// form, 3x3 / stride 1 / padding 1 items in its CV form.  Items of one launch have DIFFERENT row counts (res5's first block still
// runs conv1 at the previous stride), so every item carries its own rows_per_split and its own slice of the partials workspace:
// the planner below cuts all of them into workgroups of about the same number of contracted rows.  A second grouped launch sums
// an item's splits in a fixed order, rounds the sum to bf16 (the value a bf16 weight gradient holds), multiplies by the
// FrozenBN scale of the output channel in fp32 and writes the fp32 gradient through the destination's strides — what the
// library's convolution backward followed by the stage's scale-and-cast launch computes, with another summation order.

namespace {

constexpr int kCwMax = MPF_CONV_WGRAD_GROUP_MAX;

struct G3NC {
    G3N it[kCwMax];
    int tile_end[kCwMax];
    unsigned char cv[kCwMax];       // 1: the item is a 3x3 convolution (gemm3_nt_tile's CV form)
    int n_items, ntiles;
};
static_assert(sizeof(G3NC) <= 4096, "kernel arguments are limited to 4 KB");

// the item's kind is a template argument of the tile (a workgroup-uniform branch around the whole tile, never around a load)
__global__ __launch_bounds__(kThreads, 2) void gemm3_nt_conv_group_kernel(G3NC g)
{
    const int per_xcd = (g.ntiles + 7) >> 3;
    const int tile = ((int)blockIdx.x & 7) * per_xcd + ((int)blockIdx.x >> 3);
    if (tile >= g.ntiles) return;
    int i = 0;
    while (i + 1 < g.n_items && tile >= g.tile_end[i]) ++i;
    const int first = i ? g.tile_end[i - 1] : 0;
    if (g.cv[i]) gemm3_nt_tile<128, true, true, false, false>(g.it[i], tile - first);
    else gemm3_nt_tile<128, true, false, false, false>(g.it[i], tile - first);
}

struct CwRed {
    const float* part;          // [nsplit][Cout][K]
    const float* scale;         // [Cout]
    float* out;
    int64_t sco, sci, stap;     // destination strides (elements) of the output channel, the input channel and the tap
    int nsplit, Cout, K, Cin, vec;      // vec: the four input channels of a thread are one aligned float4 of the destination
};
struct CwRedGroup {
    CwRed it[kCwMax];
    int block_end[kCwMax];
    int n_items;
};
static_assert(sizeof(CwRedGroup) <= 4096, "kernel arguments are limited to 4 KB");

// one float4 of k per thread; the splits in ascending order, 4 loads in flight
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(CwRedGroup g)
{
    int i = 0;
    while (i + 1 < g.n_items && (int)blockIdx.x >= g.block_end[i]) ++i;
    const CwRed& p = g.it[i];
    const int first = i ? g.block_end[i - 1] : 0;
    const int64_t total = (int64_t)p.Cout * p.K;
    const int64_t e = ((int64_t)((int)blockIdx.x - first) * 256 + threadIdx.x) * 4;
    if (e >= total) return;
    const float* src = p.part + e;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    int sp = 0;
    for (; sp + 4 <= p.nsplit; sp += 4) {
        float4 t[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) t[k] = *reinterpret_cast<const float4*>(src + (int64_t)(sp + k) * total);
#pragma unroll
        for (int k = 0; k < 4; ++k) { acc.x += t[k].x; acc.y += t[k].y; acc.z += t[k].z; acc.w += t[k].w; }
    }
    for (; sp < p.nsplit; ++sp) {
        const float4 t = *reinterpret_cast<const float4*>(src + (int64_t)sp * total);
        acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
    }
    auto bf16_rn = [](float f) -> float {           // round to nearest even, as a bf16 store does (finite gradients)
        unsigned u = __float_as_uint(f);
        u += 0x7fffu + ((u >> 16) & 1u);
        return __uint_as_float(u & 0xffff0000u);
    };
    const int co = (int)(e / p.K), k = (int)(e - (int64_t)co * p.K);
    const int tap = k / p.Cin, ci = k - tap * p.Cin;            // (Cin % 4 == 0: the four k of a thread share the tap)
    const float s = p.scale[co];
    const float4 o = make_float4(bf16_rn(acc.x) * s, bf16_rn(acc.y) * s, bf16_rn(acc.z) * s, bf16_rn(acc.w) * s);
    float* dst = p.out + (int64_t)co * p.sco + (int64_t)tap * p.stap + (int64_t)ci * p.sci;
    if (p.vec) {
        *reinterpret_cast<float4*>(dst) = o;
    } else {
        dst[0] = o.x; dst[p.sci] = o.y; dst[2 * p.sci] = o.z; dst[3 * p.sci] = o.w;
    }
}

inline int cw_taps(const MpfConvWgradItem& it) { return it.kind == MPF_CONV_WGRAD_3X3 ? 9 : 1; }

// the argument checks of an item that need no plan
int cw_check_item(const MpfConvWgradItem& it)
{
    if (it.kind != MPF_CONV_WGRAD_1X1 && it.kind != MPF_CONV_WGRAD_3X3) return mpf::fail(MPF_E_SHAPE, "conv_wgrad: kind is MPF_CONV_WGRAD_1X1 or _3X3");
    if (it.R <= 0 || it.Cout <= 0 || it.Cin <= 0 || it.Cin % 4 != 0 || it.Cout > (1 << 20) || it.Cin > (1 << 20))
        return mpf::fail(MPF_E_SHAPE, "conv_wgrad: sizes must be positive, Cin a multiple of 4");
    if ((int64_t)it.Cout * cw_taps(it) * it.Cin >= (1ll << 30)) return mpf::fail(MPF_E_TOO_LARGE, "conv_wgrad: a gradient of 2^30 elements or more");
    if (it.ld_dy < it.Cout || it.ld_x < it.Cin) return mpf::fail(MPF_E_SHAPE, "conv_wgrad: a row stride is shorter than the row");
    if (it.kind == MPF_CONV_WGRAD_3X3) {
        if (it.H <= 0 || it.W <= 0 || it.W % 8 != 0 || it.Cin % 128 != 0 || it.R % (it.H * it.W) != 0)
            return mpf::fail(MPF_E_SHAPE, "conv_wgrad: a 3x3 item needs W % 8 == 0, Cin % 128 == 0 and R = images * H * W");
    }
    return 0;
}

// launches of a stage: as few as the item cap allows, of equal size (17 items: 9 + 8, not 12 + 5)
inline int cw_launches(int n_items) { return cdiv(n_items, kCwMax); }
inline int cw_launch_begin(int n_items, int launch)
{
    const int per = cdiv(n_items, cw_launches(n_items));
    return std::min(n_items, launch * per);
}

// The splits of one launch.  In units of one K step (32 rows) of one 128 x 128 tile, item i is tiles_i x steps_i of work.  With
// a common split length L every (tile, split) workgroup contracts about L steps; L is chosen so that the launch's workgroups
// fill whole rounds of the chip's slots (two 256-thread workgroups per CU), as gemm3.balanced_rps does for one problem: the cost
// of a candidate is rounds x (its longest split + the epilogue, a 64 KB tile store worth about 8 steps of operand reads).  An
// item's partial sums (nsplit x Cout x K x 4 bytes) never exceed its operand bytes (2 R (Cout + K)): res5's 2 048 rows against
// a 512 x 4608 gradient keep 1 or 2 splits however many slots are idle.
void cw_plan_launch(const MpfConvWgradItem* items, int n, int slots, MpfConvWgradPlan* plans)
{
    int tiles[kCwMax], steps[kCwMax], cap[kCwMax], max_steps = 1;
    for (int i = 0; i < n; ++i) {
        const MpfConvWgradItem& it = items[i];
        const int64_t K = (int64_t)cw_taps(it) * it.Cin;
        tiles[i] = cdiv(it.Cout, kBM) * cdiv((int)K, 128);
        steps[i] = cdiv(it.R, kBK);
        const int64_t operand = 2 * (int64_t)it.R * (it.Cout + K), part = 4 * (int64_t)it.Cout * K;
        cap[i] = (int)std::max<int64_t>(1, std::min<int64_t>(operand / part, steps[i]));
        max_steps = std::max(max_steps, steps[i]);
    }
    int best_L = max_steps;
    double best_cost = 0.0;
    for (int L = max_steps; L >= 1; --L) {
        int64_t wgs = 0;
        int longest = 0;
        for (int i = 0; i < n; ++i) {
            const int ns = std::min(cap[i], cdiv(steps[i], L));
            wgs += (int64_t)tiles[i] * cdiv(steps[i], cdiv(steps[i], ns));
            longest = std::max(longest, cdiv(steps[i], ns));
        }
        if (wgs > 3 * (int64_t)slots && L < max_steps) break;          // more than three rounds: the partial sums only grow from here
        const double cost = (double)cdiv((int)wgs, slots) * (longest + 8);
        if (L == max_steps || cost < best_cost) { best_cost = cost; best_L = L; }
    }
    for (int i = 0; i < n; ++i) {
        const int ns = std::min(cap[i], cdiv(steps[i], best_L));
        const int len = cdiv(steps[i], ns);
        plans[i].rows_per_split = len * kBK;
        plans[i].nsplit = cdiv(steps[i], len);
        plans[i].tiles = tiles[i] * plans[i].nsplit;
    }
}

}  // namespace

extern "C" int mpf_conv_wgrad_group_max(void) { return kCwMax; }

extern "C" int mpf_conv_wgrad_plan(const MpfConvWgradItem* items, int n_items, int slots, MpfConvWgradPlan* plans,
                                   size_t* workspace_bytes)
{
    if (!items || !plans || !workspace_bytes) return mpf::fail(MPF_E_NULL, "conv_wgrad_plan: NULL argument");
    if (n_items <= 0 || slots < 0) return mpf::fail(MPF_E_SHAPE, "conv_wgrad_plan: n_items must be positive, slots >= 0 (0: the current device's)");
    for (int i = 0; i < n_items; ++i)
        if (int rc = cw_check_item(items[i])) return rc;
    if (slots == 0) slots = g3_slots();
    size_t off = 0;
    for (int l = 0; l < cw_launches(n_items); ++l) {
        const int b = cw_launch_begin(n_items, l), e = cw_launch_begin(n_items, l + 1);
        cw_plan_launch(items + b, e - b, slots, plans + b);
        for (int i = b; i < e; ++i) {
            plans[i].launch = l;
            plans[i].ws_offset = (int64_t)off;
            plans[i].ws_bytes = (int64_t)mpf::align256((size_t)plans[i].nsplit * items[i].Cout * cw_taps(items[i]) * items[i].Cin * sizeof(float));
            off += (size_t)plans[i].ws_bytes;
        }
    }
    *workspace_bytes = off;
    return 0;
}

extern "C" int mpf_conv_wgrad_bf16_grouped(const MpfConvWgradItem* items, int n_items, void* workspace, size_t workspace_bytes,
                                           void* stream)
{
    hipStream_t st = (hipStream_t)stream;
    if (!items || !workspace) return mpf::fail(MPF_E_NULL, "conv_wgrad_bf16_grouped: NULL argument");
    if (n_items <= 0) return mpf::fail(MPF_E_SHAPE, "conv_wgrad_bf16_grouped: n_items must be positive");
    // every item is checked before anything is launched
    for (int i = 0; i < n_items; ++i) {
        const MpfConvWgradItem& it = items[i];
        if (!it.dy || !it.x || !it.scale || !it.out) return mpf::fail(MPF_E_NULL, "conv_wgrad_bf16_grouped: NULL buffer in an item");
        if (int rc = cw_check_item(it)) return rc;
        if (it.rows_per_split <= 0 || it.rows_per_split % kBK != 0)
            return mpf::fail(MPF_E_SHAPE, "conv_wgrad_bf16_grouped: rows_per_split must be a positive multiple of 32");
        const size_t need = (size_t)cdiv(it.R, it.rows_per_split) * it.Cout * cw_taps(it) * it.Cin * sizeof(float);
        if (it.ws_offset < 0 || it.ws_offset % 16 != 0 || (size_t)it.ws_offset + need > workspace_bytes)
            return mpf::fail(MPF_E_SHAPE, "conv_wgrad_bf16_grouped: an item's partial sums do not fit its slice of the workspace");
        for (int j = 0; j < i; ++j) {           // slices are disjoint
            const MpfConvWgradItem& o = items[j];
            const size_t need_o = (size_t)cdiv(o.R, o.rows_per_split) * o.Cout * cw_taps(o) * o.Cin * sizeof(float);
            if ((size_t)it.ws_offset < (size_t)o.ws_offset + need_o && (size_t)o.ws_offset < (size_t)it.ws_offset + need)
                return mpf::fail(MPF_E_SHAPE, "conv_wgrad_bf16_grouped: two items share workspace");
        }
    }
    for (int l = 0; l < cw_launches(n_items); ++l) {
        const int b = cw_launch_begin(n_items, l), e = cw_launch_begin(n_items, l + 1);
        G3NC g{};
        CwRedGroup r{};
        Work w{0.0, 0.0};
        double red_bytes = 0.0;
        int blocks = 0;
        for (int i = b; i < e; ++i) {
            const MpfConvWgradItem& it = items[i];
            const bool cv = it.kind == MPF_CONV_WGRAD_3X3;
            G3N& p = g.it[i - b];
            float* part = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + it.ws_offset);
            if (int rc = g3n_fill(p, "conv_wgrad_bf16_grouped", it.dy, it.ld_dy, 2, it.x, it.ld_x, 2, part, nullptr, it.R, it.Cout, it.Cin,
                                  it.rows_per_split))
                return rc;
            if (cv) {       // B in memory is the image [R, Cin]; the product's columns are (tap, channel)
                p.Ndim = 9 * it.Cin; p.c_ss = (int64_t)p.Mdim * p.Ndim; p.csb_ss = p.Ndim;
                p.cv_H = it.H; p.cv_W = it.W; p.cv_cin = it.Cin;
            }
            g3n_tiles(p, kBM, 128);
            g.cv[i - b] = cv ? 1 : 0;
            g.ntiles += p.ntiles;
            g.tile_end[i - b] = g.ntiles;
            const Work wi = g3n_work(p, 2.0, 2.0);
            w.bytes += wi.bytes; w.flops += wi.flops;

            CwRed& q = r.it[i - b];
            q.part = part; q.scale = it.scale; q.out = it.out;
            q.sco = it.out_stride_co; q.sci = it.out_stride_ci; q.stap = it.out_stride_tap;
            q.nsplit = p.nsplit; q.Cout = it.Cout; q.K = p.Ndim; q.Cin = it.Cin;
            q.vec = q.sci == 1 && q.sco % 4 == 0 && (!cv || q.stap % 4 == 0) && ((uintptr_t)it.out & 15) == 0;
            blocks += cdiv(it.Cout * p.Ndim, 1024);
            r.block_end[i - b] = blocks;
            red_bytes += 4.0 * (p.nsplit + 1) * it.Cout * p.Ndim;
        }
        g.n_items = r.n_items = e - b;
        if (int rc = g3_launch(g3n_route((const void*)gemm3_nt_conv_group_kernel, "gemm3_nt_group_kernel<bf16 conv>",
                                         "mpf_conv_wgrad_bf16_grouped", g.ntiles), g, st, w))
            return rc;
        Route rr;
        rr.fn = (const void*)conv_wgrad_reduce_kernel; rr.name = "conv_wgrad_reduce_kernel"; rr.what = "mpf_conv_wgrad_bf16_grouped(reduce)";
        rr.blocks = blocks;
        if (int rc = g3_launch(rr, r, st, Work{red_bytes, 0.0})) return rc;
    }
    return 0;
}
