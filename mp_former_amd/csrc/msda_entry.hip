// The ten MSDA op entry points (include/mpformer_hip.h).  Host code only: every entry is record, check, route, launch.
//   record   one MsdaProblem (sizes + dtype) and one MsdaOperands (pointers, workspace, stream) — msda_host.h
//   check    msda_check: NULL pointers, then dtype, then sizes; limits of one route stay with that route
//   route    msda_forward_route / msda_backward_route: pure functions of the problem, the variant option, the operands present, the plan
//   launch   the launcher of the chosen family, in msda.hip (tiled, generic, prep), msda_block.hip (blocked) or msda_bwd_binned.hip
// DESIGN.md ("MSDA host layer") has the table entry x condition -> kernel sequence.
#include "msda_host.h"

namespace {

// `who` names the entry family in the texts.  Order: NULL, dtype, sizes.  ws: the _ws forms, which serve fp32 with 32 channels
// per head only and say so in the dtype slot; their size text is their own.
int msda_check(const char* who, const MsdaProblem& p, bool ws, std::initializer_list<const void*> required)
{
    const auto failf = [&](int code, const char* what) { return mpf::failf(code, who, what); };
    if (mpf::any_null(required)) return failf(MPF_E_NULL, "NULL buffer");
    const bool sizes_ok = p.N > 0 && p.S > 0 && p.M > 0 && p.D > 0 && p.L > 0 && p.Lq > 0 && p.P > 0;
    if (ws) {
        if (p.dtype != MPF_F32 || p.D != 32) return failf(MPF_E_DTYPE, "fp32 with 32 channels per head only");
        return sizes_ok ? 0 : failf(MPF_E_SHAPE, "bad sizes");
    }
    if (p.dtype != MPF_F32 && p.dtype != MPF_F64) return mpf::fail(MPF_E_DTYPE, "msda: dtype must be MPF_F32 or MPF_F64");
    if (!sizes_ok) return mpf::fail(MPF_E_SHAPE, "msda: all sizes must be positive");
    return p.L > 16 ? mpf::fail(MPF_E_SHAPE, "msda: num_levels > 16 not supported") : 0;
}

// first-generation kernels: msda_fwd_variant / msda_bwd_variant -> channels per lane of the tiled kernels (0: generic); variant
// 0 is variant 3, and a tiled kernel that cannot serve the problem falls to the generic one
MsdaRoute first_generation_route(const MsdaProblem& p, int variant)
{
    constexpr int kVariantV[5] = {1, 0, 4, 1, 2};
    const int V = kVariantV[variant];
    if (V && mpf::msda_tiled_ok(p, V)) return {MsdaFamily::tiled, V};
    return {MsdaFamily::generic};
}

// plan.applies: host shapes that msda_block_plan accepted; dev: a *_dev call that msda_block_dev_plan accepted
MsdaRoute msda_forward_route(const MsdaProblem& p, int variant, const MsdaOperands& o, const MsdaBlockPlan& plan, bool dev)
{
    if (dev) return {MsdaFamily::blocked_dev};
    if (variant == 0 && plan.applies) {
        if (o.raw && plan.fuse_prep) return {MsdaFamily::blocked_raw};
        return {MsdaFamily::blocked, 0, o.raw != nullptr};
    }
    if (o.raw) return {MsdaFamily::tiled, 1, true};      // (the raw form's own limits imply msda_tiled_ok(p, 1))
    return first_generation_route(p, variant);
}

MsdaRoute msda_backward_route(const MsdaProblem& p, int variant, const MsdaOperands& o, const MsdaBlockPlan& plan, bool dev)
{
    if (dev) return {MsdaFamily::blocked_dev};
    if (!o.host_shapes) return first_generation_route(p, variant);
    // the _ws forms.  The raw form needs the forward result for bin + tile (delta = <grad_out, out>), and records the amax slots
    if (plan.applies && (!o.grad_raw || o.fwd_out)) return {MsdaFamily::blocked, 0, false, o.grad_raw != nullptr};
    return {MsdaFamily::binned};
}

int forward(const char* who, const MsdaProblem& p, const MsdaOperands& o, bool dev = false)
{
    if (int e = msda_check(who, p, false, {o.value, o.shapes, o.lsi, o.loc, o.attn, o.out})) return e;
    const MsdaDevPlan dplan = dev ? mpf::msda_block_dev_plan(p, false) : MsdaDevPlan();
    const MsdaBlockPlan plan = mpf::msda_block_plan(p, o.host_shapes);
    const MsdaRoute r = msda_forward_route(p, mpf::msda_fwd_variant(), o, plan, dplan.applies);
    if (r.family == MsdaFamily::blocked_dev) return mpf::msda_block_forward_dev(p, o, dplan);
    if (r.family == MsdaFamily::blocked) return mpf::msda_block_forward(p, o, plan, false);
    return mpf::msda_launch_forward(p, o, r.V, "mpf_msda_forward");      // (the *_dev forms too: other dtypes / head widths / points)
}

int forward_raw(const MsdaProblem& p, const MsdaOperands& o)
{
    if (int e = msda_check("msda_forward_raw", p, false, {o.value, o.shapes, o.lsi, o.raw, o.ref, o.out, o.loc, o.attn})) return e;
    if (!mpf::msda_tiled_ok(p, 1) || p.L * p.P > 32)
        return mpf::fail(MPF_E_DTYPE, "msda_forward_raw: fp32 with 32 channels per head and L*P <= 32 only");
    const MsdaBlockPlan plan = mpf::msda_block_plan(p, o.host_shapes);
    const MsdaRoute r = msda_forward_route(p, mpf::msda_fwd_variant(), o, plan, false);
    if (r.prep) mpf::msda_launch_prep(p, o);
    if (r.family == MsdaFamily::tiled) return mpf::msda_launch_forward(p, o, r.V, "mpf_msda_forward_raw");
    return mpf::msda_block_forward(p, o, plan, r.family == MsdaFamily::blocked_raw);
}

int backward(const char* who, const MsdaProblem& p, const MsdaOperands& o, bool dev = false)
{
    if (int e = msda_check(who, p, false, {o.value, o.shapes, o.lsi, o.loc, o.attn, o.grad_out, o.grad_value, o.grad_loc, o.grad_attn}))
        return e;
    const MsdaDevPlan dplan = dev ? mpf::msda_block_dev_plan(p, true) : MsdaDevPlan();
    MsdaBlockPlan none;      // (host shapes are what the _ws forms have)
    const MsdaRoute r = msda_backward_route(p, mpf::msda_bwd_variant(), o, none, dplan.applies);
    return r.family == MsdaFamily::blocked_dev ? mpf::msda_block_backward_dev(p, o, dplan) : mpf::msda_launch_backward(p, o, r.V);
}

// the amax slots of grad_value / grad_raw by a pass over the data: every route whose kernels do not record them themselves
int amax_after(const MsdaProblem& p, const MsdaOperands& o)
{
    if (o.gv_amax)
        if (int r = mpf_amax_f32((const float*)o.grad_value, p.n_value(), o.gv_amax, o.stream)) return r;
    if (o.graw_amax && o.grad_raw)
        if (int r = mpf_amax_f32((const float*)o.grad_raw, p.n_samples() * 3, o.graw_amax, o.stream)) return r;
    return 0;
}

// plan, then blocked or binned, then the amax passes exactly when the chosen route does not record the slots itself
int backward_ws(const MsdaProblem& p, const MsdaOperands& o)
{
    const void *gl = o.grad_raw ? o.grad_raw : o.grad_loc, *ga = o.grad_raw ? o.grad_raw : o.grad_attn;
    if (int e = msda_check("msda_backward_ws", p, true, {o.value, o.host_shapes, o.loc, o.attn, o.grad_out, o.grad_value, gl, ga, o.workspace}))
        return e;
    const MsdaBlockPlan plan = mpf::msda_block_plan(p, o.host_shapes);
    const MsdaRoute r = msda_backward_route(p, 0, o, plan, false);
    if (int e = r.family == MsdaFamily::blocked ? mpf::msda_block_backward(p, o, plan) : mpf::msda_binned_backward(p, o)) return e;
    return r.records_amax ? 0 : amax_after(p, o);
}

}  // namespace

// The size tail of every entry, and the operands the forward / backward forms share
#define MSDA_SIZES int batch, int spatial_size, int num_heads, int channels, int num_levels, int num_query, int num_point, int dtype
#define MSDA_PROBLEM MsdaProblem{batch, spatial_size, num_heads, channels, num_levels, num_query, num_point, dtype}

static MsdaOperands operands(const void* value, const int64_t* shapes, const int64_t* lsi, const int64_t* host_shapes, const void* loc,
                             const void* attn, void* workspace, size_t workspace_bytes, void* stream)
{
    MsdaOperands o;
    o.value = value; o.shapes = shapes; o.lsi = lsi; o.host_shapes = host_shapes; o.loc = loc; o.attn = attn;
    o.workspace = workspace; o.workspace_bytes = workspace_bytes; o.stream = (hipStream_t)stream;
    return o;
}

extern "C" int mpf_msda_forward(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                const void* sampling_loc, const void* attn_weight, void* output, MSDA_SIZES, void* stream)
{
    return mpf_msda_forward_hs(value, spatial_shapes, level_start_index, nullptr, sampling_loc, attn_weight, output, batch, spatial_size,
                               num_heads, channels, num_levels, num_query, num_point, dtype, stream);
}

extern "C" int mpf_msda_forward_hs(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                   const int64_t* host_spatial_shapes, const void* sampling_loc, const void* attn_weight, void* output,
                                   MSDA_SIZES, void* stream)
{
    MsdaOperands o = operands(value, spatial_shapes, level_start_index, host_spatial_shapes, sampling_loc, attn_weight, nullptr, 0, stream);
    o.out = output;
    return forward("msda_forward", MSDA_PROBLEM, o);
}

extern "C" int mpf_msda_forward_dev(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                    const void* sampling_loc, const void* attn_weight, void* output, MSDA_SIZES, void* workspace,
                                    size_t workspace_bytes, void* stream)
{
    MsdaOperands o = operands(value, spatial_shapes, level_start_index, nullptr, sampling_loc, attn_weight, workspace, workspace_bytes, stream);
    o.out = output;
    return forward("msda_forward_dev", MSDA_PROBLEM, o, true);
}

extern "C" int mpf_msda_forward_raw(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index, const void* raw,
                                    const void* ref_points, void* loc_out, void* attn_out, void* output, MSDA_SIZES, void* stream)
{
    return mpf_msda_forward_raw_hs(value, spatial_shapes, level_start_index, nullptr, raw, ref_points, loc_out, attn_out, output, batch,
                                   spatial_size, num_heads, channels, num_levels, num_query, num_point, dtype, stream);
}

extern "C" int mpf_msda_forward_raw_hs(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                       const int64_t* host_spatial_shapes, const void* raw, const void* ref_points, void* loc_out,
                                       void* attn_out, void* output, MSDA_SIZES, void* stream)
{
    MsdaOperands o = operands(value, spatial_shapes, level_start_index, host_spatial_shapes, loc_out, attn_out, nullptr, 0, stream);
    o.raw = raw; o.ref = ref_points; o.out = output;
    return forward_raw(MSDA_PROBLEM, o);
}

extern "C" int mpf_msda_backward(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                 const void* sampling_loc, const void* attn_weight, const void* grad_output, void* grad_value,
                                 void* grad_sampling_loc, void* grad_attn_weight, MSDA_SIZES, void* stream)
{
    MsdaOperands o = operands(value, spatial_shapes, level_start_index, nullptr, sampling_loc, attn_weight, nullptr, 0, stream);
    o.grad_out = grad_output; o.grad_value = grad_value; o.grad_loc = grad_sampling_loc; o.grad_attn = grad_attn_weight;
    return backward("msda_backward", MSDA_PROBLEM, o);
}

extern "C" int mpf_msda_backward_dev(const void* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                     const void* sampling_loc, const void* attn_weight, const void* grad_output, void* grad_value,
                                     void* grad_sampling_loc, void* grad_attn_weight, MSDA_SIZES, void* workspace, size_t workspace_bytes,
                                     void* stream)
{
    MsdaOperands o = operands(value, spatial_shapes, level_start_index, nullptr, sampling_loc, attn_weight, workspace, workspace_bytes, stream);
    o.grad_out = grad_output; o.grad_value = grad_value; o.grad_loc = grad_sampling_loc; o.grad_attn = grad_attn_weight;
    return backward("msda_backward_dev", MSDA_PROBLEM, o, true);
}

extern "C" int mpf_msda_backward_ws(const void* value, const int64_t* host_spatial_shapes, const void* sampling_loc,
                                    const void* attn_weight, const void* grad_output, void* grad_value, void* grad_sampling_loc,
                                    void* grad_attn_weight, MSDA_SIZES, void* workspace, size_t workspace_bytes, void* stream)
{
    MsdaOperands o = operands(value, nullptr, nullptr, host_spatial_shapes, sampling_loc, attn_weight, workspace, workspace_bytes, stream);
    o.grad_out = grad_output; o.grad_value = grad_value; o.grad_loc = grad_sampling_loc; o.grad_attn = grad_attn_weight;
    return backward_ws(MSDA_PROBLEM, o);
}

extern "C" int mpf_msda_backward_ws_raw(const void* value, const int64_t* host_spatial_shapes, const void* sampling_loc,
                                        const void* attn_weight, const void* grad_output, void* grad_value, void* grad_raw, MSDA_SIZES,
                                        void* workspace, size_t workspace_bytes, void* stream)
{
    if (!grad_raw) return mpf::fail(MPF_E_NULL, "msda_backward_ws_raw: NULL grad_raw");
    MsdaOperands o = operands(value, nullptr, nullptr, host_spatial_shapes, sampling_loc, attn_weight, workspace, workspace_bytes, stream);
    o.grad_out = grad_output; o.grad_value = grad_value; o.grad_raw = grad_raw;
    return backward_ws(MSDA_PROBLEM, o);
}

// raw form with the forward result at hand (the module keeps it): the softmax-backward sum of a (query, head) is
// <grad_output, output> of that (query, head), so the destination-side kernels (bin + tile, msda_block.hip) apply
extern "C" int mpf_msda_backward_ws_raw_o(const void* value, const int64_t* host_spatial_shapes, const void* sampling_loc,
                                          const void* attn_weight, const void* grad_output, const void* output, void* grad_value,
                                          void* grad_raw, MSDA_SIZES, void* workspace, size_t workspace_bytes, float* grad_raw_amax,
                                          float* grad_value_amax, void* stream)
{
    if (!grad_raw || !output) return mpf::fail(MPF_E_NULL, "msda_backward_ws_raw_o: NULL grad_raw / output");
    MsdaOperands o = operands(value, nullptr, nullptr, host_spatial_shapes, sampling_loc, attn_weight, workspace, workspace_bytes, stream);
    o.grad_out = grad_output; o.fwd_out = output; o.grad_value = grad_value; o.grad_raw = grad_raw;
    o.graw_amax = grad_raw_amax; o.gv_amax = grad_value_amax;
    return backward_ws(MSDA_PROBLEM, o);
}
