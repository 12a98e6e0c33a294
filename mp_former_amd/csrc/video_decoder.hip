// Video decoder kernels for MI355X.
//
// Clip decoder inputs of one feature level (video_mask2former_transformer_decoder.py:385-393 with the key input of :105 and
// PositionEmbeddingSine3D, position_encoding.py:56): from the level's feature maps of B clips x T frames, x(b * T + t, c, s) — a
// channel-last VIEW of the encoder memory whose frames need not be dense —
//   src[(t * S + s), b, c] = x(b * T + t, c, s) + level_embed[c]                  (value input of the cross-attention)
//   kin[(t * S + s), b, c] = src[...] + (pos_yx[s, c] + pos_z[t, c])              (key input: + the 3D sine embedding)
// both frame-major, sequence-first, row-contiguous, bf16 (autocast) or fp32.  The 3D embedding is the sum of a per-pixel and a
// per-frame table, so the [T * S, C] table of a whole video (over 100 MB at 36 frames of 45 x 80) is never formed.  fp32
// arithmetic in the order written: x + level first, the two tables summed first as the reference sums them, then one add; the
// kernel only adds, so there is nothing for the compiler to contract.
// Backward: dx(b * T + t, c, s) = g_src[...] + g_kin[...] (either may be NULL), written with x's strides.
// Memory-bound, one pass each way.  Thread = 8 consecutive channels of one (t, s, b), as in decoder.hip's image kernels.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "mpf_common.h"

namespace {

template <typename TO>
__device__ __forceinline__ void store8(TO* dst, const float (&v)[8]);

template <>
__device__ __forceinline__ void store8<float>(float* dst, const float (&v)[8])
{
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

template <>
__device__ __forceinline__ void store8<__hip_bfloat16>(__hip_bfloat16* dst, const float (&v)[8])
{
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const __hip_bfloat16 lo = __float2bfloat16(v[2 * j]), hi = __float2bfloat16(v[2 * j + 1]);
        w[j] = (unsigned)(*reinterpret_cast<const unsigned short*>(&lo)) | ((unsigned)(*reinterpret_cast<const unsigned short*>(&hi)) << 16);
    }
    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void load8(const float* p, float (&v)[8])
{
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

__device__ __forceinline__ void load8(const __hip_bfloat16* p, float (&v)[8])
{
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[2 * j] = __uint_as_float(w[j] << 16);
        v[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
    }
}

// idx -> (t, s, b, 8-channel group), channel group fastest: consecutive threads write consecutive 16 / 32 bytes of the outputs
struct ClipIndex {
    int t, s, b, cg;
    int64_t in, out;                 // element offsets into x / dx and into src / kin / their gradients
};

__device__ __forceinline__ ClipIndex clip_index(int64_t idx, int64_t sx_n, int64_t sx_s, int S, int T, int B, int C)
{
    const int c8 = C >> 3;
    ClipIndex k;
    k.cg = (int)(idx % c8);
    k.b = (int)((idx / c8) % B);
    const int64_t row = idx / ((int64_t)c8 * B);         // t * S + s
    k.t = (int)(row / S);
    k.s = (int)(row - (int64_t)k.t * S);
    k.in = ((int64_t)k.b * T + k.t) * sx_n + (int64_t)k.s * sx_s + 8 * k.cg;
    k.out = (row * B + k.b) * C + 8 * k.cg;
    return k;
}

template <typename TO>
__global__ __launch_bounds__(256) void clip_inputs_fwd_kernel(const float* __restrict__ x, int64_t sx_n, int64_t sx_s,
                                                              const float* __restrict__ level_embed, const float* __restrict__ pos_yx,
                                                              const float* __restrict__ pos_z, TO* __restrict__ src,
                                                              TO* __restrict__ kin, int S, int T, int B, int C)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)T * S * B * (C >> 3)) return;
    const ClipIndex k = clip_index(idx, sx_n, sx_s, S, T, B, C);
    float a[8], e[8], pyx[8], pz[8], v[8], kk[8];
    load8(x + k.in, a);
    load8(level_embed + 8 * k.cg, e);
    load8(pos_yx + (int64_t)k.s * C + 8 * k.cg, pyx);
    load8(pos_z + (int64_t)k.t * C + 8 * k.cg, pz);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        v[j] = a[j] + e[j];
        const float p = pyx[j] + pz[j];
        kk[j] = v[j] + p;
    }
    store8<TO>(src + k.out, v);
    store8<TO>(kin + k.out, kk);
}

template <typename TG>
__global__ __launch_bounds__(256) void clip_inputs_bwd_kernel(const TG* __restrict__ g_src, const TG* __restrict__ g_kin,
                                                              float* __restrict__ dx, int64_t sx_n, int64_t sx_s, int S, int T, int B,
                                                              int C)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)T * S * B * (C >> 3)) return;
    const ClipIndex k = clip_index(idx, sx_n, sx_s, S, T, B, C);
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (g_src) load8(g_src + k.out, a);
    if (g_kin) load8(g_kin + k.out, b);
    float d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = a[j] + b[j];
    store8<float>(dx + k.in, d);
}

// shared argument check of the two entry points; `total` = number of threads
int check_clip_shape(const char* who, const void* x, int64_t sx_n, int64_t sx_s, int S, int T, int B, int C, int64_t* total)
{
    if (S < 0 || T < 0 || B < 0 || C <= 0 || C % 8 || sx_n % 4 || sx_s % 4 || sx_n < 0 || sx_s < 0 || ((uintptr_t)x & 15)) {
        return mpf::fail(MPF_E_SHAPE, who);
    }
    *total = (int64_t)T * S * B * (C / 8);
    if ((*total + 255) / 256 > 0x7fffffffLL) return mpf::fail(MPF_E_TOO_LARGE, who);
    return 0;
}

}  // namespace

extern "C" int mpf_clip_inputs_forward(const float* x, int64_t sx_n, int64_t sx_s, const float* level_embed, const float* pos_yx,
                                       const float* pos_z, void* src, void* kin, int out_dtype, int S, int T, int B, int C,
                                       void* stream)
{
    if (S == 0 || T == 0 || B == 0) return 0;
    if (!x || !level_embed || !pos_yx || !pos_z || !src || !kin) return mpf::fail(MPF_E_NULL, "clip_inputs_forward: NULL buffer");
    int64_t total = 0;
    if (int rc = check_clip_shape("clip_inputs_forward: C % 8 == 0 and 16-B aligned rows (unit channel stride) required", x, sx_n, sx_s,
                                  S, T, B, C, &total))
        return rc;
    if (((uintptr_t)level_embed | (uintptr_t)pos_yx | (uintptr_t)pos_z | (uintptr_t)src | (uintptr_t)kin) & 15)
        return mpf::fail(MPF_E_SHAPE, "clip_inputs_forward: tables and outputs must be 16-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((total + 255) / 256));
    mpf::set_kernel("clip_inputs_fwd_kernel");
    if (out_dtype == MPF_BF16)
        hipLaunchKernelGGL(clip_inputs_fwd_kernel<__hip_bfloat16>, grid, dim3(256), 0, st, x, sx_n, sx_s, level_embed, pos_yx, pos_z,
                           (__hip_bfloat16*)src, (__hip_bfloat16*)kin, S, T, B, C);
    else if (out_dtype == MPF_F32)
        hipLaunchKernelGGL(clip_inputs_fwd_kernel<float>, grid, dim3(256), 0, st, x, sx_n, sx_s, level_embed, pos_yx, pos_z, (float*)src,
                           (float*)kin, S, T, B, C);
    else
        return mpf::fail(MPF_E_DTYPE, "clip_inputs_forward: out dtype must be MPF_F32 or MPF_BF16");
    return mpf::check(hipGetLastError(), "mpf_clip_inputs_forward");
}

extern "C" int mpf_clip_inputs_backward(const void* g_src, const void* g_kin, int g_dtype, float* dx, int64_t sx_n, int64_t sx_s, int S,
                                        int T, int B, int C, void* stream)
{
    if (S == 0 || T == 0 || B == 0) return 0;
    if (!dx || (!g_src && !g_kin)) return mpf::fail(MPF_E_NULL, "clip_inputs_backward: NULL buffer");
    int64_t total = 0;
    if (int rc = check_clip_shape("clip_inputs_backward: C % 8 == 0 and 16-B aligned rows required", dx, sx_n, sx_s, S, T, B, C, &total))
        return rc;
    if (((uintptr_t)g_src | (uintptr_t)g_kin) & 15)
        return mpf::fail(MPF_E_SHAPE, "clip_inputs_backward: gradients must be 16-B aligned");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((total + 255) / 256));
    mpf::set_kernel("clip_inputs_bwd_kernel");
    if (g_dtype == MPF_BF16)
        hipLaunchKernelGGL(clip_inputs_bwd_kernel<__hip_bfloat16>, grid, dim3(256), 0, st, (const __hip_bfloat16*)g_src,
                           (const __hip_bfloat16*)g_kin, dx, sx_n, sx_s, S, T, B, C);
    else if (g_dtype == MPF_F32)
        hipLaunchKernelGGL(clip_inputs_bwd_kernel<float>, grid, dim3(256), 0, st, (const float*)g_src, (const float*)g_kin, dx, sx_n,
                           sx_s, S, T, B, C);
    else
        return mpf::fail(MPF_E_DTYPE, "clip_inputs_backward: gradient dtype must be MPF_F32 or MPF_BF16");
    return mpf::check(hipGetLastError(), "mpf_clip_inputs_backward");
}
