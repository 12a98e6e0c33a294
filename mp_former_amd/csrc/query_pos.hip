// Learned query positions of the clip decoder (video_mask2former_transformer_decoder.py:45-47, :104-106, :396): the operand
// of a projection that takes x + query_pos, and the way back.  Rows are sequence-first, r = q * N + n, 256 channels; the
// position of a row is qpos[r / N].
//   forward    out[r, c]  = bf16(x[r, c] + qpos[r / N, c])                   fp32 add, ONE round-to-nearest-even: what
//                                                                            (x + qpos).to(bfloat16) gives under autocast
//   backward   d_x0[r, c] += float(dxq0[r, c])                               (the cast's backward, added to the fp32 stream)
//              d_qpos[q, c] = sum_n (float(dxq0[q N + n, c]) + float(dxq1[q N + n, c]))      n ascending, fp32
// The N rows of a query are adjacent in memory, so one thread owns a (q, 8 channels) strip of the backward: d_qpos has one
// writer per element and is fully written (no atomics, nothing to zero, the same bits every run).  Both kernels only add, so
// there is nothing for the compiler to contract.  Memory-bound row kernels, 16-byte accesses, one pass each:
//   forward   R * 256 * (4 + 2) + Q * 256 * 4 bytes          backward   R * 256 * (2 + 2 + 4 + 4) + Q * 256 * 4 bytes
// (0.41 / 0.72 MB at 100 queries x 2 clips: launch-bound like the rest of the layer; no share of peak bandwidth was measured).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "mpf_common.h"

namespace {

constexpr int kC = 256, kC8 = kC / 8;

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

__device__ __forceinline__ void store8(float* dst, const float (&v)[8])
{
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

__device__ __forceinline__ void store8(__hip_bfloat16* dst, const float (&v)[8])
{
    unsigned w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const __hip_bfloat16 lo = __float2bfloat16(v[2 * j]), hi = __float2bfloat16(v[2 * j + 1]);      // round to nearest even
        w[j] = (unsigned)(*reinterpret_cast<const unsigned short*>(&lo)) | ((unsigned)(*reinterpret_cast<const unsigned short*>(&hi)) << 16);
    }
    *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
}

// thread = 8 consecutive channels of one row, channel group fastest
__global__ __launch_bounds__(256) void qpos_operand_fwd_kernel(const float* __restrict__ x, const float* __restrict__ qpos,
                                                               __hip_bfloat16* __restrict__ out, int Q, int N)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)Q * N * kC8) return;
    const int cg = (int)(idx % kC8);
    const int64_t r = idx / kC8;
    const int q = (int)(r / N);
    float a[8], p[8], v[8];
    load8(x + r * kC + 8 * cg, a);
    load8(qpos + (int64_t)q * kC + 8 * cg, p);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = a[j] + p[j];
    store8(out + r * kC + 8 * cg, v);
}

// thread = 8 consecutive channels of one query, walking its N rows in order
__global__ __launch_bounds__(256) void qpos_bwd_kernel(const __hip_bfloat16* __restrict__ dxq0, const __hip_bfloat16* __restrict__ dxq1,
                                                       float* __restrict__ d_x0, float* __restrict__ d_qpos, int Q, int N)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)Q * kC8) return;
    const int cg = (int)(idx % kC8);
    const int64_t q = idx / kC8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int n = 0; n < N; ++n) {
        const int64_t at = (q * N + n) * kC + 8 * cg;
        float a[8], b[8], d[8];
        load8(dxq0 + at, a);
        load8(dxq1 + at, b);
        load8(d_x0 + at, d);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            d[j] += a[j];
            acc[j] += a[j] + b[j];
        }
        store8(d_x0 + at, d);
    }
    store8(d_qpos + q * kC + 8 * cg, acc);
}

// acc[r, c] += float(g[r, c]): a bf16 gradient joining the fp32 chain of the residual stream (thread = 8 channels of one row)
__global__ __launch_bounds__(256) void bf16_rows_add_kernel(const __hip_bfloat16* __restrict__ g, float* __restrict__ acc, int64_t rows)
{
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * kC8) return;
    float a[8], d[8];
    load8(g + idx * 8, a);
    load8(acc + idx * 8, d);
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] += a[j];
    store8(acc + idx * 8, d);
}

int check_rows(const char* who, int Q, int N, int64_t* rows)
{
    if (Q <= 0 || N <= 0) return mpf::fail(MPF_E_SHAPE, who);
    *rows = (int64_t)Q * N;
    if (*rows * kC >= 0x7fffffffLL) return mpf::fail(MPF_E_TOO_LARGE, who);
    return 0;
}

}  // namespace

namespace mpf {
int bf16_rows_add256(const void* g, float* acc, int64_t rows, void* stream)
{
    if (!g || !acc) return fail(MPF_E_NULL, "bf16_rows_add256: NULL buffer");
    if (rows <= 0 || rows * kC >= 0x7fffffffLL || (((uintptr_t)g | (uintptr_t)acc) & 15))
        return fail(MPF_E_SHAPE, "bf16_rows_add256: positive row count below 2^31 elements and 16-B aligned buffers required");
    set_kernel("bf16_rows_add_kernel");
    hipLaunchKernelGGL(bf16_rows_add_kernel, dim3((unsigned)((rows * kC8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const __hip_bfloat16*)g, acc, rows);
    return check(hipGetLastError(), "bf16_rows_add256");
}
}  // namespace mpf

extern "C" int mpf_qpos_operand_forward(const float* x, const float* qpos, void* out, int Q, int N, void* stream)
{
    if (!x || !qpos || !out) return mpf::fail(MPF_E_NULL, "qpos_operand_forward: NULL buffer");
    int64_t rows = 0;
    if (int rc = check_rows("qpos_operand_forward: Q, N > 0 and fewer than 2^31 elements required", Q, N, &rows)) return rc;
    if (((uintptr_t)x | (uintptr_t)qpos | (uintptr_t)out) & 15)
        return mpf::fail(MPF_E_SHAPE, "qpos_operand_forward: buffers must be 16-B aligned");
    mpf::set_kernel("qpos_operand_fwd_kernel");
    hipLaunchKernelGGL(qpos_operand_fwd_kernel, dim3((unsigned)((rows * kC8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, qpos,
                       (__hip_bfloat16*)out, Q, N);
    return mpf::check(hipGetLastError(), "mpf_qpos_operand_forward");
}

extern "C" int mpf_qpos_backward(const void* dxq0, const void* dxq1, float* d_x0, float* d_qpos, int Q, int N, void* stream)
{
    if (!dxq0 || !dxq1 || !d_x0 || !d_qpos) return mpf::fail(MPF_E_NULL, "qpos_backward: NULL buffer");
    int64_t rows = 0;
    if (int rc = check_rows("qpos_backward: Q, N > 0 and fewer than 2^31 elements required", Q, N, &rows)) return rc;
    if (((uintptr_t)dxq0 | (uintptr_t)dxq1 | (uintptr_t)d_x0 | (uintptr_t)d_qpos) & 15)
        return mpf::fail(MPF_E_SHAPE, "qpos_backward: buffers must be 16-B aligned");
    mpf::set_kernel("qpos_bwd_kernel");
    hipLaunchKernelGGL(qpos_bwd_kernel, dim3((unsigned)(((int64_t)Q * kC8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const __hip_bfloat16*)dxq0, (const __hip_bfloat16*)dxq1, d_x0, d_qpos, Q, N);
    return mpf::check(hipGetLastError(), "mpf_qpos_backward");
}
