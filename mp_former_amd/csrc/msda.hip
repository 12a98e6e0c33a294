// Multi-scale deformable attention (MSDA) forward / backward for MI355X (gfx950, wave64).
//
// What it computes (reference: mask2former/modeling/pixel_decoder/ops/src/cuda/
// ms_deform_im2col_cuda.cuh:242-304 forward, :306-408 + :92-164 backward):
//   out[b,q,m,:] = sum_{l,p} A[b,q,m,l,p] * bilinear(V_l[b,:,m,:], loc[b,q,m,l,p])
// with zero padding, align_corners=False pixel coordinates (x = loc_x*W - 0.5).
//
// Design (written for CDNA4, not translated from the CUDA kernels):
//   * work unit = one (query, head) pair "qm"; a 256-thread workgroup owns QMB consecutive qm.
//   * phase 1: the workgroup decodes its QMB*L*P sampling points ONCE, cooperatively and with
//     coalesced reads of sampling_loc / attn_weight, into LDS "sample descriptors"
//     (4 corner row offsets + 4 corner weights).  The reference re-derives them per channel.
//   * phase 2: G = D/V lanes share one qm; each lane owns V consecutive channels and gathers the
//     4 corner rows with V*4-byte vector loads (V=4: one 128-B value row = 8 lanes x 16 B, a wave
//     instruction fetches 8 full rows).  Descriptors are LDS broadcasts.
//   * backward: per-point partial sums for grad_attn / grad_loc are reduced across the G lanes of a
//     qm with DPP/shuffle butterflies (no LDS, no barriers), staged in LDS and written coalesced;
//     grad_value goes out as hardware fp32 atomics (global_atomic_add_f32).
//   * blockIdx -> tile mapping is XCD-aware: the 8 XCDs (private L2s) each walk a contiguous
//     1/8 of the (image, query) range, so the value rows a tile gathers are L2-resident.
//   * any other shape / dtype (D != 32, fp64) takes the generic kernels below (correctness path
//     used by the reference's own test matrix: D in {2,30,32,64,71,1025,2048,3096}, fp64).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msda_host.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxLevels = 16;

template <typename T, int V> struct VecT;
template <> struct VecT<float, 4> { using type = float4; };
template <> struct VecT<float, 2> { using type = float2; };
template <> struct VecT<float, 1> { using type = float; };

__device__ __forceinline__ void vec_load(float (&r)[4], const float* p) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
}
__device__ __forceinline__ void vec_load(float (&r)[2], const float* p) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    r[0] = v.x; r[1] = v.y;
}
__device__ __forceinline__ void vec_load(float (&r)[1], const float* p) { r[0] = *p; }
__device__ __forceinline__ void vec_store(float* p, const float (&r)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
}
__device__ __forceinline__ void vec_store(float* p, const float (&r)[2]) {
    *reinterpret_cast<float2*>(p) = make_float2(r[0], r[1]);
}
__device__ __forceinline__ void vec_store(float* p, const float (&r)[1]) { *p = r[0]; }

// Gather through a buffer descriptor: the element offset comes from the sample descriptor, and a corner
// that contributes nothing is encoded as offset -1, which becomes a byte offset beyond num_records —
// the hardware bounds check returns 0 for it, so the four corner loads need no branch / exec masking.
__device__ __forceinline__ void buf_load(float (&r)[4], __amdgpu_buffer_rsrc_t rs, int elem_off, int lane_bytes) {
    const unsigned vo = elem_off < 0 ? 0x80000000u : (unsigned)elem_off * 4u + (unsigned)lane_bytes;
    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)vo, 0, 0);
    r[0] = __int_as_float(v[0]); r[1] = __int_as_float(v[1]); r[2] = __int_as_float(v[2]); r[3] = __int_as_float(v[3]);
}
__device__ __forceinline__ void buf_load(float (&r)[2], __amdgpu_buffer_rsrc_t rs, int elem_off, int lane_bytes) {
    const unsigned vo = elem_off < 0 ? 0x80000000u : (unsigned)elem_off * 4u + (unsigned)lane_bytes;
    const auto v = __builtin_amdgcn_raw_buffer_load_b64(rs, (int)vo, 0, 0);
    r[0] = __int_as_float(v[0]); r[1] = __int_as_float(v[1]);
}
__device__ __forceinline__ void buf_load(float (&r)[1], __amdgpu_buffer_rsrc_t rs, int elem_off, int lane_bytes) {
    const unsigned vo = elem_off < 0 ? 0x80000000u : (unsigned)elem_off * 4u + (unsigned)lane_bytes;
    r[0] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)vo, 0, 0));
}

// XCD-aware tile index: workgroup b is observed to run on XCD b % 8 (speed only, never
// correctness); give each XCD a contiguous run of tiles.  Bijective for any ntiles because the
// grid is rounded up to a multiple of 8 and surplus workgroups exit.
__device__ __forceinline__ int xcd_tile(int ntiles) {
    const int per_xcd = (ntiles + 7) >> 3;
    const int bid = (int)blockIdx.x;
    return (bid & 7) * per_xcd + (bid >> 3);
}

// sum over the G (power of two, <= 64) consecutive lanes that share one qm
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
}

struct LevelInfo {
    int H[kMaxLevels], W[kMaxLevels], start[kMaxLevels];
};

// --------------------------------------------------------------------------------------------
// Tiled forward, fp32.  D = channels per head, V = channels per lane.
// LDS: per sampling point 4 x int32 corner offsets (elements, -1 = corner contributes nothing)
//      + 4 x f32 weights (bilinear weight * attention weight).
// --------------------------------------------------------------------------------------------
template <int D, int V>
__global__ __launch_bounds__(kThreads) void msda_fwd_tiled_f32(
    const float* __restrict__ value, const int64_t* __restrict__ shapes,
    const int64_t* __restrict__ level_start, const float* __restrict__ loc,
    const float* __restrict__ attn, float* __restrict__ out,
    int S, int M, int L, int Lq, int P, int total_qm, int ntiles, unsigned value_bytes)
{
    constexpr int G = D / V;               // lanes per qm
    constexpr int QMB = kThreads / G;      // qm per workgroup
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int LP = L * P;
    int4* s_off = reinterpret_cast<int4*>(smem);                       // [QMB*LP]
    float4* s_w = reinterpret_cast<float4*>(smem + (size_t)QMB * LP * 16);  // [QMB*LP]
    __shared__ LevelInfo lv;

    const int tile = xcd_tile(ntiles);
    if (tile >= ntiles) return;
    const int tid = threadIdx.x;
    if (tid < L) {
        lv.H[tid] = (int)shapes[2 * tid];
        lv.W[tid] = (int)shapes[2 * tid + 1];
        lv.start[tid] = (int)level_start[tid];
    }
    __syncthreads();

    const int qm0 = tile * QMB;
    const int n_items = min(QMB, total_qm - qm0) * LP;
    const int LqM = Lq * M;

    // ---- phase 1: decode sampling points (coalesced: consecutive threads, consecutive points) --
    for (int it = tid; it < n_items; it += kThreads) {
        const int qml = it / LP;
        const int lp = it - qml * LP;
        const int l = lp / P;
        const int qm = qm0 + qml;
        const int b = qm / LqM;
        const int m = qm % M;
        const int64_t gi = (int64_t)qm0 * LP + it;
        const int H = lv.H[l], W = lv.W[l];
        const float2 xy = reinterpret_cast<const float2*>(loc)[gi];
        const float a = attn[gi];
        const float x = xy.x * (float)W - 0.5f;
        const float y = xy.y * (float)H - 0.5f;
        int4 off = make_int4(-1, -1, -1, -1);
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (y > -1.f && x > -1.f && y < (float)H && x < (float)W) {
            const float yf = floorf(y), xf = floorf(x);
            const int y0 = (int)yf, x0 = (int)xf;
            const float ly = y - yf, lx = x - xf, hy = 1.f - ly, hx = 1.f - lx;
            const int row = ((b * S + lv.start[l]) * M + m) * D;   // element offset of pixel (0,0)
            const int sx = M * D, sy = W * sx;
            const int base = row + y0 * sy + x0 * sx;
            const bool y0v = y0 >= 0, y1v = y0 + 1 <= H - 1, x0v = x0 >= 0, x1v = x0 + 1 <= W - 1;
            if (y0v && x0v) { off.x = base;           w.x = hy * hx * a; }
            if (y0v && x1v) { off.y = base + sx;      w.y = hy * lx * a; }
            if (y1v && x0v) { off.z = base + sy;      w.z = ly * hx * a; }
            if (y1v && x1v) { off.w = base + sy + sx; w.w = ly * lx * a; }
        }
        s_off[it] = off;
        s_w[it] = w;
    }
    __syncthreads();

    // ---- phase 2: gather + accumulate ---------------------------------------------------------
    const int g = tid / G;            // which qm of the tile
    const int j = tid - g * G;        // which V-channel slice
    if (qm0 + g >= total_qm) return;
    float acc[V];
#pragma unroll
    for (int i = 0; i < V; ++i) acc[i] = 0.f;
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(value), 0, value_bytes, 0x00020000);
    const int lane_bytes = j * V * 4;
    const int it0 = g * LP;
#pragma unroll 4
    for (int lp = 0; lp < LP; ++lp) {
        const int4 off = s_off[it0 + lp];
        const float4 w = s_w[it0 + lp];
        float v0[V], v1[V], v2[V], v3[V];
        buf_load(v0, vrs, off.x, lane_bytes);
        buf_load(v1, vrs, off.y, lane_bytes);
        buf_load(v2, vrs, off.z, lane_bytes);
        buf_load(v3, vrs, off.w, lane_bytes);
#pragma unroll
        for (int i = 0; i < V; ++i)
            acc[i] += w.x * v0[i] + w.y * v1[i] + w.z * v2[i] + w.w * v3[i];
    }
    vec_store(out + (int64_t)(qm0 + g) * D + j * V, acc);
}

// --------------------------------------------------------------------------------------------
// Tiled backward, fp32.
// LDS per sampling point: int4 corner offsets, float4 {lx, ly, a, 0}, int2 {W, H};
// results staged per point: float {gA}, float2 {gLoc}.
// --------------------------------------------------------------------------------------------
template <int D, int V>
__global__ __launch_bounds__(kThreads) void msda_bwd_tiled_f32(
    const float* __restrict__ value, const int64_t* __restrict__ shapes,
    const int64_t* __restrict__ level_start, const float* __restrict__ loc,
    const float* __restrict__ attn, const float* __restrict__ grad_out,
    float* __restrict__ grad_value, float* __restrict__ grad_loc, float* __restrict__ grad_attn,
    int S, int M, int L, int Lq, int P, int total_qm, int ntiles)
{
    constexpr int G = D / V;
    constexpr int QMB = kThreads / G;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int LP = L * P;
    const int cap = QMB * LP;
    int4* s_off = reinterpret_cast<int4*>(smem);                              // [cap]
    float4* s_f = reinterpret_cast<float4*>(smem + (size_t)cap * 16);         // [cap] lx,ly,a,-
    float2* s_wh = reinterpret_cast<float2*>(smem + (size_t)cap * 32);        // [cap] W,H (float)
    float2* s_gl = reinterpret_cast<float2*>(smem + (size_t)cap * 40);        // [cap]
    float* s_ga = reinterpret_cast<float*>(smem + (size_t)cap * 48);          // [cap]
    __shared__ LevelInfo lv;

    const int tile = xcd_tile(ntiles);
    if (tile >= ntiles) return;
    const int tid = threadIdx.x;
    if (tid < L) {
        lv.H[tid] = (int)shapes[2 * tid];
        lv.W[tid] = (int)shapes[2 * tid + 1];
        lv.start[tid] = (int)level_start[tid];
    }
    __syncthreads();

    const int qm0 = tile * QMB;
    const int n_items = min(QMB, total_qm - qm0) * LP;
    const int LqM = Lq * M;

    for (int it = tid; it < n_items; it += kThreads) {
        const int qml = it / LP;
        const int lp = it - qml * LP;
        const int l = lp / P;
        const int qm = qm0 + qml;
        const int b = qm / LqM;
        const int m = qm % M;
        const int64_t gi = (int64_t)qm0 * LP + it;
        const float2 xy = reinterpret_cast<const float2*>(loc)[gi];
        const float a = attn[gi];
        const int H = lv.H[l], W = lv.W[l];
        const float x = xy.x * (float)W - 0.5f;
        const float y = xy.y * (float)H - 0.5f;
        int4 off = make_int4(-1, -1, -1, -1);
        float4 f = make_float4(0.f, 0.f, a, 0.f);
        if (y > -1.f && x > -1.f && y < (float)H && x < (float)W) {
            const float yf = floorf(y), xf = floorf(x);
            const int y0 = (int)yf, x0 = (int)xf;
            f.x = x - xf;
            f.y = y - yf;
            const int row = ((b * S + lv.start[l]) * M + m) * D;
            const int sx = M * D, sy = W * sx;
            const int base = row + y0 * sy + x0 * sx;
            const bool y0v = y0 >= 0, y1v = y0 + 1 <= H - 1, x0v = x0 >= 0, x1v = x0 + 1 <= W - 1;
            if (y0v && x0v) off.x = base;
            if (y0v && x1v) off.y = base + sx;
            if (y1v && x0v) off.z = base + sy;
            if (y1v && x1v) off.w = base + sy + sx;
        }
        s_off[it] = off;
        s_f[it] = f;
        s_wh[it] = make_float2((float)W, (float)H);
    }
    __syncthreads();

    const int g = tid / G;
    const int j = tid - g * G;
    const bool active = qm0 + g < total_qm;
    if (active) {
        float go[V];
        vec_load(go, grad_out + (int64_t)(qm0 + g) * D + j * V);
        const float* vbase = value + j * V;
        float* gvbase = grad_value + j * V;
        const int it0 = g * LP;
// (no unroll request: the trip count is data-dependent and hipcc rejects the hint)
        for (int lp = 0; lp < LP; ++lp) {
            const int4 off = s_off[it0 + lp];
            const float4 f = s_f[it0 + lp];
            const float lx = f.x, ly = f.y, a = f.z;
            const float hx = 1.f - lx, hy = 1.f - ly;
            float v0[V], v1[V], v2[V], v3[V];
#pragma unroll
            for (int i = 0; i < V; ++i) { v0[i] = 0.f; v1[i] = 0.f; v2[i] = 0.f; v3[i] = 0.f; }
            if (off.x >= 0) vec_load(v0, vbase + off.x);
            if (off.y >= 0) vec_load(v1, vbase + off.y);
            if (off.z >= 0) vec_load(v2, vbase + off.z);
            if (off.w >= 0) vec_load(v3, vbase + off.w);
            const float w0 = hy * hx, w1 = hy * lx, w2 = ly * hx, w3 = ly * lx;
            float pa = 0.f, px = 0.f, py = 0.f;
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float val = w0 * v0[i] + w1 * v1[i] + w2 * v2[i] + w3 * v3[i];
                const float gh = hx * (v2[i] - v0[i]) + lx * (v3[i] - v1[i]);
                const float gw = hy * (v1[i] - v0[i]) + ly * (v3[i] - v2[i]);
                pa += go[i] * val;
                px += go[i] * gw;
                py += go[i] * gh;
            }
            // scatter-add into grad_value: hardware fp32 atomics (no CAS loop; -munsafe-fp-atomics)
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float ta = go[i] * a;
                if (off.x >= 0) atomicAdd(gvbase + off.x + i, w0 * ta);
                if (off.y >= 0) atomicAdd(gvbase + off.y + i, w1 * ta);
                if (off.z >= 0) atomicAdd(gvbase + off.z + i, w2 * ta);
                if (off.w >= 0) atomicAdd(gvbase + off.w + i, w3 * ta);
            }
            pa = group_sum<G>(pa);
            px = group_sum<G>(px);
            py = group_sum<G>(py);
            if (j == 0) {
                const float2 wh = s_wh[it0 + lp];
                s_ga[it0 + lp] = pa;
                s_gl[it0 + lp] = make_float2(wh.x * a * px, wh.y * a * py);
            }
        }
    }
    __syncthreads();
    // coalesced write-out of the per-point gradients
    for (int it = tid; it < n_items; it += kThreads) {
        const int64_t gi = (int64_t)qm0 * LP + it;
        grad_attn[gi] = s_ga[it];
        reinterpret_cast<float2*>(grad_loc)[gi] = s_gl[it];
    }
}

// --------------------------------------------------------------------------------------------
// Generic kernels: any D, fp32 / fp64, 64-bit indexing.  Correctness path.
// --------------------------------------------------------------------------------------------
template <typename T>
struct Sample {
    bool in_range;
    int64_t o[4];   // element offsets (without channel) of the 4 corners, -1 if outside
    T lx, ly;
};

template <typename T>
__device__ __forceinline__ Sample<T> decode(const T* loc, int64_t gi, int H, int W, int64_t row0,
                                            int M, int D)
{
    Sample<T> s;
    const T x = loc[2 * gi] * (T)W - (T)0.5;
    const T y = loc[2 * gi + 1] * (T)H - (T)0.5;
    s.in_range = (y > (T)-1 && x > (T)-1 && y < (T)H && x < (T)W);
    s.o[0] = s.o[1] = s.o[2] = s.o[3] = -1;
    s.lx = 0; s.ly = 0;
    if (s.in_range) {
        const T yf = floor(y), xf = floor(x);
        const int y0 = (int)yf, x0 = (int)xf;
        s.ly = y - yf; s.lx = x - xf;
        const int64_t sx = (int64_t)M * D, sy = (int64_t)W * sx;
        const int64_t base = row0 + y0 * sy + x0 * sx;
        const bool y0v = y0 >= 0, y1v = y0 + 1 <= H - 1, x0v = x0 >= 0, x1v = x0 + 1 <= W - 1;
        if (y0v && x0v) s.o[0] = base;
        if (y0v && x1v) s.o[1] = base + sx;
        if (y1v && x0v) s.o[2] = base + sy;
        if (y1v && x1v) s.o[3] = base + sy + sx;
    }
    return s;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void msda_fwd_generic(
    const T* __restrict__ value, const int64_t* __restrict__ shapes,
    const int64_t* __restrict__ level_start, const T* __restrict__ loc,
    const T* __restrict__ attn, T* __restrict__ out,
    int S, int M, int D, int L, int Lq, int P, int64_t total)
{
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * kThreads) {
        const int c = (int)(idx % D);
        const int64_t qm = idx / D;
        const int m = (int)(qm % M);
        const int64_t b = qm / ((int64_t)Lq * M);
        T acc = 0;
        for (int l = 0; l < L; ++l) {
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
            const int64_t row0 = ((b * S + level_start[l]) * M + m) * D;
            for (int p = 0; p < P; ++p) {
                const int64_t gi = (qm * L + l) * P + p;
                const Sample<T> s = decode<T>(loc, gi, H, W, row0, M, D);
                if (!s.in_range) continue;
                const T hx = (T)1 - s.lx, hy = (T)1 - s.ly;
                T val = 0;
                if (s.o[0] >= 0) val += hy * hx * value[s.o[0] + c];
                if (s.o[1] >= 0) val += hy * s.lx * value[s.o[1] + c];
                if (s.o[2] >= 0) val += s.ly * hx * value[s.o[2] + c];
                if (s.o[3] >= 0) val += s.ly * s.lx * value[s.o[3] + c];
                acc += attn[gi] * val;
            }
        }
        out[idx] = acc;
    }
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave per (b,q,m); lanes stride over channels; per-point wave reduction
template <typename T>
__global__ __launch_bounds__(kThreads) void msda_bwd_generic(
    const T* __restrict__ value, const int64_t* __restrict__ shapes,
    const int64_t* __restrict__ level_start, const T* __restrict__ loc,
    const T* __restrict__ attn, const T* __restrict__ grad_out,
    T* __restrict__ grad_value, T* __restrict__ grad_loc, T* __restrict__ grad_attn,
    int S, int M, int D, int L, int Lq, int P, int64_t total_qm)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    constexpr int kWaves = kThreads / 64;
    for (int64_t qm = (int64_t)blockIdx.x * kWaves + wave; qm < total_qm;
         qm += (int64_t)gridDim.x * kWaves) {
        const int m = (int)(qm % M);
        const int64_t b = qm / ((int64_t)Lq * M);
        const T* go = grad_out + qm * D;
        for (int l = 0; l < L; ++l) {
            const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
            const int64_t row0 = ((b * S + level_start[l]) * M + m) * D;
            for (int p = 0; p < P; ++p) {
                const int64_t gi = (qm * L + l) * P + p;
                const Sample<T> s = decode<T>(loc, gi, H, W, row0, M, D);
                T pa = 0, px = 0, py = 0;
                const T a = attn[gi];
                if (s.in_range) {
                    const T lx = s.lx, ly = s.ly, hx = (T)1 - lx, hy = (T)1 - ly;
                    const T w0 = hy * hx, w1 = hy * lx, w2 = ly * hx, w3 = ly * lx;
                    for (int c = lane; c < D; c += 64) {
                        const T v0 = s.o[0] >= 0 ? value[s.o[0] + c] : (T)0;
                        const T v1 = s.o[1] >= 0 ? value[s.o[1] + c] : (T)0;
                        const T v2 = s.o[2] >= 0 ? value[s.o[2] + c] : (T)0;
                        const T v3 = s.o[3] >= 0 ? value[s.o[3] + c] : (T)0;
                        const T gc = go[c];
                        const T ta = gc * a;
                        pa += gc * (w0 * v0 + w1 * v1 + w2 * v2 + w3 * v3);
                        px += gc * (hy * (v1 - v0) + ly * (v3 - v2));
                        py += gc * (hx * (v2 - v0) + lx * (v3 - v1));
                        if (s.o[0] >= 0) atomicAdd(grad_value + s.o[0] + c, w0 * ta);
                        if (s.o[1] >= 0) atomicAdd(grad_value + s.o[1] + c, w1 * ta);
                        if (s.o[2] >= 0) atomicAdd(grad_value + s.o[2] + c, w2 * ta);
                        if (s.o[3] >= 0) atomicAdd(grad_value + s.o[3] + c, w3 * ta);
                    }
                }
                pa = wave_sum(pa);
                px = wave_sum(px);
                py = wave_sum(py);
                if (lane == 0) {
                    grad_attn[gi] = pa;
                    grad_loc[2 * gi] = (T)W * a * px;
                    grad_loc[2 * gi + 1] = (T)H * a * py;
                }
            }
        }
    }
}

// process-wide options (benchmarks / tests)
int g_fwd_variant = 0;
int g_bwd_variant = 0;

// launch size of a tiled kernel: kThreads / (32 / V) (query, head) pairs per workgroup, `per_point` LDS bytes per sample
struct TiledSize { int total_qm, ntiles, grid; size_t lds; };
template <int V>
TiledSize tiled_size(const MsdaProblem& p, int per_point)
{
    constexpr int QMB = kThreads / (32 / V);
    const int total_qm = p.N * p.Lq * p.M, ntiles = (total_qm + QMB - 1) / QMB;
    return {total_qm, ntiles, ((ntiles + 7) / 8) * 8, (size_t)QMB * p.L * p.P * per_point};
}

}  // namespace

namespace mpf {
int set_msda_option(const char* key, int v)
{
    const bool mine = !strcmp(key, "msda_fwd_variant") || !strcmp(key, "msda_bwd_variant");
    if (!mine) return 1;
    if (v < 0 || v > 4) return MPF_E_SHAPE;
    if (!strcmp(key, "msda_fwd_variant")) g_fwd_variant = v; else g_bwd_variant = v;
    return 0;
}
}  // namespace mpf

// Module-level op, front part (ops/modules/ms_deform_attn.py:103-117): from the raw projection outputs
// raw[row, M*L*P*2 offsets | M*L*P logits] and the reference points ref[q, 2] (valid_ratios == 1: the same
// point for every level) produce attn = softmax over the L*P logits of (q, m) and loc = ref + offset /
// (W_l, H_l) in one pass — one launch instead of softmax + div + add.
// (Deriving them inside the gather kernel's decode phase was slower: +47 us on the gather kernel for
// 59 us of element-wise kernels removed; this kernel costs ~25 us.)
namespace {
// one thread per sampling point (coalesced reads of the offsets / writes of loc, attn); the L*P logits of
// a (row, head) group go through LDS for the softmax; a workgroup takes kThreads / LP whole groups
__global__ __launch_bounds__(kThreads) void msda_prep_kernel(const float* __restrict__ raw, const float* __restrict__ ref,
                                                             const int64_t* __restrict__ shapes, float* __restrict__ loc,
                                                             float* __restrict__ attn, int groups, int M, int L, int Lq, int P)
{
    __shared__ float s_lg[kThreads];
    const int LP = L * P;
    const int gpb = kThreads / LP;                              // groups per workgroup
    const int gl = threadIdx.x / LP, lp = threadIdx.x - gl * LP;
    const int grp = blockIdx.x * gpb + gl;                      // (row, head)
    const bool ok = gl < gpb && grp < groups;
    const int row = ok ? grp / M : 0, m = ok ? grp - row * M : 0;
    const float* r = raw + (int64_t)row * (M * LP * 3);
    if (ok) s_lg[threadIdx.x] = r[M * LP * 2 + m * LP + lp];
    __syncthreads();
    if (!ok) return;
    float mx = -3.0e38f;
    for (int j = 0; j < LP; ++j) mx = fmaxf(mx, s_lg[gl * LP + j]);
    float sum = 0.f;
    for (int j = 0; j < LP; ++j) sum += expf(s_lg[gl * LP + j] - mx);
    const int l = lp / P;
    const float W = (float)shapes[2 * l + 1], H = (float)shapes[2 * l];
    const float2 o = reinterpret_cast<const float2*>(r + m * LP * 2)[lp];
    const float2 rp = reinterpret_cast<const float2*>(ref)[row % Lq];
    const int64_t gi = (int64_t)grp * LP + lp;
    attn[gi] = expf(s_lg[threadIdx.x] - mx) / sum;
    reinterpret_cast<float2*>(loc)[gi] = make_float2(rp.x + o.x / W, rp.y + o.y / H);
}

template <typename T>
hipError_t launch_fwd_generic(const MsdaProblem& p, const MsdaOperands& o)
{
    const int64_t total = p.n_rows(), want = (total + kThreads - 1) / kThreads;
    const int grid = (int)(want < 65536 * 8 ? want : 65536 * 8);
    hipLaunchKernelGGL(msda_fwd_generic<T>, dim3(grid), dim3(kThreads), 0, o.stream, (const T*)o.value, o.shapes, o.lsi, (const T*)o.loc,
                       (const T*)o.attn, (T*)o.out, p.S, p.M, p.D, p.L, p.Lq, p.P, total);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_bwd_generic(const MsdaProblem& p, const MsdaOperands& o)
{
    const int64_t total_qm = (int64_t)p.N * p.Lq * p.M, want = (total_qm + 3) / 4;
    const int grid = (int)(want < 65536 * 8 ? want : 65536 * 8);
    hipLaunchKernelGGL(msda_bwd_generic<T>, dim3(grid), dim3(kThreads), 0, o.stream, (const T*)o.value, o.shapes, o.lsi, (const T*)o.loc,
                       (const T*)o.attn, (const T*)o.grad_out, (T*)o.grad_value, (T*)o.grad_loc, (T*)o.grad_attn, p.S, p.M, p.D, p.L, p.Lq,
                       p.P, total_qm);
    return hipGetLastError();
}
}  // namespace

namespace mpf {
int msda_fwd_variant() { return g_fwd_variant; }
int msda_bwd_variant() { return g_bwd_variant; }

// the tiled kernels use 32-bit element offsets and need a 16-byte aligned row
bool msda_tiled_ok(const MsdaProblem& p, int V)
{
    if (p.dtype != MPF_F32 || p.D != 32) return false;
    if (p.n_value() * 4 >= (1ll << 31) || p.n_samples() * 2 >= (1ll << 31)) return false;   // value bytes < 2 GiB: byte offsets in buffer loads
    const size_t lds = (size_t)(kThreads / (p.D / V)) * p.L * p.P * 52;
    return lds <= 64 * 1024;
}

// loc / attn of the raw forward from the projection output and the reference points
void msda_launch_prep(const MsdaProblem& p, const MsdaOperands& o)
{
    const int groups = p.N * p.Lq * p.M, gpb = kThreads / (p.L * p.P);
    set_kernel("msda_prep_kernel");
    hipLaunchKernelGGL(msda_prep_kernel, dim3((groups + gpb - 1) / gpb), dim3(kThreads), 0, o.stream, (const float*)o.raw,
                       (const float*)o.ref, o.shapes, (float*)const_cast<void*>(o.loc), (float*)const_cast<void*>(o.attn), groups, p.M, p.L,
                       p.Lq, p.P);
}

int msda_launch_forward(const MsdaProblem& p, const MsdaOperands& o, int V, const char* who)
{
    hipError_t err = hipSuccess;
    prof_begin(o.stream);
    static const char* const kTiled[5] = {nullptr, "msda_fwd_tiled_f32<32,1>", "msda_fwd_tiled_f32<32,2>", nullptr, "msda_fwd_tiled_f32<32,4>"};
    set_kernel(V ? kTiled[V] : p.dtype == MPF_F32 ? "msda_fwd_generic<float>" : "msda_fwd_generic<double>");
    if (V)
        with_int_of<1, 2, 4>(V, [&](auto v) {
            const TiledSize t = tiled_size<decltype(v)::value>(p, 32);
            hipLaunchKernelGGL((msda_fwd_tiled_f32<32, decltype(v)::value>), dim3(t.grid), dim3(kThreads), t.lds, o.stream, (const float*)o.value,
                               o.shapes, o.lsi, (const float*)o.loc, (const float*)o.attn, (float*)o.out, p.S, p.M, p.L, p.Lq, p.P, t.total_qm,
                               t.ntiles, (unsigned)((size_t)p.n_value() * 4));
            err = hipGetLastError();
        });
    else
        err = p.dtype == MPF_F32 ? launch_fwd_generic<float>(p, o) : launch_fwd_generic<double>(p, o);
    prof_end(mpf_last_kernel(), o.stream, p.forward_bytes());
    return check(err, who);
}

int msda_launch_backward(const MsdaProblem& p, const MsdaOperands& o, int V)
{
    hipError_t err = hipMemsetAsync(o.grad_value, 0, (size_t)p.n_value() * p.esz(), o.stream);
    if (err != hipSuccess) return check(err, "mpf_msda_backward(memset)");
    prof_begin(o.stream);
    static const char* const kTiled[5] = {nullptr, "msda_bwd_tiled_f32<32,1>", "msda_bwd_tiled_f32<32,2>", nullptr, "msda_bwd_tiled_f32<32,4>"};
    set_kernel(V ? kTiled[V] : p.dtype == MPF_F32 ? "msda_bwd_generic<float>" : "msda_bwd_generic<double>");
    if (V)
        with_int_of<1, 2, 4>(V, [&](auto v) {
            const TiledSize t = tiled_size<decltype(v)::value>(p, 52);
            hipLaunchKernelGGL((msda_bwd_tiled_f32<32, decltype(v)::value>), dim3(t.grid), dim3(kThreads), t.lds, o.stream, (const float*)o.value,
                               o.shapes, o.lsi, (const float*)o.loc, (const float*)o.attn, (const float*)o.grad_out, (float*)o.grad_value,
                               (float*)o.grad_loc, (float*)o.grad_attn, p.S, p.M, p.L, p.Lq, p.P, t.total_qm, t.ntiles);
            err = hipGetLastError();
        });
    else
        err = p.dtype == MPF_F32 ? launch_bwd_generic<float>(p, o) : launch_bwd_generic<double>(p, o);
    prof_end(mpf_last_kernel(), o.stream, p.backward_bytes());
    return check(err, "mpf_msda_backward");
}
}  // namespace mpf

