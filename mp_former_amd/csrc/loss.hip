// Point-sampled mask loss kernels (matcher cost sampling, importance sampling, BCE + dice sums and
// their backward) for MI355X.
//
// Reference semantics: detectron2 point_sample(x, c) = grid_sample(x, 2c-1, bilinear, zeros,
// align_corners=False), used at mask2former/modeling/criterion.py:164-182 (loss) and
// mask2former/modeling/matcher.py:122-132 (matching cost); sigmoid_ce_loss / dice_loss at
// criterion.py:21-65.
//
// The reference materialises, per loss call: a gathered copy of the matched prediction maps, a
// float copy of the full-resolution ground-truth masks, three grid_sample outputs, and the
// element-wise BCE / sigmoid tensors.  Here one kernel reads the prediction map (f32 or bf16) and
// the BYTE ground-truth mask directly at the sampled corners and emits four sums per (prediction,
// target) pair; the backward scatters d(loss)/d(logit) to the four corners with fp32 atomics.
// All of it is HBM/L2-latency bound gather work: one thread per point, coalesced coordinate reads.
//
// The kernels come first, then the ten entry points on loss_host.h: an entry fills one LossProblem, runs loss_check, asks the route
// function which kernel serves it, names that kernel and launches it, once per argument list (with_map_type and mpf::with_bool choose
// the element type and the byte / bit form of the masks), and through launch_lds where the kernel takes dynamic LDS.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "loss_host.h"

namespace {

__device__ __forceinline__ float ld(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float ld(const __hip_bfloat16* p, int64_t i) { return __bfloat162float(p[i]); }
__device__ __forceinline__ float ld(const uint8_t* p, int64_t i) { return p[i] ? 1.f : 0.f; }

// ground-truth masks packed 32 pixels per word (mpf_pack_mask_bits): 1 MiB -> 128 KiB per 1024^2 mask,
// so a step's masks stay L2-resident under the random bilinear gathers of the loss kernels
struct BitPlane {
    const uint32_t* words;      // base of ALL planes
    int64_t first;              // pixel index of this plane's (0, 0)
};
__device__ __forceinline__ float ld(const BitPlane& m, int64_t i)
{
    const int64_t j = m.first + i;
    return ((m.words[j >> 5] >> (unsigned)(j & 31)) & 1u) ? 1.f : 0.f;
}

struct Bilin {
    int x0, y0;
    float lx, ly;
};

// align_corners=False: pixel coordinate = c * size - 0.5
__device__ __forceinline__ Bilin bilin(float cx, float cy, int h, int w)
{
    const float x = cx * (float)w - 0.5f, y = cy * (float)h - 0.5f;
    const float xf = floorf(x), yf = floorf(y);
    Bilin b;
    b.x0 = (int)xf; b.y0 = (int)yf; b.lx = x - xf; b.ly = y - yf;
    return b;
}

// the four corner loads are UNCONDITIONAL (indices clamped into the plane, out-of-range corners zeroed
// afterwards): a load behind a run-time condition makes hipcc branch around it and wait for it separately,
// i.e. four dependent round trips per sample instead of four loads in flight
template <typename MAP>
__device__ __forceinline__ float sample(const MAP map, int h, int w, const Bilin& b)
{
    const bool x0v = b.x0 >= 0 && b.x0 < w, x1v = b.x0 + 1 >= 0 && b.x0 + 1 < w;
    const bool y0v = b.y0 >= 0 && b.y0 < h, y1v = b.y0 + 1 >= 0 && b.y0 + 1 < h;
    const int xa = min(max(b.x0, 0), w - 1), xb = min(max(b.x0 + 1, 0), w - 1);
    const int64_t ra = (int64_t)min(max(b.y0, 0), h - 1) * w, rb = (int64_t)min(max(b.y0 + 1, 0), h - 1) * w;
    const float l00 = ld(map, ra + xa), l01 = ld(map, ra + xb), l10 = ld(map, rb + xa), l11 = ld(map, rb + xb);
    const float v00 = (y0v && x0v) ? l00 : 0.f, v01 = (y0v && x1v) ? l01 : 0.f;
    const float v10 = (y1v && x0v) ? l10 : 0.f, v11 = (y1v && x1v) ? l11 : 0.f;
    const float hx = 1.f - b.lx, hy = 1.f - b.ly;
    return hy * (hx * v00 + b.lx * v01) + b.ly * (hx * v10 + b.lx * v11);
}

// the ground-truth plane of row r as a sampling source: byte mask or bit-packed
template <bool BITS>
struct GtPlane;
template <>
struct GtPlane<false> {
    const uint8_t* p;
    __device__ __forceinline__ GtPlane(const void* gt, int64_t row, int H, int W) : p((const uint8_t*)gt + row * H * W) {}
    __device__ __forceinline__ float at(int H, int W, const Bilin& b) const { return sample(p, H, W, b); }
};
template <>
struct GtPlane<true> {
    BitPlane p;
    __device__ __forceinline__ GtPlane(const void* gt, int64_t row, int H, int W) : p{(const uint32_t*)gt, row * H * W} {}
    __device__ __forceinline__ float at(int H, int W, const Bilin& b) const { return sample(p, H, W, b); }
};

// bits[i] = 32 consecutive pixels of the byte masks (pixel count a multiple of 32)
__global__ __launch_bounds__(kThreads) void pack_mask_bits_kernel(const uint8_t* __restrict__ m, uint32_t* __restrict__ bits, int64_t nwords)
{
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < nwords; i += (int64_t)gridDim.x * kThreads) {
        const uint4 a = reinterpret_cast<const uint4*>(m)[2 * i], b = reinterpret_cast<const uint4*>(m)[2 * i + 1];
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        uint32_t o = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) o |= (((w[k] >> (8 * j)) & 0xFFu) ? 1u : 0u) << (4 * k + j);
        bits[i] = o;
    }
}

// out[i, p] = bilinear(bit plane offs[i] (pixel index), coords[coord_rows ? coord_rows[i] : i, p])
__global__ __launch_bounds__(kThreads) void point_sample_bits_kernel(
    const uint32_t* __restrict__ src, int h, int w, const int64_t* __restrict__ offs,
    const float* __restrict__ coords, const int32_t* __restrict__ coord_rows, float* __restrict__ out, int n, int P)
{
    const int i = blockIdx.y;
    const BitPlane map{src, offs[i]};
    const float2* c = reinterpret_cast<const float2*>(coords) + (int64_t)(coord_rows ? coord_rows[i] : i) * P;
    for (int p = blockIdx.x * kThreads + threadIdx.x; p < P; p += gridDim.x * kThreads) {
        const float2 xy = c[p];
        out[(int64_t)i * P + p] = sample(map, h, w, bilin(xy.x, xy.y, h, w));
    }
}

// out[i, p] = bilinear(map at src + offs[i], coords[coord_rows ? coord_rows[i] : i, p])
template <typename T>
__global__ __launch_bounds__(kThreads) void point_sample_kernel(
    const T* __restrict__ src, int h, int w, const int64_t* __restrict__ offs,
    const float* __restrict__ coords, const int32_t* __restrict__ coord_rows, float* __restrict__ out, int n, int P)
{
    const int i = blockIdx.y;
    const T* map = src + offs[i];
    const float2* c = reinterpret_cast<const float2*>(coords) + (int64_t)(coord_rows ? coord_rows[i] : i) * P;
    for (int p = blockIdx.x * kThreads + threadIdx.x; p < P; p += gridDim.x * kThreads) {
        const float2 xy = c[p];
        out[(int64_t)i * P + p] = sample(map, h, w, bilin(xy.x, xy.y, h, w));
    }
}

__device__ __forceinline__ float block_sum(float v, float* red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < kThreads / 64; ++k) s += red[k];
    return s;
}

// partial[i, chunk, 0..3] = sum over the chunk's points of {bce(x,t), sigmoid(x)*t, sigmoid(x), t}
template <typename T, bool BITS>
__global__ __launch_bounds__(kThreads) void mask_loss_fwd_kernel(
    const T* __restrict__ pred, int h, int w, const int64_t* __restrict__ pred_offs,
    const void* __restrict__ gt, int H, int W, const int32_t* __restrict__ gt_rows,
    const float* __restrict__ coords, float* __restrict__ partial, int n, int P, int chunks)
{
    __shared__ float red[kThreads / 64];
    const int i = blockIdx.y, ch = blockIdx.x;
    const T* pm = pred + pred_offs[i];
    const GtPlane<BITS> gm(gt, gt_rows[i], H, W);
    const float2* c = reinterpret_cast<const float2*>(coords) + (int64_t)i * P;
    const int per = (P + chunks - 1) / chunks;
    const int p0 = ch * per, p1 = min(P, p0 + per);
    float s_bce = 0.f, s_pt = 0.f, s_p = 0.f, s_t = 0.f;
    for (int p = p0 + threadIdx.x; p < p1; p += kThreads) {
        const float2 xy = c[p];
        const float x = sample(pm, h, w, bilin(xy.x, xy.y, h, w));
        const float t = gm.at(H, W, bilin(xy.x, xy.y, H, W));
        const float sg = 1.f / (1.f + __expf(-x));
        s_bce += fmaxf(x, 0.f) - x * t + log1pf(__expf(-fabsf(x)));   // BCE-with-logits, stable form
        s_pt += sg * t;
        s_p += sg;
        s_t += t;
    }
    s_bce = block_sum(s_bce, red);
    s_pt = block_sum(s_pt, red);
    s_p = block_sum(s_p, red);
    s_t = block_sum(s_t, red);
    if (threadIdx.x == 0) {
        float* o = partial + ((int64_t)i * chunks + ch) * 4;
        o[0] = s_bce; o[1] = s_pt; o[2] = s_p; o[3] = s_t;
    }
}

// grad map (fp32, at grad_pred + grad_offs[i]) += d/dx of  g[i,0]*bce + g[i,1]*sum(s*t) + g[i,2]*sum(s)
template <typename T>
__global__ __launch_bounds__(kThreads) void mask_loss_bwd_kernel(
    const T* __restrict__ pred, int h, int w, const int64_t* __restrict__ pred_offs,
    const uint8_t* __restrict__ gt, int H, int W, const int32_t* __restrict__ gt_rows,
    const float* __restrict__ coords, const float* __restrict__ gsum, float* __restrict__ grad_pred,
    const int64_t* __restrict__ grad_offs, int n, int P)
{
    const int i = blockIdx.y;
    const T* pm = pred + pred_offs[i];
    float* gp = grad_pred + grad_offs[i];
    const uint8_t* gm = gt + (int64_t)gt_rows[i] * H * W;
    const float2* c = reinterpret_cast<const float2*>(coords) + (int64_t)i * P;
    const float g_bce = gsum[4 * i], g_pt = gsum[4 * i + 1], g_p = gsum[4 * i + 2];
    for (int p = blockIdx.x * kThreads + threadIdx.x; p < P; p += gridDim.x * kThreads) {
        const float2 xy = c[p];
        const Bilin b = bilin(xy.x, xy.y, h, w);
        const float x = sample(pm, h, w, b);
        const float t = sample(gm, H, W, bilin(xy.x, xy.y, H, W));
        const float sg = 1.f / (1.f + __expf(-x));
        const float dx = g_bce * (sg - t) + (g_pt * t + g_p) * sg * (1.f - sg);
        const bool x0v = b.x0 >= 0 && b.x0 < w, x1v = b.x0 + 1 >= 0 && b.x0 + 1 < w;
        const bool y0v = b.y0 >= 0 && b.y0 < h, y1v = b.y0 + 1 >= 0 && b.y0 + 1 < h;
        const int64_t o = (int64_t)b.y0 * w + b.x0;
        const float hx = 1.f - b.lx, hy = 1.f - b.ly;
        if (y0v && x0v) atomicAdd(gp + o, dx * hy * hx);
        if (y0v && x1v) atomicAdd(gp + o + 1, dx * hy * b.lx);
        if (y1v && x0v) atomicAdd(gp + o + w, dx * b.ly * hx);
        if (y1v && x1v) atomicAdd(gp + o + w + 1, dx * b.ly * b.lx);
    }
}

// ------------------------------------------------------------------------------------------------
// Backward without global atomics: one workgroup per (pair, horizontal band of the prediction plane).
// The band lives in LDS as 32-bit FIXED-POINT accumulators (per-lane LDS integer atomics run >10x
// faster than fp32 LDS or global atomics on this chip, tools/ubench/lds_atomics.hip, and make the sum
// order-independent = deterministic); every point of the pair whose bilinear footprint touches the
// band is re-evaluated and scattered into it; the band is then written ONCE, converted to the
// gradient dtype, to its place in the dense gradient of the prediction maps.  Scale: |d loss/d x| <=
// B = |g_bce| + (|g_pt| + |g_p|)/4 per point, so 2^31 / (256 B) leaves room for 256 full-magnitude
// hits on one pixel at a resolution of B * 2^-23 (fp32-grade).
// ------------------------------------------------------------------------------------------------
template <typename T, typename TG, bool BITS>
__global__ __launch_bounds__(1024) void mask_loss_bwd_band_kernel(
    const T* __restrict__ pred, int h, int w, const int64_t* __restrict__ pred_offs,
    const void* __restrict__ gt, int H, int W, const int32_t* __restrict__ gt_rows,
    const float* __restrict__ coords, const float* __restrict__ gsum, TG* __restrict__ grad,
    const int64_t* __restrict__ grad_offs, int n, int P, int band_rows)
{
    extern __shared__ int band[];
    const int i = blockIdx.y;
    const int y_lo = blockIdx.x * band_rows, y_hi = min(h, y_lo + band_rows);
    const int cells = (y_hi - y_lo) * w;
    for (int k = threadIdx.x; k < cells; k += 1024) band[k] = 0;
    const T* pm = pred + pred_offs[i];
    const GtPlane<BITS> gm(gt, gt_rows[i], H, W);
    const float2* c = reinterpret_cast<const float2*>(coords) + (int64_t)i * P;
    const float g_bce = gsum[4 * i], g_pt = gsum[4 * i + 1], g_p = gsum[4 * i + 2];
    const float B = fabsf(g_bce) + 0.25f * (fabsf(g_pt) + fabsf(g_p));
    const float scale = B > 0.f ? 8388608.f / B : 0.f;             // 2^23 / B
    const float inv = B > 0.f ? B * (1.f / 8388608.f) : 0.f;
    __syncthreads();
    if (B > 0.f) {
        for (int p = threadIdx.x; p < P; p += 1024) {
            const float2 xy = c[p];
            const Bilin b = bilin(xy.x, xy.y, h, w);
            if (b.y0 + 1 < y_lo || b.y0 >= y_hi) continue;       // footprint rows y0, y0+1 miss the band
            const float x = sample(pm, h, w, b);
            const float t = gm.at(H, W, bilin(xy.x, xy.y, H, W));
            const float sg = 1.f / (1.f + __expf(-x));
            const float dx = (g_bce * (sg - t) + (g_pt * t + g_p) * sg * (1.f - sg)) * scale;
            const bool x0v = b.x0 >= 0 && b.x0 < w, x1v = b.x0 + 1 >= 0 && b.x0 + 1 < w;
            const bool y0v = b.y0 >= y_lo && b.y0 < y_hi, y1v = b.y0 + 1 >= y_lo && b.y0 + 1 < y_hi;
            const int o = (b.y0 - y_lo) * w + b.x0;
            const float hx = 1.f - b.lx, hy = 1.f - b.ly;
            if (y0v && x0v) atomicAdd(&band[o], __float2int_rn(dx * hy * hx));
            if (y0v && x1v) atomicAdd(&band[o + 1], __float2int_rn(dx * hy * b.lx));
            if (y1v && x0v) atomicAdd(&band[o + w], __float2int_rn(dx * b.ly * hx));
            if (y1v && x1v) atomicAdd(&band[o + w + 1], __float2int_rn(dx * b.ly * b.lx));
        }
    }
    __syncthreads();
    TG* dst = grad + grad_offs[i] + (int64_t)y_lo * w;
    for (int k = threadIdx.x; k < cells; k += 1024) dst[k] = (TG)((float)band[k] * inv);
}

// ================================================================================================
// Importance selection: per row keep the k points with the SMALLEST |logit| (= the most uncertain,
// uncertainty = -|logit|, criterion.py:73-87 + detectron2 get_uncertain_point_coords_with_randomness)
// and emit their coordinates.  MSB-first 8-bit radix select on the bit pattern of |x| (monotonic for
// non-negative floats) with an LDS histogram, then an order-preserving compaction — replaces
// torch.topk (a full sort of 37632 keys per row) + gather.
// ================================================================================================
__device__ __forceinline__ int block_excl_scan_1024(int v, int* red, int* total)
{
    // exclusive scan of one int per thread over 1024 threads (16 waves)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    __syncthreads();
    if (lane == 63) red[wave] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kSelThreads / 64; ++k) {
        const int r = red[k];
        if (k < wave) base += r;
        tot += r;
    }
    *total = tot;
    return base + incl - v;
}

__global__ __launch_bounds__(kSelThreads) void select_uncertain_kernel(
    const float* __restrict__ vals, const float* __restrict__ coords_in, float* __restrict__ coords_out,
    int M, int k, int P_out)
{
    __shared__ int hist[256];
    __shared__ int red[kSelThreads / 64];
    __shared__ unsigned s_prefix;
    __shared__ int s_krem;
    const int row = blockIdx.x;
    const float* v = vals + (int64_t)row * M;
    const float2* cin = reinterpret_cast<const float2*>(coords_in) + (int64_t)row * M;
    float2* cout = reinterpret_cast<float2*>(coords_out) + (int64_t)row * P_out;
    const int tid = threadIdx.x;
    if (tid == 0) { s_prefix = 0u; s_krem = k; }
    unsigned prefix = 0u, mask = 0u;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        prefix = s_prefix;
        for (int i = tid; i < M; i += kSelThreads) {
            const unsigned key = __float_as_uint(fabsf(v[i]));
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int krem = s_krem, d = 0;
            for (; d < 256; ++d) {
                const int c = hist[d];
                if (krem <= c) break;
                krem -= c;
            }
            if (d > 255) d = 255;
            s_krem = krem;                       // how many of the threshold digit's bucket are needed
            s_prefix = prefix | ((unsigned)d << shift);
        }
        mask |= 255u << shift;
        __syncthreads();
    }
    const unsigned thr = s_prefix;               // exact k-th smallest key
    const int need_eq = s_krem;                  // number of == thr elements to take
    // order-preserving compaction: contiguous slices per thread
    const int per = (M + kSelThreads - 1) / kSelThreads;
    const int i0 = tid * per, i1 = min(M, i0 + per);
    int n_less = 0, n_eq = 0;
    for (int i = i0; i < i1; ++i) {
        const unsigned key = __float_as_uint(fabsf(v[i]));
        n_less += key < thr;
        n_eq += key == thr;
    }
    int tot_less, tot_eq;
    const int off_less = block_excl_scan_1024(n_less, red, &tot_less);
    const int off_eq = block_excl_scan_1024(n_eq, red, &tot_eq);
    int pl = off_less, pe = off_eq;
    for (int i = i0; i < i1; ++i) {
        const unsigned key = __float_as_uint(fabsf(v[i]));
        if (key < thr) {
            cout[pl++] = cin[i];
        } else if (key == thr) {
            if (pe < need_eq) cout[tot_less + pe] = cin[i];
            ++pe;
        }
    }
}

// ================================================================================================
// Matching cost (matcher.py:105-148, mask + dice part): for every (layer, image, query) row and every
// ground-truth mask t of that image,
//   cost[row, t] = w_mask * (sum_p softplus(x_p) - sum_p x_p t_p) / P
//                + w_dice * (1 - (2 sum_p s_p t_p + 1) / (sum_p s_p + sum_p t_p + 1))
// x sampled on the fly from the prediction map, t from the pre-sampled [.., P] ground-truth points.
// One workgroup per row; TT targets at a time in registers.
//
// CLIP (mpf_match_cost_clip, mask2former_video/modeling/matcher.py:113-141): a row is a tube of gridDim.y frames whose planes lie
// stride_f elements apart and a target row holds gridDim.y * P samples, frame-major; the point set is the same in every frame.
// All five sums are additive over the frames, so workgroup (row, f) does exactly the work of the image form on frame f and,
// instead of the cost, leaves its sums in partial[row][f][2 + 3 Tmax] = {softplus, sigmoid, then (x t, s t, t) per target};
// match_cost_clip_fold_kernel adds the frames in order and applies the two formulas.  No atomics: bit-identical run to run.
// ================================================================================================
constexpr int kTT = 8;

template <typename T, bool CLIP>
__global__ __launch_bounds__(kThreads) void match_cost_kernel(
    const T* __restrict__ pred, int h, int w, const int64_t* __restrict__ pred_offs,
    const float* __restrict__ coords, const int32_t* __restrict__ coord_rows,
    const float* __restrict__ tsamp, const int32_t* __restrict__ t_first, const int32_t* __restrict__ t_count,
    float* __restrict__ cost, int Tmax, int P, float w_mask, float w_dice, int64_t stride_f, float* __restrict__ partial)
{
    extern __shared__ float xs[];                    // [P] sampled logits of this row's frame (gathered ONCE)
    __shared__ float red[kThreads / 64];
    const int row = blockIdx.x;
    const int f = CLIP ? blockIdx.y : 0, F = CLIP ? gridDim.y : 1;
    const int Tn = t_count[row];
    if (Tn == 0) return;
    const T* pm = pred + pred_offs[row] + f * stride_f;
    const float2* c = reinterpret_cast<const float2*>(coords) + (int64_t)coord_rows[row] * P;
    const int T0 = t_first[row];
    const int64_t t_len = (int64_t)F * P;              // floats per target row
    const float* ts = tsamp + (int64_t)f * P;
    float* out = CLIP ? partial + ((int64_t)row * F + f) * clip_partial_floats(Tmax) : cost + (int64_t)row * Tmax;
    float sp = 0.f, sg_sum = 0.f;
    for (int p = threadIdx.x; p < P; p += kThreads) {
        const float2 xy = c[p];
        const float x = sample(pm, h, w, bilin(xy.x, xy.y, h, w));
        xs[p] = x;
        sp += fmaxf(x, 0.f) + log1pf(__expf(-fabsf(x)));          // softplus(x)
        sg_sum += 1.f / (1.f + __expf(-x));
    }
    sp = block_sum(sp, red);
    sg_sum = block_sum(sg_sum, red);                               // (block_sum's barriers publish xs)
    if (CLIP && threadIdx.x == 0) { out[0] = sp; out[1] = sg_sum; }
    for (int tb = 0; tb < Tn; tb += kTT) {
        float ax[kTT], as[kTT], at[kTT];
#pragma unroll
        for (int j = 0; j < kTT; ++j) { ax[j] = 0.f; as[j] = 0.f; at[j] = 0.f; }
        for (int p = threadIdx.x; p < P; p += kThreads) {
            const float x = xs[p];
            const float sg = 1.f / (1.f + __expf(-x));
#pragma unroll
            for (int j = 0; j < kTT; ++j) {
                if (tb + j < Tn) {
                    const float tv = ts[(int64_t)(T0 + tb + j) * t_len + p];
                    ax[j] += x * tv; as[j] += sg * tv; at[j] += tv;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kTT; ++j) {
            const float sx = block_sum(ax[j], red), ss = block_sum(as[j], red), st = block_sum(at[j], red);
            if (threadIdx.x == 0 && tb + j < Tn) {
                if (CLIP) {
                    float* o = out + 2 + 3 * (tb + j);
                    o[0] = sx; o[1] = ss; o[2] = st;
                } else {
                    const float cm = (sp - sx) / (float)P;
                    const float cd = 1.f - (2.f * ss + 1.f) / (sg_sum + st + 1.f);
                    out[tb + j] = w_mask * cm + w_dice * cd;
                }
            }
        }
    }
}

// cost[row, t] from the per-frame sums of the two CLIP kernels: frames added in index order, then the image form's formulas with
// F * P points.  One thread per (row, t); t >= t_count[row] is left untouched.
__global__ __launch_bounds__(kThreads) void match_cost_clip_fold_kernel(
    const float* __restrict__ partial, const int32_t* __restrict__ t_count, float* __restrict__ cost,
    int n_rows, int F, int Tmax, int P, float w_mask, float w_dice)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (int64_t)n_rows * Tmax) return;
    const int row = (int)(i / Tmax), t = (int)(i - (int64_t)row * Tmax);
    if (t >= t_count[row]) return;
    const int W = clip_partial_floats(Tmax);
    const float* p = partial + (int64_t)row * F * W;
    float sp = 0.f, sg = 0.f, sx = 0.f, ss = 0.f, st = 0.f;
    for (int f = 0; f < F; ++f, p += W) {
        sp += p[0]; sg += p[1];
        sx += p[2 + 3 * t]; ss += p[3 + 3 * t]; st += p[4 + 3 * t];
    }
    const float cm = (sp - sx) / ((float)F * (float)P);
    const float cd = 1.f - (2.f * ss + 1.f) / (sg + st + 1.f);
    cost[i] = w_mask * cm + w_dice * cd;
}

}  // namespace

// ------------------------------------------------------------------------------------------------
// Matching cost with the prediction plane staged in LDS.  The samples of a row are 4 x P random 2-byte
// gathers from a 128 KB plane — from L2 that is the whole cost of the kernel above; from LDS it is
// noise.  One workgroup takes G consecutive rows that share their point set and targets (the queries of
// one (output, image)): for each row the plane is copied into LDS with 16-byte loads and sampled (the
// samples and their sigmoids stay in registers, PT points per thread), then the target samples are
// streamed ONCE for the G rows.  fp32 throughout; block reductions by wave shuffles + one LDS pass.
// ------------------------------------------------------------------------------------------------
// global -> LDS copy of a plane by a 1024-thread workgroup: all loads of a thread are issued before its
// first LDS store (a load-store-load-store loop exposes one memory latency per 16 KiB)
template <int THREADS = 1024>
__device__ __forceinline__ void copy_plane_to_lds(void* lds_plane, const void* src_plane, int plane_bytes, int tid)
{
    const uint4* src = reinterpret_cast<const uint4*>(src_plane);
    uint4* dst = reinterpret_cast<uint4*>(lds_plane);
    const int n16 = plane_bytes / 16;
    for (int base = 0; base < n16; base += 8 * THREADS) {
        uint4 t[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int idx = base + tid + k * THREADS;
            t[k] = idx < n16 ? src[idx] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int idx = base + tid + k * THREADS;
            if (idx < n16) dst[idx] = t[k];
        }
    }
}

template <typename T>
__device__ __forceinline__ float sample_lds(const T* plane, int h, int w, const Bilin& b)
{
    const bool x0v = b.x0 >= 0 && b.x0 < w, x1v = b.x0 + 1 >= 0 && b.x0 + 1 < w;
    const bool y0v = b.y0 >= 0 && b.y0 < h, y1v = b.y0 + 1 >= 0 && b.y0 + 1 < h;
    const int o = b.y0 * w + b.x0;
    const float v00 = (y0v && x0v) ? ld(plane, o) : 0.f;
    const float v01 = (y0v && x1v) ? ld(plane, o + 1) : 0.f;
    const float v10 = (y1v && x0v) ? ld(plane, o + w) : 0.f;
    const float v11 = (y1v && x1v) ? ld(plane, o + w + 1) : 0.f;
    const float hx = 1.f - b.lx, hy = 1.f - b.ly;
    return hy * (hx * v00 + b.lx * v01) + b.ly * (hx * v10 + b.lx * v11);
}

// sum over the 64 lanes with DPP row operations (VALU cross-lane moves; __shfl_xor lowers to ds_bpermute
// = an LDS instruction + a wait per step) and two v_readlane
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_add_(float v)
{
    const int t = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, true);
    return v + __int_as_float(t);
}
__device__ __forceinline__ float wave_sum64(float v)
{
    v = dpp_add_<0xB1>(v);          // quad_perm [1,0,3,2]
    v = dpp_add_<0x4E>(v);          // quad_perm [2,3,0,1]
    v = dpp_add_<0x141>(v);         // row_half_mirror
    v = dpp_add_<0x140>(v);         // row_mirror: every lane = sum of its row of 16
    v = dpp_add_<0x142, 0xa>(v);    // row_bcast15 into rows 1 and 3: lanes 16..31 / 48..63 = sums of the 32-lane halves
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 31)) + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// CLIP: workgroup (x, f) stages frame f of its rows and writes the per-frame sums (see match_cost_kernel); a run of `rpg` rows
// that share their point set is cut into ceil(rpg / G) workgroups, the last one of a run taking the rows that are left.
template <typename T, int G, int PT, int THREADS, bool CLIP>
__global__ __launch_bounds__(THREADS) void match_cost_lds_kernel(
    const T* __restrict__ pred, int h, int w, const int64_t* __restrict__ pred_offs,
    const float* __restrict__ coords, const int32_t* __restrict__ coord_rows,
    const float* __restrict__ tsamp, const int32_t* __restrict__ t_first, const int32_t* __restrict__ t_count,
    float* __restrict__ cost, int n_rows, int Tmax, int P, float w_mask, float w_dice, int plane_bytes,
    int64_t stride_f, float* __restrict__ partial, int rpg)
{
    constexpr int TT = 4;                       // targets per pass
    constexpr int NV = 2 * G * TT + TT;         // values reduced per pass
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* plane = reinterpret_cast<T*>(smem);
    float* red = reinterpret_cast<float*>(smem + plane_bytes);       // [16 waves][NV]
    int row0 = blockIdx.x * G, left = n_rows - row0;
    if (CLIP) {
        const int per = (rpg + G - 1) / G, run = blockIdx.x / per, sub = blockIdx.x - run * per;
        row0 = run * rpg + sub * G;
        left = rpg - sub * G;
    }
    const int f = CLIP ? blockIdx.y : 0, F = CLIP ? gridDim.y : 1;
    const int Tn = t_count[row0];
    if (Tn == 0) return;
    const int T0 = t_first[row0];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float2* c = reinterpret_cast<const float2*>(coords) + (int64_t)coord_rows[row0] * P;
    const int ng = min(G, left);
    const int64_t t_len = (int64_t)F * P;              // floats per target row
    const float* ts = tsamp + (int64_t)f * P;

    float2 xy[PT];
#pragma unroll
    for (int j = 0; j < PT; ++j) {
        const int p = tid + j * THREADS;
        xy[j] = p < P ? c[p] : make_float2(-4.f, -4.f);          // far outside: samples 0
    }
    float xs[G][PT];            // (the sigmoids are recomputed per target pass: 1024 threads leave 128 VGPRs per lane)
    float sp[G], sgs[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        sp[g] = 0.f; sgs[g] = 0.f;
        __syncthreads();
        if (g < ng) copy_plane_to_lds<THREADS>(plane, pred + pred_offs[row0 + g] + f * stride_f, plane_bytes, tid);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PT; ++j) {
            const bool valid = (tid + j * THREADS < P) && g < ng;
            const float x = valid ? sample_lds(plane, h, w, bilin(xy[j].x, xy[j].y, h, w)) : 0.f;
            const float s_ = 1.f / (1.f + __expf(-x));
            xs[g][j] = x;                                        // (0 for padding points)
            if (valid) {
                sp[g] += fmaxf(x, 0.f) + __logf(1.f + __expf(-fabsf(x)));       // softplus; |error| <= 6e-8 per point
                sgs[g] += s_;
            }
        }
    }
    // softplus / sigmoid sums of each row
    __syncthreads();
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float a = wave_sum64(sp[g]), b = wave_sum64(sgs[g]);
        if (lane == 0) { red[wave * NV + 2 * g] = a; red[wave * NV + 2 * g + 1] = b; }
    }
    __syncthreads();
    float sp_tot = 0.f, sg_tot = 0.f;          // needed by the threads that finalise (tid < G*TT): row g = tid / TT
    {
        const int g = min(tid / TT, G - 1);
#pragma unroll
        for (int k = 0; k < THREADS / 64; ++k) { sp_tot += red[k * NV + 2 * g]; sg_tot += red[k * NV + 2 * g + 1]; }
    }
    for (int tb = 0; tb < Tn; tb += TT) {
        float ax[G][TT], as_[G][TT], at[TT];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
            at[tt] = 0.f;
#pragma unroll
            for (int g = 0; g < G; ++g) { ax[g][tt] = 0.f; as_[g][tt] = 0.f; }
        }
        // 5 points x TT targets of loads in flight at a time (all PT x TT at once would spill ~200 registers)
        constexpr int JC = 5;
#pragma unroll
        for (int jc = 0; jc < PT; jc += JC) {
            float tv[JC][TT];
#pragma unroll
            for (int jj = 0; jj < JC; ++jj) {
                const int j = jc + jj;
                const int p = min(tid + j * THREADS, P - 1);
                // unconditional loads (indices clamped, values masked below): a load behind a run-time condition
                // makes hipcc wait for each one separately — 100 dependent L2 round trips per pass
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) tv[jj][tt] = ts[(int64_t)(T0 + min(tb + tt, Tn - 1)) * t_len + p];
            }
#pragma unroll
            for (int jj = 0; jj < JC; ++jj) {
                const int j = jc + jj;
                if (j < PT) {
                    const bool pv = tid + j * THREADS < P;         // padding point: its target value counts as 0
                    float sgv[G];
#pragma unroll
                    for (int g = 0; g < G; ++g) sgv[g] = __frcp_rn(1.f + __expf(-xs[g][j]));
#pragma unroll
                    for (int tt = 0; tt < TT; ++tt) {
                        const float t_ = pv ? tv[jj][tt] : 0.f;
                        at[tt] += t_;
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            ax[g][tt] += xs[g][j] * t_;
                            as_[g][tt] += sgv[g] * t_;
                        }
                    }
                }
            }
            asm volatile("" ::: "memory");       // keep the next chunk's loads behind this chunk's arithmetic
        }
        __syncthreads();                        // previous pass's red[] fully consumed
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
            const float v = wave_sum64(at[tt]);
            if (lane == 0) red[wave * NV + 2 * G * TT + tt] = v;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float a = wave_sum64(ax[g][tt]), b = wave_sum64(as_[g][tt]);
                if (lane == 0) { red[wave * NV + (g * TT + tt) * 2] = a; red[wave * NV + (g * TT + tt) * 2 + 1] = b; }
            }
        }
        __syncthreads();
        if (tid < G * TT) {
            const int g = tid / TT, tt = tid - g * TT;
            if (g < ng && tb + tt < Tn) {
                float sx = 0.f, ss = 0.f, st = 0.f;
#pragma unroll
                for (int k = 0; k < THREADS / 64; ++k) {
                    sx += red[k * NV + (g * TT + tt) * 2];
                    ss += red[k * NV + (g * TT + tt) * 2 + 1];
                    st += red[k * NV + 2 * G * TT + tt];
                }
                if (CLIP) {
                    float* o = partial + ((int64_t)(row0 + g) * F + f) * clip_partial_floats(Tmax);
                    if (tb + tt == 0) { o[0] = sp_tot; o[1] = sg_tot; }
                    o += 2 + 3 * (tb + tt);
                    o[0] = sx; o[1] = ss; o[2] = st;
                } else {
                    const float cm = (sp_tot - sx) / (float)P;
                    const float cd = 1.f - (2.f * ss + 1.f) / (sg_tot + st + 1.f);
                    cost[(int64_t)(row0 + g) * Tmax + tb + tt] = w_mask * cm + w_dice * cd;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Importance sampling in one kernel (criterion.py:164-170 + detectron2
// get_uncertain_point_coords_with_randomness): sample the M = 3P candidate points of a prediction
// plane and keep the k with the smallest |logit|.  One workgroup per (prediction, target) pair: the
// 128 KB bf16 plane is copied into LDS and sampled from there, the |logit| keys never leave the
// registers (PT per thread, point p = tid + 1024 j), the k-th smallest key is found by an MSB-first
// 8-bit radix select on an LDS histogram, and the selected coordinates are emitted in index order
// (ties at the threshold broken by index) from wave ballots + one scan of the per-(j, wave) counts.
// Replaces point_sample (60 MB of logits written and read back) + select_uncertain.
// ------------------------------------------------------------------------------------------------
template <typename T, int PT>
__global__ __launch_bounds__(kMcThreads) void sample_select_kernel(
    const T* __restrict__ pred, int h, int w, const int64_t* __restrict__ pred_offs,
    const float* __restrict__ coords_in, float* __restrict__ coords_out, int M, int k, int P_out, int plane_bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* plane = reinterpret_cast<T*>(smem);
    int* hist = reinterpret_cast<int*>(smem + plane_bytes);           // [256]
    int* cnt = hist + 256;                                             // [2][PT][16] less / equal counts per (j, wave)
    int* misc = cnt + 2 * PT * 16;                                     // [0] prefix, [1] krem, [2] total less
    const int row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float2* cin = reinterpret_cast<const float2*>(coords_in) + (int64_t)row * M;
    float2* cout = reinterpret_cast<float2*>(coords_out) + (int64_t)row * P_out;
    copy_plane_to_lds(plane, pred + pred_offs[row], plane_bytes, tid);
    if (tid == 0) { misc[0] = 0; misc[1] = k; }
    __syncthreads();
    unsigned key[PT];
    // (The coordinate loads stay behind `if (p < M)`, one dependent round trip each: every unconditional form measured in round
    // 3 — batches of 2..8 on clamped indices, buffer loads with the point stride as scalar offset, scheduling barriers between
    // batches — made hipcc spill ~240 registers at the 128 VGPRs of a 1024-thread workgroup: 172 -> 280 us.)
#pragma unroll
    for (int j = 0; j < PT; ++j) {
        const int p = tid + j * kMcThreads;
        key[j] = 0xFFFFFFFFu;                                          // past the end: never selected (k <= M)
        if (p < M) {
            const float2 xy = cin[p];
            key[j] = __float_as_uint(fabsf(sample_lds(plane, h, w, bilin(xy.x, xy.y, h, w))));
        }
    }
    unsigned prefix = 0u, mask = 0u;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        prefix = (unsigned)misc[0];
#pragma unroll
        for (int j = 0; j < PT; ++j)
            if (tid + j * kMcThreads < M && (key[j] & mask) == prefix) atomicAdd(&hist[(key[j] >> shift) & 255u], 1);
        __syncthreads();
        const int krem = misc[1];
        // exclusive prefix of the 256 digit counts: wave scan (threads 0..255 = 4 waves) + the sums of the lower waves
        // (a per-thread loop `for d < tid` was up to 255 dependent LDS reads on the critical path of every pass)
        int below = 0, mine = 0;
        if (tid < 256) {
            mine = hist[tid];
            int incl = mine;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            if (lane == 63) misc[4 + wave] = incl;
            below = incl - mine;
        }
        __syncthreads();                                               // everyone has read misc[1] / hist; wave sums published
        if (tid < 256) {
            for (int wv = 0; wv < wave; ++wv) below += misc[4 + wv];
            if (below < krem && krem <= below + mine) {                // exactly one digit holds the k-th key
                misc[1] = krem - below;
                misc[0] = (int)(prefix | ((unsigned)tid << shift));
            }
        }
        mask |= 255u << shift;
        __syncthreads();
    }
    const unsigned thr = (unsigned)misc[0];
    const int need_eq = misc[1];
    // per-(j, wave) counts -> exclusive offsets in index order p = tid + 1024 j  (j major, then wave, then lane)
#pragma unroll
    for (int j = 0; j < PT; ++j) {
        const bool in = tid + j * kMcThreads < M;
        const unsigned long long bl = __ballot(in && key[j] < thr), be = __ballot(in && key[j] == thr);
        if (lane == 0) { cnt[j * 16 + wave] = __popcll(bl); cnt[PT * 16 + j * 16 + wave] = __popcll(be); }
    }
    __syncthreads();
    if (wave < 2) {                                                    // wave 0 scans the "less" counts, wave 1 the "equal" counts
        int* c = cnt + wave * PT * 16;
        constexpr int N = PT * 16, PER = (N + 63) / 64;
        int loc[PER], tot = 0;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int idx = lane * PER + i;
            loc[i] = idx < N ? c[idx] : 0;
            tot += loc[i];
        }
        int incl = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        int run = incl - tot;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int idx = lane * PER + i;
            if (idx < N) c[idx] = run;
            run += loc[i];
        }
        if (wave == 0 && lane == 63) misc[2] = incl;                   // total number of keys below the threshold
    }
    __syncthreads();
    const int tot_less = misc[2];
    const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < PT; ++j) {
        const int p = tid + j * kMcThreads;
        const bool less = p < M && key[j] < thr, eq = p < M && key[j] == thr;
        const unsigned long long bl = __ballot(less), be = __ballot(eq);
        if (less) {
            cout[cnt[j * 16 + wave] + __popcll(bl & lt)] = cin[p];
        } else if (eq) {
            const int rank = cnt[PT * 16 + j * 16 + wave] + __popcll(be & lt);
            if (rank < need_eq) cout[tot_less + rank] = cin[p];
        }
    }
}

// mask_loss_fwd with the prediction plane staged in LDS (bf16 planes of at most 128 KiB): one workgroup per
// pair, all P points; partial[i, 0, :] receives the sums, the other chunks zeros
template <bool BITS>
__global__ __launch_bounds__(kMcThreads) void mask_loss_fwd_lds_kernel(
    const __hip_bfloat16* __restrict__ pred, int h, int w, const int64_t* __restrict__ pred_offs,
    const void* __restrict__ gt, int H, int W, const int32_t* __restrict__ gt_rows,
    const float* __restrict__ coords, float* __restrict__ partial, int P, int chunks, int plane_bytes)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __hip_bfloat16* plane = reinterpret_cast<__hip_bfloat16*>(smem);
    float* red = reinterpret_cast<float*>(smem + plane_bytes);          // [16 waves][4]
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    copy_plane_to_lds(plane, pred + pred_offs[i], plane_bytes, tid);
    const GtPlane<BITS> gm(gt, gt_rows[i], H, W);
    const float2* c = reinterpret_cast<const float2*>(coords) + (int64_t)i * P;
    __syncthreads();
    float s_bce = 0.f, s_pt = 0.f, s_p = 0.f, s_t = 0.f;
    for (int p = tid; p < P; p += kMcThreads) {
        const float2 xy = c[p];
        const float x = sample_lds(plane, h, w, bilin(xy.x, xy.y, h, w));
        const float t = gm.at(H, W, bilin(xy.x, xy.y, H, W));
        const float sg = 1.f / (1.f + __expf(-x));
        s_bce += fmaxf(x, 0.f) - x * t + log1pf(__expf(-fabsf(x)));
        s_pt += sg * t;
        s_p += sg;
        s_t += t;
    }
    s_bce = wave_sum64(s_bce); s_pt = wave_sum64(s_pt); s_p = wave_sum64(s_p); s_t = wave_sum64(s_t);
    if (lane == 0) { red[wave * 4] = s_bce; red[wave * 4 + 1] = s_pt; red[wave * 4 + 2] = s_p; red[wave * 4 + 3] = s_t; }
    __syncthreads();
    if (tid < 4 * chunks) {
        float v = 0.f;
        if (tid < 4)
            for (int k = 0; k < kMcThreads / 64; ++k) v += red[k * 4 + tid];
        partial[(int64_t)i * chunks * 4 + tid] = v;
    }
}

// ---- entry points (loss_host.h: record, check, routes, launcher) ------------------------------------------------------------------
namespace {

using bf16 = __hip_bfloat16;

// loss_begin: the profiler's start and the name of the kernel the route chose; loss_done: unless the launcher failed (e), the
// profiler's record of that launch and its status
hipStream_t loss_begin(void* stream, const char* kernel)
{
    mpf::prof_begin((hipStream_t)stream);
    mpf::set_kernel(kernel);
    return (hipStream_t)stream;
}
int loss_done(const char* who, hipStream_t st, double bytes, int e = 0)
{
    if (e) return e;
    mpf::prof_end(mpf_last_kernel(), st, bytes);
    return mpf::check(hipGetLastError(), who);
}

// both forms of the matching cost: p.F == 0 is the image form (no workspace, the kernels write the cost themselves)
int match_cost(const char* who, const LossProblem& p, const void* pred, const int64_t* pred_offs, const float* coords, const int32_t* coord_rows,
               const float* tsamp, const int32_t* t_first, const int32_t* t_count, float* cost, float w_mask, float w_dice, float* partial, void* stream)
{
    const LossRoute route = match_cost_route(p);
    const bool lds = route == LossRoute::lds;
    const char* const names[2][2] = {{p.pick("match_cost_kernel<float>", "match_cost_kernel<bf16>"), "match_cost_lds_kernel<bf16>"},
                                     {p.pick("match_cost_clip_kernel<float>", "match_cost_clip_kernel<bf16>"), "match_cost_clip_lds_kernel<bf16>"}};
    hipStream_t st = loss_begin(stream, names[p.F > 0][lds]);
    int e = 0;
    mpf::with_bool(p.F > 0, [&](auto clip) { with_map_type(p.dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        constexpr bool CLIP = decltype(clip)::value;
        if (lds)
            e = launch_lds<match_cost_lds_kernel<bf16, kCostRows, kCostPT, kCostThreads, CLIP>>(
                p.cost_lds_grid(), kCostThreads, p.cost_lds(), st, (const bf16*)pred, p.h, p.w, pred_offs, coords, coord_rows, tsamp, t_first,
                t_count, cost, p.n, p.Tmax, p.P, w_mask, w_dice, (int)p.plane_bytes(), p.stride_f, partial, p.G);
        else
            e = launch_lds<match_cost_kernel<T, CLIP>, kDefaultLds>(
                p.cost_grid(), kThreads, p.xs_bytes(), st, (const T*)pred, p.h, p.w, pred_offs, coords, coord_rows, tsamp, t_first, t_count, cost,
                p.Tmax, p.P, w_mask, w_dice, p.stride_f, partial);
    }); });
    if (e || !p.F) return loss_done(who, st, p.bytes(route), e);
    if (int e2 = mpf::check(hipGetLastError(), who)) return e2;
    hipLaunchKernelGGL(match_cost_clip_fold_kernel, p.fold_grid(), dim3(kThreads), 0, st, partial, t_count, cost, p.n, p.F, p.Tmax, p.P,
                       w_mask, w_dice);
    return loss_done(who, st, p.bytes());
}

}  // namespace

extern "C" int mpf_point_sample(const void* src, int src_dtype, int h, int w, const int64_t* rows, const float* coords, const int32_t* coord_rows,
                                float* out, int n, int P, void* stream)
{
    const LossProblem p(LossEntry::point_sample, src_dtype, h, w, n, P);
    if (int e = loss_check("mpf_point_sample", p, {src, rows, coords, out}); e || p.empty()) return e;
    const bool bits = src_dtype == MPF_BITS;                                  // rows[] are then PIXEL indices of the planes' first pixel
    hipStream_t st = loss_begin(stream, bits ? "point_sample_bits_kernel" : src_dtype == MPF_U8 ? "point_sample_kernel<u8>"
                                                                          : p.pick("point_sample_kernel<float>", "point_sample_kernel<bf16>"));
    const dim3 grid = p.sample_grid(), block(kThreads);
    if (bits)
        hipLaunchKernelGGL(point_sample_bits_kernel, grid, block, 0, st, (const uint32_t*)src, h, w, rows, coords, coord_rows, out, n, P);
    else
        with_map_type<true>(src_dtype, [&](auto t) {
            using T = typename decltype(t)::type;
            hipLaunchKernelGGL(point_sample_kernel<T>, grid, block, 0, st, (const T*)src, h, w, rows, coords, coord_rows, out, n, P);
        });
    return loss_done("mpf_point_sample", st, p.bytes());
}

extern "C" int mpf_pack_mask_bits(const uint8_t* masks, void* bits, int64_t n_pixels, void* stream)
{
    if (mpf::any_null({masks, bits})) return mpf::failf(MPF_E_NULL, "pack_mask_bits", "NULL buffer");
    if (n_pixels < 0 || n_pixels % 32 != 0) return mpf::failf(MPF_E_SHAPE, "pack_mask_bits", "pixel count must be a multiple of 32");
    if (n_pixels == 0) return 0;
    const int64_t nwords = n_pixels / 32, want = (nwords + kThreads - 1) / kThreads;
    mpf::set_kernel("pack_mask_bits_kernel");
    hipLaunchKernelGGL(pack_mask_bits_kernel, dim3((int)(want < 4096 ? want : 4096)), dim3(kThreads), 0, (hipStream_t)stream, masks,
                       (uint32_t*)bits, nwords);
    return mpf::check(hipGetLastError(), "mpf_pack_mask_bits");
}

extern "C" int mpf_mask_loss_forward(const void* pred, int pred_dtype, int h, int w, const int64_t* pred_rows, const void* gt, int gt_dtype, int H,
                                     int W, const int32_t* gt_rows, const float* coords, float* partial, int n, int P, int chunks, void* stream)
{
    LossProblem p(LossEntry::forward, pred_dtype, h, w, n, P);
    p.H = H; p.W = W; p.gt_dtype = gt_dtype; p.chunks = chunks;
    if (int e = loss_check("mpf_mask_loss_forward", p, {pred, pred_rows, coords, partial}, {gt, gt_rows}); e || p.empty()) return e;
    const LossRoute route = mask_loss_fwd_route(p);
    const bool lds = route == LossRoute::lds;
    hipStream_t st = loss_begin(stream, lds ? "mask_loss_fwd_lds_kernel" : p.pick("mask_loss_fwd_kernel<float>", "mask_loss_fwd_kernel<bf16>"));
    int e = 0;
    with_map_type(pred_dtype, [&](auto t) { mpf::with_bool(p.bits(), [&](auto b) {
        using T = typename decltype(t)::type;
        constexpr bool BITS = decltype(b)::value;
        if (lds)
            e = launch_lds<mask_loss_fwd_lds_kernel<BITS>>(dim3(n), kMcThreads, p.fwd_lds(), st, (const bf16*)pred, h, w, pred_rows, gt, H, W,
                                                          gt_rows, coords, partial, P, chunks, (int)p.plane_bytes());
        else
            hipLaunchKernelGGL((mask_loss_fwd_kernel<T, BITS>), p.fwd_grid(), dim3(kThreads), 0, st, (const T*)pred, h, w, pred_rows, gt, H, W,
                               gt_rows, coords, partial, n, P, chunks);
    }); });
    return loss_done("mpf_mask_loss_forward", st, p.bytes(route), e);
}

extern "C" int mpf_mask_loss_backward(const void* pred, int pred_dtype, int h, int w, const int64_t* pred_rows, const uint8_t* gt, int H, int W,
                                      const int32_t* gt_rows, const float* coords, const float* grad_sums, float* grad_pred,
                                      const int64_t* grad_offs, int n, int P, void* stream)
{
    LossProblem p(LossEntry::backward, pred_dtype, h, w, n, P);
    p.H = H; p.W = W;
    const int bad = loss_check("mpf_mask_loss_backward", p, {pred, pred_rows, coords, grad_pred}, {gt, gt_rows, grad_sums, grad_offs});
    if (bad || p.empty()) return bad;
    hipStream_t st = loss_begin(stream, p.pick("mask_loss_bwd_kernel<float>", "mask_loss_bwd_kernel<bf16>"));
    with_map_type(pred_dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL(mask_loss_bwd_kernel<T>, p.bwd_grid(), dim3(kThreads), 0, st, (const T*)pred, h, w, pred_rows, gt, H, W, gt_rows, coords,
                           grad_sums, grad_pred, grad_offs, n, P);
    });
    return loss_done("mpf_mask_loss_backward", st, p.bytes());
}

extern "C" int mpf_mask_loss_backward_dense(const void* pred, int pred_dtype, int h, int w, const int64_t* pred_rows, const void* gt, int gt_dtype,
                                            int H, int W, const int32_t* gt_rows, const float* coords, const float* grad_sums, void* grad,
                                            int grad_dtype, const int64_t* grad_offs, int n, int P, void* stream)
{
    LossProblem p(LossEntry::backward_dense, pred_dtype, h, w, n, P);
    p.H = H; p.W = W; p.gt_dtype = gt_dtype; p.grad_dtype = grad_dtype;
    const int bad = loss_check("mpf_mask_loss_backward_dense", p, {pred, pred_rows, coords, grad}, {gt, gt_rows, grad_sums, grad_offs});
    if (bad || p.empty()) return bad;
    hipStream_t st = loss_begin(stream, p.pick("mask_loss_bwd_band_kernel<float>", "mask_loss_bwd_band_kernel<bf16>"));
    int e = 0;
    with_map_type(pred_dtype, [&](auto t) { mpf::with_bool(p.bits(), [&](auto b) {
        using T = typename decltype(t)::type;
        e = launch_lds<mask_loss_bwd_band_kernel<T, T, decltype(b)::value>>(
            p.band_grid(), kBandThreads, p.band_lds(), st, (const T*)pred, h, w, pred_rows, gt, H, W, gt_rows, coords, grad_sums, (T*)grad,
            grad_offs, n, P, p.band_rows());
    }); });
    return loss_done("mpf_mask_loss_backward_dense", st, p.bytes(), e);
}

extern "C" int mpf_select_uncertain(const float* vals, const float* coords_in, float* coords_out, int n, int M, int k, int P_out, void* stream)
{
    LossProblem p(LossEntry::select, MPF_F32, 1, 1, n);
    p.M = M; p.k = k; p.P_out = P_out;
    if (int e = loss_check("mpf_select_uncertain", p, {vals, coords_in, coords_out}); e || p.empty()) return e;
    hipStream_t st = loss_begin(stream, "select_uncertain_kernel");
    hipLaunchKernelGGL(select_uncertain_kernel, dim3(n), dim3(kSelThreads), 0, st, vals, coords_in, coords_out, M, k, P_out);
    return loss_done("mpf_select_uncertain", st, p.bytes());
}

extern "C" int mpf_sample_select_uncertain(const void* pred, int pred_dtype, int h, int w, const int64_t* pred_offs, const float* coords_in,
                                           float* coords_out, int n, int M, int k, int P_out, void* stream)
{
    LossProblem p(LossEntry::sample_select, pred_dtype, h, w, n);
    p.M = M; p.k = k; p.P_out = P_out;
    if (int e = loss_check("mpf_sample_select_uncertain", p, {pred, pred_offs, coords_in, coords_out}); e || p.empty()) return e;
    hipStream_t st = loss_begin(stream, "sample_select_kernel<bf16>");
    int e = 0;
    mpf::with_int_of<16, 37, 40>(sample_select_pt(M), [&](auto pt) {
        constexpr int PT = decltype(pt)::value;
        e = launch_lds<sample_select_kernel<bf16, PT>>(dim3(n), kMcThreads, p.select_lds(PT), st, (const bf16*)pred, h, w, pred_offs, coords_in,
                                                       coords_out, M, k, P_out, (int)p.plane_bytes());
    });
    return loss_done("mpf_sample_select_uncertain", st, p.bytes(), e);
}

extern "C" int mpf_match_cost(const void* pred, int pred_dtype, int h, int w, const int64_t* pred_offs, const float* coords,
                              const int32_t* coord_rows, const float* tsamp, const int32_t* t_first, const int32_t* t_count, float* cost,
                              int n_rows, int Tmax, int P, float w_mask, float w_dice, int rows_per_group, void* stream)
{
    LossProblem p(LossEntry::cost, pred_dtype, h, w, n_rows, P);
    p.Tmax = Tmax; p.G = rows_per_group;
    if (int e = loss_check("mpf_match_cost", p, {pred, pred_offs, coords, coord_rows, tsamp, t_first, t_count, cost}); e || p.empty()) return e;
    return match_cost("mpf_match_cost", p, pred, pred_offs, coords, coord_rows, tsamp, t_first, t_count, cost, w_mask, w_dice, nullptr, stream);
}

extern "C" size_t mpf_match_cost_clip_workspace_bytes(int n_rows, int F, int Tmax)
{
    LossProblem p(LossEntry::cost_clip, MPF_BF16, 1, 1, n_rows);
    p.F = F; p.Tmax = Tmax;
    return p.workspace_bytes();
}

extern "C" int mpf_match_cost_clip(const void* pred, int pred_dtype, int h, int w, const int64_t* pred_offs, int F, int64_t stride_f,
                                   const float* coords, const int32_t* coord_rows, const float* tsamp, const int32_t* t_first,
                                   const int32_t* t_count, float* cost, int n_rows, int Tmax, int P, float w_mask, float w_dice,
                                   int rows_per_group, void* workspace, size_t workspace_bytes, void* stream)
{
    LossProblem p(LossEntry::cost_clip, pred_dtype, h, w, n_rows, P);
    p.F = F; p.stride_f = stride_f; p.Tmax = Tmax; p.G = rows_per_group;
    const int bad = loss_check("mpf_match_cost_clip", p, {pred, pred_offs, coords, coord_rows, tsamp, t_first, t_count, cost}, {}, workspace, workspace_bytes);
    if (bad || p.empty()) return bad;
    float* partial = (float*)workspace;
    return match_cost("mpf_match_cost_clip", p, pred, pred_offs, coords, coord_rows, tsamp, t_first, t_count, cost, w_mask, w_dice, partial, stream);
}

